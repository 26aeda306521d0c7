"""GPU: bench.py --dump-outputs writes what the timed rounds computed.  A
small config-4 cluster through bench.main itself (pre-roll, warmup, timed
rounds, dump), against the oracle run for the same rounds: checksums, the
sampled views and the timed rounds' counters, bit for bit; and a plain run's
line carries the headline without the --full sections."""
import json
import os

import numpy as np
import pytest

import bench
import oracle

pytestmark = pytest.mark.gpu

N, SEED, CHURN, PREROLL, WARMUP, STEPS = 300, 2024, 3, 4, 1, 3  # (ceil(1 % of 300) = 3 re-assertions per round)


def test_dump_outputs_match_the_oracle(gpu_lib, tmp_path, capsys):
    argv = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--preroll", str(PREROLL), "--nodes",
            str(N), "--seed", str(SEED), "--dump-outputs", str(tmp_path)]
    assert bench.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "member-updates/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    for key in ("stages", "box_ceiling", "clocks", "traffic_pmc", "observed_checksums", "config1", "config2",
                "config3", "config5", "cpu_baseline"):
        assert key not in line, key
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    c = oracle.Sim(N, SEED, churn_k=CHURN)
    want = dict.fromkeys(("evaluated", "applied", "full_syncs", "messages"), 0)
    for r in range(PREROLL + WARMUP + STEPS):
        st = c.round(churn=True)
        if r >= PREROLL + WARMUP:
            for key in want:
                want[key] += st[key]
    assert got["counters"][:4].tolist() == [want[k] for k in ("evaluated", "applied", "full_syncs", "messages")]
    # value = the timed rounds' evaluated changes / their time (ms_per_step is rounded to 1 us: within 1 %)
    assert abs(line["value"] * line["ms_per_step"] * STEPS / 1e3 / want["evaluated"] - 1) < 1e-2
    assert got["checksums"].tolist() == c.checksums()
    nodes = got["view_nodes"].astype(int)
    assert len(nodes) == 32 and (np.diff(nodes) > 0).all() and nodes[0] >= 0 and nodes[-1] < N
    alive = 0
    for i, v in enumerate(nodes):
        s, inc = c.view(int(v))
        assert np.array_equal(got["view_status"][i], s) and np.array_equal(got["view_incarnation"][i], inc), v
        alive += int((s == 1).sum())
    assert got["view_counts"].shape == (N, 6)
    assert got["view_counts"][nodes, 1].sum() == alive  # (column 1: alive members of each view)
    c.close()
