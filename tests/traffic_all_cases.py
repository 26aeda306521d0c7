"""Multi-key request traffic (rp_traffic_all_*): the model,
restated from the rules in include/ringpop_hip.h over the CPU oracle alone --
Sim.ring_lookup(v, h), Sim.info(v)["ring_checksum"], Sim.info(v)["dead"] and
route_cases.cut -- on traffic_cases' scenarios; everything is integer-exact."""
import functools

import numpy as np

import oracle
import route_cases as rc
import traffic_cases as tc

OUTCOMES = ("local", "delivered", "rerouted_local", "failed", "entry_dead", "aborted")
LOCAL, DELIVERED, REROUTED_LOCAL, FAILED, ENTRY_DEAD, ABORTED = range(6)
PENDING, NEVER = 255, 0xFFFFFFFF
STATS = ("requests", "requests_entry_dead", "requests_empty", "requests_ok", "requests_failed", "keys", "sends") + \
    OUTCOMES + ("proxied", "send_unreachable", "checksums_differ", "retry_scheduled", "retry_attempted",
                "retry_rerouted", "retry_succeeded", "retry_failed", "misrouted_keys")
SCENARIOS, DRAIN = tc.SCENARIOS, tc.DRAIN
K_CYCLE = (0, 1, 2, 3, 8, 33, 64, 65, 130, 256)
PER_ROUND = 40


class Model:
    """The tracker over a CPU oracle simulation `cpu`, whose round count the caller passes as `clock`."""

    def __init__(self, cpu, partition=None, max_retries=3, schedule=tc.DEFAULT_SCHEDULE, enforce_consistency=True):
        self.cpu, self.partition = cpu, partition
        self.max_retries, self.schedule, self.enforce = max_retries, tuple(schedule), enforce_consistency
        self.stats = dict.fromkeys(STATS, 0)
        self.by_retries = {k: [0] * tc.RETRY_SLOTS for k in OUTCOMES}
        self.pending = []   # requests with an open send: id, entry, submit_clock, first_error, sends
        self.results = []   # by id: (outcome, max_retries_seen, fanout, submit_clock, first_error_clock, done_clock)
        self.seen = set()   # what the default runs must contain (test_traffic_all_cpu.py)
        self._state_clock = None

    def _state(self, clock):
        if self._state_clock != clock:
            info = [self.cpu.info(v) for v in range(self.cpu.n)]
            self._dead = [i["dead"] != 0 for i in info]
            self._rcs = [i["ring_checksum"] for i in info]
            self._look = functools.lru_cache(maxsize=None)(self.cpu.ring_lookup)
            self._state_clock = clock

    def _lookup(self, v, h):
        d = self._look(v, h)
        return v if d < 0 else d  # (an empty ring: lookup falls back to whoami)

    def _advance(self, q, s, clock, attempt):
        """One send from its next event until it is final or due later."""
        e = q["entry"]

        def final(outcome, dest):
            s["outcome"], s["dest"] = outcome, dest
            self.stats[OUTCOMES[outcome]] += 1
            self.by_retries[OUTCOMES[outcome]][min(s["retries"], tc.RETRY_SLOTS - 1)] += 1
            if outcome >= FAILED and q["first_error"] == NEVER:
                q["first_error"] = clock

        target = s["first_dest"]
        while True:
            if not attempt:
                if self._dead[e]:
                    self.seen.add("entry_dead_at_retry")
                    return final(ENTRY_DEAD, -1)
                s["retries"] += 1
                owners = {self._lookup(e, h) for h in s["keys"]}
                if len(owners) > 1:
                    self.seen.add("aborted_2_keys" if len(s["keys"]) == 2 else "aborted")
                    if q["nkeys"] > 64:
                        self.seen.add("aborted_over_64")
                    return final(ABORTED, s["first_dest"])
                self.stats["retry_attempted"] += 1
                nd, = owners
                if nd != s["first_dest"]:
                    self.stats["retry_rerouted"] += 1
                    if len(s["keys"]) > 1:
                        self.seen.add("multi_rerouted_local" if nd == e else "multi_rerouted_remote")
                    if nd == e:
                        return final(REROUTED_LOCAL, e)
                self.stats["proxied"] += 1
                target = nd
            attempt, d = False, target
            if self._dead[d] or rc.cut(self.partition, clock, e, d):
                self.stats["send_unreachable"] += 1
                error = True
            else:
                differ = self._rcs[e] != self._rcs[d]
                self.stats["checksums_differ"] += differ
                error = differ and self.enforce
            if not error:
                self.stats["retry_succeeded"] += s["retries"] > 0
                self.stats["misrouted_keys"] += sum(1 for h in s["keys"] if self._look(d, h) != d)
                return final(DELIVERED, d)
            if s["retries"] >= self.max_retries:
                self.stats["retry_failed"] += self.max_retries > 0
                return final(FAILED, d)
            self.stats["retry_scheduled"] += 1
            s["due"] = clock + self.schedule[min(s["retries"], len(self.schedule) - 1)]
            if s["due"] > clock:
                return

    def _settle(self, q, clock):
        """The request's record; True when its last send is final."""
        ocs = [s["outcome"] for s in q["sends"]]
        done = PENDING not in ocs
        worst = max(ocs, default=LOCAL)
        self.results[q["id"]] = (worst if done else PENDING, max((s["retries"] for s in q["sends"]), default=0),
                                 len(ocs), q["submit_clock"], q["first_error"], clock if done else 0)
        if done:
            self.stats["requests_ok" if worst <= REROUTED_LOCAL else "requests_failed"] += 1
            if len(set(ocs)) > 1:
                self.seen.add("mixed_outcomes")
            if q["first_error"] < clock:
                self.seen.add("failed_before_done")
        return done

    def submit(self, clock, entries, offsets, keys):
        self._state(clock)
        keys = [int(h) for h in keys]
        for i, e in enumerate(int(x) for x in entries):
            hs = keys[int(offsets[i]):int(offsets[i + 1])]
            q = {"id": len(self.results), "entry": e, "nkeys": len(hs), "submit_clock": clock, "first_error": NEVER,
                 "sends": []}
            self.results.append(None)
            self.stats["requests"] += 1
            if self._dead[e]:
                self.stats["requests_entry_dead"] += 1
                self.stats["requests_failed"] += 1
                self.results[q["id"]] = (ENTRY_DEAD, 0, 0, clock, NEVER, clock)
                continue
            self.stats["requests_empty"] += not hs
            self.stats["keys"] += len(hs)
            groups = {}  # owner -> keys: insertion order is first appearance (_.groupBy)
            for h in hs:
                groups.setdefault(self._lookup(e, h), []).append(h)
            self.stats["sends"] += len(groups)
            for j, (d, ghs) in enumerate(groups.items()):
                s = {"group": j, "keys": ghs, "first_dest": d, "due": 0, "retries": 0, "outcome": PENDING, "dest": -1}
                q["sends"].append(s)
                if d == e:
                    s["outcome"], s["dest"] = LOCAL, e
                    self.stats["local"] += 1
                    self.by_retries["local"][0] += 1
                else:
                    self.stats["proxied"] += 1
                    self._advance(q, s, clock, True)
            if not self._settle(q, clock):
                self.pending.append(q)

    def poll(self, clock):
        self._state(clock)
        left = []
        for q in self.pending:
            due = [s for s in q["sends"] if s["outcome"] == PENDING and s["due"] <= clock]
            for s in due:
                self._advance(q, s, clock, False)
            if not due or not self._settle(q, clock):
                left.append(q)
                if q["nkeys"] > 64:
                    self.seen.add("over_64_survives_a_poll")
        self.pending = left


def snapshot(m):
    """What a GPU run is compared with after a step (copies)."""
    sends = [(q["id"], q["entry"], s["group"], len(s["keys"]), s["first_dest"], s["due"], q["submit_clock"], s["retries"])
             for q in m.pending for s in q["sends"] if s["outcome"] == PENDING]
    keys = [h for q in m.pending for s in q["sends"] if s["outcome"] == PENDING for h in s["keys"]]
    return {"stats": dict(m.stats), "by_retries": {k: list(v) for k, v in m.by_retries.items()}, "sends": sends,
            "keys": keys, "results": list(m.results)}


def batch(n, index, ks):
    """Batch `index` of the seed-11 stream: requests of ks[i] keys over consecutive draws, request i's entry the
    entry of its first draw: (entries, offsets, key_hashes)."""
    ks = np.asarray(ks, dtype=np.uint64)
    off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(ks, dtype=np.uint64)])
    T = int(off[-1])
    e, h = rc.requests(tc.REQ_SEED, (index + 1) * T, n)
    e, h = e[index * T:], h[index * T:]
    return e[np.minimum(off[:-1], T - 1).astype(np.int64)].copy(), off, h.copy()


def round_batch(n, r):
    """Round r's ragged batch: PER_ROUND requests whose K cycles through K_CYCLE."""
    return batch(n, r - 1, [K_CYCLE[i % len(K_CYCLE)] for i in range(PER_ROUND)])


def run_model(name, per_step=None, **cfg):
    """The scenario on the oracle (seed 7, churn on): after every round a poll, then the round's batch; then DRAIN
    rounds with polls only.  per_step(model, clock) is called after each step's calls.  Returns the model."""
    n, kw, rounds = SCENARIOS[name]
    cpu = oracle.Sim(n, tc.SIM_SEED, **kw)
    m = Model(cpu, kw.get("partition"), **cfg)
    for r in range(1, rounds + DRAIN + 1):
        cpu.round(churn=True)
        m.poll(r)
        if r <= rounds:
            m.submit(r, *round_batch(n, r))
        if per_step:
            per_step(m, r)
    cpu.close()
    m.cpu = None
    return m


@functools.lru_cache(maxsize=None)
def expected(name):
    """The default-configuration run of a scenario: (the final model, the snapshot after every step).  Computed
    once and shared; read-only."""
    snaps = []
    m = run_model(name, per_step=lambda mm, r: snaps.append(snapshot(mm)))
    return m, snaps
