"""Request traffic with proxy retries (rp_traffic_*): the scenarios and the
model, restated from DESIGN.md §11 and the CPU oracle alone.

The model uses three oracle calls -- Sim.ring_lookup(v, h),
Sim.info(v)["ring_checksum"] and Sim.info(v)["dead"] -- and route_cases' cut,
request and requests; everything is integer-exact."""
import functools

import oracle
import route_cases as rc

OUTCOMES = ("local", "delivered", "rerouted_local", "failed", "entry_dead")
LOCAL, DELIVERED, REROUTED_LOCAL, FAILED, ENTRY_DEAD = range(5)
PENDING = 255
STATS = ("submitted", "local", "delivered", "rerouted_local", "failed", "entry_dead", "proxied", "send_unreachable",
         "checksums_differ", "retry_scheduled", "retry_attempted", "retry_rerouted", "retry_succeeded", "retry_failed",
         "misrouted")
RETRY_SLOTS = 9
DEFAULT_SCHEDULE = (0, 5, 18)

SIM_SEED, REQ_SEED = rc.SIM_SEED, rc.REQ_SEED
PER_ROUND, DRAIN = 200, 30

# name -> (n, Sim keywords, rounds)
SCENARIOS = {k: rc.SCENARIOS[k][:3] for k in ("failstop", "partition", "shift")}
# entries that die while they wait for a retry
SCENARIOS["failstop_late"] = (96, {"failures": {2: [5, 40], 30: [41, 95], 33: [7]}}, 45)


class Model:
    """The tracker of DESIGN.md §11 over a CPU oracle simulation `cpu`, whose
    round count the caller passes as `clock`."""

    def __init__(self, cpu, partition=None, max_retries=3, schedule=DEFAULT_SCHEDULE, enforce_consistency=True):
        self.cpu, self.partition = cpu, partition
        self.max_retries, self.schedule, self.enforce = max_retries, tuple(schedule), enforce_consistency
        self.stats = dict.fromkeys(STATS, 0)
        self.history = {}  # clock -> the counts of calls made at it
        self.by_retries = {k: [0] * RETRY_SLOTS for k in OUTCOMES}
        self.pending = []  # dicts in submission order: id, entry, key_hash, first_dest, due, submit_clock, retries
        self.results = []  # by id: (dest, outcome, retries, submit_clock, done_clock), None while pending
        self._state_clock = None

    def _state(self, clock):
        if self._state_clock != clock:
            info = [self.cpu.info(v) for v in range(self.cpu.n)]
            self._dead = [i["dead"] != 0 for i in info]
            self._rcs = [i["ring_checksum"] for i in info]
            self._state_clock = clock

    def _count(self, clock, key):
        self.stats[key] += 1
        row = self.history.setdefault(clock, dict.fromkeys(STATS, 0))
        row[key] += 1

    def _lookup(self, v, h):
        d = self.cpu.ring_lookup(v, h)
        return v if d < 0 else d  # (an empty ring: lookup falls back to whoami)

    def _advance(self, q, clock, target):
        """Steps 2-5 for request q: a send to `target` is ready, or (None) a
        retry is due.  True when q is final."""
        e, h = q["entry"], q["key_hash"]

        def final(outcome, dest):
            self._count(clock, OUTCOMES[outcome])
            self.by_retries[OUTCOMES[outcome]][min(q["retries"], RETRY_SLOTS - 1)] += 1
            self.results[q["id"]] = (dest, outcome, q["retries"], q["submit_clock"], clock)
            return True

        while True:
            if target is None:
                if self._dead[e]:
                    return final(ENTRY_DEAD, -1)
                q["retries"] += 1
                self._count(clock, "retry_attempted")
                nd = self._lookup(e, h)
                if nd != q["first_dest"]:
                    self._count(clock, "retry_rerouted")
                    if nd == e:
                        return final(REROUTED_LOCAL, e)
                self._count(clock, "proxied")
                target = nd
            d, target = target, None
            if self._dead[d] or rc.cut(self.partition, clock, e, d):
                self._count(clock, "send_unreachable")
                error = True
            else:
                differ = self._rcs[e] != self._rcs[d]
                if differ:
                    self._count(clock, "checksums_differ")
                error = differ and self.enforce
            if not error:
                if q["retries"]:
                    self._count(clock, "retry_succeeded")
                if self.cpu.ring_lookup(d, h) != d:
                    self._count(clock, "misrouted")
                return final(DELIVERED, d)
            if q["retries"] >= self.max_retries:
                if self.max_retries:
                    self._count(clock, "retry_failed")
                return final(FAILED, d)
            self._count(clock, "retry_scheduled")
            q["due"] = clock + self.schedule[min(q["retries"], len(self.schedule) - 1)]
            if q["due"] > clock:
                return False

    def submit(self, clock, entries, keys):
        self._state(clock)
        for e, h in zip(entries, keys):
            e, h = int(e), int(h)
            q = {"id": len(self.results), "entry": e, "key_hash": h, "first_dest": -1, "due": 0, "submit_clock": clock,
                 "retries": 0}
            self.results.append(None)
            self._count(clock, "submitted")
            if self._dead[e]:
                self._count(clock, "entry_dead")
                self.by_retries["entry_dead"][0] += 1
                self.results[q["id"]] = (-1, ENTRY_DEAD, 0, clock, clock)
                continue
            d0 = self._lookup(e, h)
            if d0 == e:
                self._count(clock, "local")
                self.by_retries["local"][0] += 1
                self.results[q["id"]] = (e, LOCAL, 0, clock, clock)
                continue
            q["first_dest"] = d0
            self._count(clock, "proxied")
            if not self._advance(q, clock, d0):
                self.pending.append(q)

    def poll(self, clock):
        self._state(clock)
        self.history.setdefault(clock, dict.fromkeys(STATS, 0))
        self.pending = [q for q in self.pending if q["due"] > clock or not self._advance(q, clock, None)]

    def row(self, clock):
        return self.history.get(clock, dict.fromkeys(STATS, 0))


def stream(n, first, count):
    """Requests first .. first + count - 1 of the seed-11 stream: two lists."""
    e, h = rc.requests(REQ_SEED, first + count, n)
    return e[first:].tolist(), h[first:].tolist()


def run_model(name, per_step=None, **cfg):
    """The scenario on the oracle (seed 7, churn on): after every round a poll,
    then the next PER_ROUND requests of the stream; then DRAIN rounds with
    polls only.  per_step(model, clock) is called after each step's calls.
    Returns the model."""
    n, kw, rounds = SCENARIOS[name]
    cpu = oracle.Sim(n, SIM_SEED, **kw)
    m = Model(cpu, kw.get("partition"), **cfg)
    for r in range(1, rounds + DRAIN + 1):
        cpu.round(churn=True)
        m.poll(r)
        if r <= rounds:
            m.submit(r, *stream(n, (r - 1) * PER_ROUND, PER_ROUND))
        if per_step:
            per_step(m, r)
    cpu.close()
    m.cpu = None
    return m


def snapshot(m, clock):
    """What a GPU run is compared with after the calls at `clock` (copies)."""
    return {"stats": dict(m.stats), "row": dict(m.row(clock)), "by_retries": {k: list(v) for k, v in m.by_retries.items()},
            "pending": [(q["id"], q["entry"], q["key_hash"], q["first_dest"], q["due"], q["submit_clock"], q["retries"])
                        for q in m.pending],
            "results": list(m.results)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The default-configuration run of a scenario: (the final model, the
    snapshot after every step).  Computed once and shared; read-only."""
    snaps = []
    m = run_model(name, per_step=lambda mm, r: snaps.append(snapshot(mm, r)))
    return m, snaps
