// SimCluster.traffic() on the 64-node partition scenario for 30 rounds: after
// every round a poll, then the next requests of the stream; against the
// statistics, by_retries, history rows and pending table the Python side
// restated from the CPU oracle (tests/test_js_traffic.py passes them as JSON).
'use strict';
var assert = require('assert');
var fs = require('fs');
var path = require('path');
var ROOT = path.join(__dirname, '..', '..');
var rp = require(path.join(ROOT, 'js', 'index.js'));

var w = JSON.parse(fs.readFileSync(process.argv[2]));
var sim = new rp.SimCluster({ n: w.n, seed: w.seed, churnK: w.churnK });
sim.partition(w.partition.start, w.partition.end, w.partition.split);
var t = sim.traffic({ track: true });
assert.ok(t instanceof rp.SimCluster.Traffic);
assert.deepStrictEqual(rp.SimCluster.Traffic.OUTCOMES, w.outcomeNames);

for (var r = 1; r <= w.rounds; r++) {
    sim.round(true);
    t.poll();
    var lo = (r - 1) * w.perRound, hi = r * w.perRound;
    var first = t.submit(Uint32Array.from(w.entries.slice(lo, hi)), Uint32Array.from(w.keyHashes.slice(lo, hi)));
    assert.strictEqual(first, lo);
    assert.strictEqual(t.pending().count, w.pendingCounts[r - 1], 'pending after round ' + r);
}
var got = t.stats();
assert.deepStrictEqual(got.stats, w.stats);
assert.deepStrictEqual(got.byRetries, w.byRetries);
assert.deepStrictEqual(t.history(1, w.rounds), w.history);
var p = t.pending();
assert.ok(p.ids instanceof Float64Array && p.firstDests instanceof Int32Array && p.due instanceof Uint32Array);
assert.strictEqual(p.count, w.pending.length);
for (var i = 0; i < p.count; i++) {
    assert.deepStrictEqual([p.ids[i], p.entries[i], p.keyHashes[i], p.firstDests[i], p.due[i], p.submitClocks[i],
                            p.retries[i]], w.pending[i], 'pending record ' + i);
}
var res = t.results(0, w.rounds * w.perRound);
assert.ok(res.outcomes instanceof Uint8Array && res.dests instanceof Int32Array);
assert.deepStrictEqual(Array.from(res.outcomes), w.outcomes);
assert.strictEqual(rp.SimCluster.Traffic.PENDING, 255);

// the device generator and run(): a second tracker on the same cluster
var u = sim.traffic({ maxRetries: 1, schedule: [2], enforceConsistency: false, capacity: 4096 });
u.submitUniform(w.reqSeed, 0, 100);
assert.strictEqual(u.stats().stats.submitted, 100);
u.run(2, 50, w.reqSeed);
assert.strictEqual(u.stats().stats.submitted, 200);
assert.throws(function () { u.submit([1, 2], [3, 4]); }, TypeError);
assert.throws(function () { u.submit(new Uint32Array(2), new Uint32Array(3)); }, RangeError);
assert.throws(function () { sim.traffic({ schedule: [] }); }, RangeError);
assert.throws(function () { u.submitUniform(1, 0, 5000); }, /capacity/);
u.close();
assert.throws(function () { u.poll(); }, /closed/);
t.close();
console.log('js traffic ok');
