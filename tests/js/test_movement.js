// SimCluster.ownershipSnapshot() and SimCluster.ownershipMoved() on the 64-node
// partition scenario between clocks 39 and 42, against the Python binding's
// result on the same scenario (tests/test_js_movement.py passes it as a JSON
// file).
'use strict';
var assert = require('assert');
var fs = require('fs');
var path = require('path');
var ROOT = path.join(__dirname, '..', '..');
var rp = require(path.join(ROOT, 'js', 'index.js'));

var w = JSON.parse(fs.readFileSync(process.argv[2]));
var sim = new rp.SimCluster({ n: w.n, seed: w.seed, churnK: w.churnK });
sim.partition(w.partition.start, w.partition.end, w.partition.split);
for (var r = 0; r < w.from; r++) sim.round(true);
var from = sim.ownershipSnapshot();
assert.strictEqual(from.clock, w.from);
assert.deepStrictEqual(from.stats.measure, sim.ownership().measure);
for (r = w.from; r < w.to; r++) sim.round(true);

function check(got) {
    Object.keys(w.stats).forEach(function (k) { assert.deepStrictEqual(got[k], w.stats[k], k); });
    assert.deepStrictEqual(Object.keys(got).sort(), Object.keys(w.stats).concat(['gainedBy', 'lostBy']).sort());
    assert.strictEqual(got.transition.reduce(function (a, row) {
        return a + row.reduce(function (x, y) { return x + y; }, 0);
    }, 0), 4294967296);
    assert.ok(got.gainedBy instanceof BigUint64Array && got.gainedBy.length === w.n);
    assert.ok(got.lostBy instanceof BigUint64Array && got.lostBy.length === w.n);
    assert.deepStrictEqual(Array.from(got.gainedBy, String), w.gainedBy);
    assert.deepStrictEqual(Array.from(got.lostBy, String), w.lostBy);
}
check(sim.ownershipMoved(from));  // (to: the cluster as it is now)
var to = sim.ownershipSnapshot();
assert.strictEqual(to.clock, w.to);
check(sim.ownershipMoved(from, to));
var same = sim.ownershipMoved(to, to);
assert.strictEqual(same.sameSet, 4294967296);
assert.strictEqual(same.gained + same.lost + same.maxTurnover, 0);
assert.throws(function () { sim.ownershipMoved({}, to); }, TypeError);
to.close();
assert.throws(function () { sim.ownershipMoved(from, to); }, /closed/);
from.close();
from.close();
console.log('js movement ok');
