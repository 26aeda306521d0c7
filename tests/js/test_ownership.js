// SimCluster.ownership() and SimCluster.ownershipAt() on the 64-node partition
// scenario after round 30, against the Python binding's result on the same
// scenario (tests/test_js_ownership.py passes it as a JSON file).
'use strict';
var assert = require('assert');
var fs = require('fs');
var path = require('path');
var ROOT = path.join(__dirname, '..', '..');
var rp = require(path.join(ROOT, 'js', 'index.js'));

var w = JSON.parse(fs.readFileSync(process.argv[2]));
var sim = new rp.SimCluster({ n: w.n, seed: w.seed, churnK: w.churnK });
sim.partition(w.partition.start, w.partition.end, w.partition.split);
for (var r = 0; r < w.rounds; r++) sim.round(true);

var got = sim.ownership();
assert.deepStrictEqual(Object.keys(got).sort(),
    ['claimants', 'claimed', 'intervals', 'maxClaims', 'maxClaimsHash', 'measure']);
assert.deepStrictEqual(got.measure, w.measure);
assert.strictEqual(got.measure.reduce(function (a, b) { return a + b; }, 0), 4294967296);
assert.strictEqual(got.claimants, w.claimants);
assert.strictEqual(got.intervals, w.intervals);
assert.strictEqual(got.maxClaims, w.maxClaims);
assert.strictEqual(got.maxClaimsHash, w.maxClaimsHash);
assert.ok(got.claimed instanceof BigUint64Array && got.claimed.length === w.n);
assert.deepStrictEqual(Array.from(got.claimed, String), w.claimed);

var at = sim.ownershipAt(Uint32Array.from(w.keyHashes));
assert.ok(at instanceof Uint32Array);
assert.deepStrictEqual(Array.from(at), w.claims);
assert.deepStrictEqual(sim.ownership().measure, w.measure);  // (the cached census)
assert.strictEqual(sim.ownershipAt(new Uint32Array(0)).length, 0);
assert.throws(function () { sim.ownershipAt([1, 2]); }, TypeError);
console.log('js ownership ok');
