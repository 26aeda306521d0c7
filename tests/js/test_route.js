// SimCluster.ringChecksums() and SimCluster.route() on the 64-node partition
// scenario after round 30, against the expectation the Python side restated
// from the CPU oracle (tests/test_js_route.py passes it as a JSON file).
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

var cs = sim.ringChecksums();
assert.ok(cs instanceof Uint32Array);
assert.deepStrictEqual(Array.from(cs), w.ringChecksums);
assert.strictEqual(sim.node(5).ring.checksum, w.ringChecksums[5]);

var got = sim.route(Uint32Array.from(w.entries), Uint32Array.from(w.keyHashes));
assert.ok(got.dests instanceof Int32Array && got.outcomes instanceof Uint8Array && got.ownerAgrees instanceof Uint8Array);
assert.deepStrictEqual(Array.from(got.dests), w.dests);
assert.deepStrictEqual(Array.from(got.outcomes), w.outcomes);
assert.deepStrictEqual(Array.from(got.ownerAgrees), w.ownerAgrees);
assert.deepStrictEqual(got.stats, w.stats);
assert.strictEqual(rp.SimCluster.ROUTE_OUTCOMES[got.outcomes[0]], w.outcomeNames[w.outcomes[0]]);
assert.throws(function () { sim.route([1, 2], [3, 4]); }, TypeError);
assert.throws(function () { sim.route(new Uint32Array(2), new Uint32Array(3)); }, RangeError);
console.log('js route ok');
