// Graceful leave and rejoin through SimCluster (leave, rejoin, flags) on the
// 10-node case of tests/golden/sim_lifecycle.json.gz, recorded from the
// reference's admin handlers: every round's counts and checksums, and at the
// dump rounds each node's ring server count (10 -> 9 -> 10),
// maxPiggybackCount (-> 15 -> 30), view and flags.
'use strict';
var assert = require('assert');
var path = require('path');
var zlib = require('zlib');
var fs = require('fs');
var ROOT = path.join(__dirname, '..', '..');
var rp = require(path.join(ROOT, 'js', 'index.js'));

var g = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'sim_lifecycle.json.gz'))));
var c = g.cases[2], cfg = c.config;
assert.strictEqual(c.name, 'piggyback');
var STATUS = [null, 'alive', 'suspect', 'faulty', 'leave'];
var sim = new rp.SimCluster({ n: cfg.n, seed: cfg.seed, churnK: cfg.churnK });
assert.throws(function () { sim.rejoin(4, 25); });  // a rejoin comes after a leave
Object.keys(cfg.leaves).forEach(function (r) { cfg.leaves[r].forEach(function (v) { sim.leave(v, Number(r)); }); });
Object.keys(cfg.rejoins).forEach(function (r) { cfg.rejoins[r].forEach(function (v) { sim.rejoin(v, Number(r)); }); });
assert.throws(function () { sim.rejoin(4, 30); });  // two rejoins in a row
var dumps = 0;
c.rounds.forEach(function (jr, r) {
    var st = sim.round(r < cfg.churnRounds);
    assert.strictEqual(st.evaluated, jr.evaluated, 'round ' + r);
    assert.strictEqual(st.applied, jr.applied, 'round ' + r);
    assert.strictEqual(st.converged, jr.converged, 'round ' + r);
    assert.deepStrictEqual(Array.from(sim.checksums()), jr.checksums, 'round ' + r);
    var d = c.dumps[r];
    if (!d) return;
    dumps++;
    d.forEach(function (f, v) {
        var node = sim.node(v), fl = sim.flags(v);
        assert.strictEqual(node.ring.getServerCount(), f.ringServers, 'round ' + r + ' node ' + v);
        assert.strictEqual(node.ring.checksum, f.ringChecksum);
        assert.strictEqual(node.dissemination.maxPiggybackCount, f.maxPiggyback, 'round ' + r + ' node ' + v);
        assert.strictEqual(fl.gossipStopped, !f.gossiping);
        assert.strictEqual(fl.suspicionStopped, f.suspicionStopped);
        f.view.forEach(function (e, a) {
            var m = node.membership.findMemberByAddress(sim.addresses()[a]);
            assert.strictEqual(m.status, STATUS[e[0]]);
            assert.strictEqual(m.incarnationNumber, e[1]);
        });
        assert.deepStrictEqual(Object.keys(node.dissemination.changes),
                               f.changes.map(function (row) { return sim.addresses()[row[0]]; }));
    });
});
assert.strictEqual(dumps, 3);
assert.strictEqual(c.dumps[20][0].ringServers, 9);
assert.strictEqual(c.dumps[20][0].maxPiggyback, 15);
assert.strictEqual(c.dumps[45][0].maxPiggyback, 30);
assert.deepStrictEqual(sim.flags(4), { gossipStopped: false, suspicionStopped: false });
console.log('js lifecycle ok');
