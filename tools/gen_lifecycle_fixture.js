// TEST INFRASTRUCTURE ONLY.  Writes tests/golden/sim_lifecycle.json.gz: the
// graceful leave / rejoin cases of DESIGN.md §12, recorded from the
// UNMODIFIED reference modules under tools/lifecycle_harness.js.
//
//   NODE_PATH=oracle/harness/shims node tools/gen_lifecycle_fixture.js tests/golden
//
// Every case asserts the properties it is there for and the script fails
// when one does not hold (tests/test_lifecycle_fixture.py checks them again
// on the committed file).
'use strict';

var fs = require('fs');
var path = require('path');
var zlib = require('zlib');
var HARNESS = process.env.RINGPOP_HARNESS || path.join(__dirname, '..', 'oracle', 'harness');
var common = require(path.join(HARNESS, 'common.js'));
var farmhash = require('farmhash');
var life = require('./lifecycle_harness.js');

var outDir = process.argv[2] || 'tests/golden';
var MAX_BYTES = 367747;  // the largest fixture there before this one (ring_farmhash.json)

function check(ok, what) { if (!ok) throw new Error('fixture property does not hold: ' + what); }

function fixture(name, cfg) {
    var t = Date.now();
    var r = life.runLifecycle(cfg);
    var out = { name: name, config: cfg, convergedAt: r.convergedAt, log: r.log, dumps: r.dumps, final: r.final,
                rounds: r.rounds.map(function (x) {
        return { round: x.round, churned: x.churned, evaluated: x.evaluated, applied: x.applied,
                 fullSyncs: x.fullSyncs, messages: x.messages, waves: x.waves, converged: x.converged,
                 checksums: x.checksums };
    }) };
    console.log(name, 'converged at', r.convergedAt, 'in', Date.now() - t, 'ms;', r.log.leaves.length, 'leaves',
                r.log.rejoins.length, 'rejoins', r.log.refusedStarts.length, 'refused starts', r.log.pingsToLeft,
                'pings and', r.log.pingReqsToLeft, 'ping-reqs to left nodes', r.log.fullSyncsToRejoined,
                'fullSyncs to rejoined nodes');
    return out;
}

function convergedRounds(c) { return c.rounds.filter(function (x) { return x.converged; }).map(function (x) { return x.round; }); }

// addresses of mixed shapes, 4-32 bytes, in sort order
function addresses(n, seed) {
    var r = common.nodeRng(seed, 0), set = {}, out = [];
    function d(k) { return Math.floor(r.random() * k); }
    while (out.length < n) {
        var k = d(4), a;
        if (k === 0) a = d(10) + '.' + d(10) + '.' + d(10) + '.' + d(10) + ':' + (1 + d(9));
        else if (k === 1) a = '192.168.' + d(256) + '.' + d(256) + ':' + (20000 + d(1000));
        else if (k === 2) a = 'host-' + d(100000) + '.dc' + d(9) + '.example:' + (8000 + d(100));
        else a = '172.' + (16 + d(16)) + '.' + d(256) + '.' + d(256) + ':' + (30000 + d(5000));
        if (a.length > 32 || set[a]) continue;
        set[a] = 1;
        out.push(a);
    }
    return out.sort(function (x, y) { return x < y ? -1 : x > y ? 1 : 0; });
}

var cases = [];

// 1. fail-stops, a storm, leaves and rejoins at 64 nodes
var c1 = fixture('storm', { n: 64, seed: 11, maxRounds: 90, churnRounds: 20, churnK: 2, failures: { 2: [3, 40] },
                            storm: { start: 5, end: 25, ppm: 40000 }, leaves: { 8: [5, 9, 17, 33], 12: [20] },
                            rejoins: { 45: [5, 17], 50: [20] }, dumpRounds: [8, 30, 46, 70] });
check(c1.log.leaves.some(function (e) { return e[2] > 0; }), 'a leaver with a pending timer');
check(c1.log.refusedStarts.length > 0, 'a refused suspicion start');
check(c1.log.pingsToLeft > 0 && c1.log.pingReqsToLeft > 0, 'a ping and a ping-req to a left node');
check(c1.log.fullSyncsToRejoined > 0, 'a fullSync to a rejoined node');
check(convergedRounds(c1).some(function (r) { return r < 45; }) && convergedRounds(c1).some(function (r) { return r > 50; }),
      'converged before and after the rejoins');
(function () {  // the routing test restates lookups from the ring ids: no two replica hashes may collide
    var seen = {};
    common.simAddresses(64).forEach(function (a) {
        for (var i = 0; i < 100; i++) {
            var h = farmhash.hash32(a + i);
            check(!seen[h], 'distinct replica hashes at 64 nodes');
            seen[h] = 1;
        }
    });
})();
cases.push(c1);

// 2. a partition, a leave during it, a rejoin long after it healed
var c2 = fixture('partition', { n: 32, seed: 12, maxRounds: 120, churnRounds: 0, churnK: 0,
                                partition: { start: 2, end: 40, split: 16 }, leaves: { 3: [20] }, rejoins: { 90: [20] },
                                dumpRounds: [3, 45, 91] });
check(c2.log.leaves.length === 1 && c2.log.rejoins.length === 1, 'the leave and the rejoin happened');
cases.push(c2);

// 3. 10 nodes: the server count crosses 10 -> 9 -> 10, maxPiggybackCount 30 -> 15 -> 30
var c3 = fixture('piggyback', { n: 10, seed: 13, maxRounds: 50, churnRounds: 0, churnK: 0, leaves: { 2: [4] },
                                rejoins: { 25: [4] }, dumpRounds: [1, 20, 45] });
// (before the first ring change a node still has the count set when it alone
// was in its ring: adjustMaxPiggybackCount runs on 'ringChanged' only)
[[1, 10, null], [20, 9, 15], [45, 10, 30]].forEach(function (e) {
    c3.dumps[e[0]].forEach(function (d, v) {
        check(d.ringServers === e[1] && (e[2] === null || d.maxPiggyback === e[2]),
              'round ' + e[0] + ' node ' + v + ': ' + e[1] + ' servers, maxPiggybackCount ' + e[2]);
    });
});
cases.push(c3);

// 4. 96 nodes on explicit addresses, leaves in three consecutive rounds --
// the first and the last node of a 4-shard block among them -- all rejoining, churn throughout
var c4 = fixture('sharded', { n: 96, seed: 14, maxRounds: 70, churnRounds: 70, churnK: 2, addresses: addresses(96, 91),
                              leaves: { 5: [24, 60], 6: [47, 0], 7: [95, 30] },
                              rejoins: { 30: [24, 47], 31: [0, 95], 40: [60, 30] }, dumpRounds: [7, 32], noFinal: false });
check(c4.log.leaves.length === 6 && c4.log.rejoins.length === 6, 'six leaves and six rejoins');
cases.push(c4);

// 5. leave after join: joiner 9 (joined at round 2) leaves at round 6; seed 1
// serves the join of round 4 and leaves at round 6 too; both rejoin
var c5 = fixture('join', { n: 24, seed: 15, maxRounds: 80, churnRounds: 10, churnK: 1,
                           joins: [[0, 8, [0, 1]], [2, 9, [1, 2, 3]], [2, 10, [0]], [4, 11, [1, 9]], [4, 12, [8, 2]],
                                   [6, 13, [3]], [8, 14, [10, 11, 12]], [8, 15, [0, 13]], [10, 16, [2]], [10, 17, [14]],
                                   [12, 18, [15, 16]], [12, 19, [0]], [14, 20, [17]], [14, 21, [18, 3]], [16, 22, [19]],
                                   [16, 23, [20, 21]]],
                           leaves: { 6: [9, 1] }, rejoins: { 40: [9], 44: [1] }, dumpRounds: [6, 41] });
check(c5.log.leaves.length === 2 && c5.log.rejoins.length === 2, 'the joiner and the seed left and rejoined');
cases.push(c5);

var p = path.join(outDir, 'sim_lifecycle.json.gz');
var buf = zlib.gzipSync(Buffer.from(JSON.stringify({ cases: cases })), { level: 9 });
check(buf.length <= MAX_BYTES, 'fixture of ' + buf.length + ' bytes within ' + MAX_BYTES);
fs.writeFileSync(p, buf);
console.log('wrote', p, buf.length, 'bytes');
