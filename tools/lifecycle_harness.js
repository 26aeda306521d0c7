// TEST INFRASTRUCTURE ONLY (runs under Node beside the reference; never on a
// GPU).  The round driver of oracle/harness/sim.js restated with graceful
// leaves and rejoins (DESIGN.md §12): it `require`s the UNMODIFIED reference
// modules at run time and calls the reference's own admin handlers
// (server/admin-leave-handler.js, server/admin-join-handler.js) for the
// events.  oracle/harness/common.js and the shims are reused as they are:
//
//   NODE_PATH=oracle/harness/shims node tools/lifecycle_harness.js '<config json>'
//
//   round r, virtual now = T0 + 200 r:
//     1. fail-stops   2. due suspicion timers   3. joins
//     4. leaves and rejoins scheduled for r     5. churn   6. storm
//     7. every live, gossiping node pings; message waves
//
// cfg.leaves / cfg.rejoins: {round: [ids]}.  An event for a node that has
// fail-stopped or not yet joined is skipped.  rp.gossip is a stub: start() is
// membership.shuffle() (lib/swim/gossip.js:85) plus the flag, stop() the flag
// only -- Gossip.run would draw Math.random and arm the wall-clock timers
// that this driver replaces.  Without events the output equals sim.js's
// (tests/test_lifecycle_harness.py compares them field by field).
'use strict';

var path = require('path');
var REF = process.env.RINGPOP_REFERENCE || '/root/reference';
var HARNESS = process.env.RINGPOP_HARNESS || path.join(__dirname, '..', 'oracle', 'harness');
var common = require(path.join(HARNESS, 'common.js'));

var STATUS_CODE = { alive: 1, suspect: 2, faulty: 3, leave: 4 };

function runLifecycle(cfg) {
    var RingPop = require(path.join(REF, 'index.js'));
    var createServer = require(path.join(REF, 'server/index.js'));
    var handleJoin = require(path.join(REF, 'server/join-handler.js'));
    var handleAdminLeave = require(path.join(REF, 'server/admin-leave-handler.js'));
    var handleAdminJoin = require(path.join(REF, 'server/admin-join-handler.js'));
    var mergeJoinResponses = require(path.join(REF, 'lib/swim/join-response-merge.js'));
    var uuid = require('node-uuid');
    uuid._reset();

    var n = cfg.n;
    var addr = cfg.addresses || common.simAddresses(n);
    var STATUS_NAME = [null, 'alive', 'suspect', 'faulty', 'leave'];
    var idOf = {};
    addr.forEach(function (a, i) { idOf[a] = i; });
    var seed = cfg.seed;
    var rngs = [];
    for (var i = 0; i < n; i++) rngs.push(common.nodeRng(seed, i));
    var crng = common.churnRng(seed);
    var srng = common.stormRng(seed);
    var ctx = { node: -1, now: 0 };
    var timers = new common.TimerQueue();

    var saved = { now: Date.now, random: Math.random, st: global.setTimeout, ct: global.clearTimeout };
    Date.now = function () { return ctx.now; };
    Math.random = function () {
        if (ctx.node < 0) throw new Error('Math.random outside a node context');
        return rngs[ctx.node].random();
    };
    global.setTimeout = function (fn, ms) { return timers.add(ctx.now + ms, ctx.node, fn); };
    global.clearTimeout = function (t) { if (t && typeof t === 'object' && 'cancelled' in t) t.cancelled = true; };

    var dead = new Array(n).fill(false);
    var joinsAt = {}, joined = new Array(n).fill(true);
    (cfg.joins || []).forEach(function (e) {
        (joinsAt[e[0]] = joinsAt[e[0]] || []).push(e);
        joined[e[1]] = false;
    });
    var gossiping = new Array(n).fill(true);
    var next = [];
    var handlers = [];
    var stats = { evaluated: 0, applied: 0, fullSyncs: 0, messages: 0 };
    // what the events did and met (the fixture's assertions)
    var log = { leaves: [], rejoins: [], refusedStarts: [], pingsToLeft: 0, pingReqsToLeft: 0, fullSyncsToRejoined: 0 };
    var everRejoined = new Array(n).fill(false);
    var curRound = 0;

    function enqueue(m) { next.push(m); stats.messages++; }

    var rps = [];
    try {
        for (i = 0; i < n; i++) {
            (function (me) {
                handlers.push({});
                var channel = {
                    waitForIdentified: function (opts, cb) { cb(); },
                    request: function (opts) {
                        return {
                            send: function (endpoint, head, body, cb) {
                                enqueue({ type: 'req', from: me, to: idOf[opts.host], endpoint: endpoint,
                                          head: head, body: body, cb: cb });
                            }
                        };
                    }
                };
                var tchannel = { register: function (url, h) { handlers[me][url] = h; } };
                ctx.node = me;
                ctx.now = common.INC0 + me;
                var rp = new RingPop({ app: 'sim', hostPort: addr[me], channel: channel });
                rp.membershipUpdateRollup = { trackUpdates: function () {}, destroy: function () {} };
                createServer(rp, tchannel);
                rp.gossip = {
                    start: function () { rp.membership.shuffle(); gossiping[me] = true; },
                    stop: function () { gossiping[me] = false; }
                };

                if (joined[me]) {
                    var row = cfg.views ? cfg.views[me] : null;
                    rp.membership.makeAlive(addr[me], row ? row[me][1] : common.INC0 + me);
                    var stash = [];
                    for (var j = 0; j < n; j++) {
                        if (row ? row[j][0] === 0 : !joined[j]) continue;
                        stash.push(row ? { address: addr[j], status: STATUS_NAME[row[j][0]], incarnationNumber: row[j][1] }
                                       : { address: addr[j], status: 'alive', incarnationNumber: common.INC0 + j });
                    }
                    rp.membership.stashedUpdates = [stash];
                    rp.membership.set();
                    rp.membership.shuffle();
                    rp.isReady = true;
                    rp.dissemination.clearChanges();
                }

                var upd = rp.membership.update;
                rp.membership.update = function (changes, isLocal) {
                    var c = Array.isArray(changes) ? changes.length : 1;
                    var res = upd.apply(this, arguments);
                    stats.evaluated += c;
                    stats.applied += res.length;
                    return res;
                };
                var fs = rp.dissemination.fullSync;
                rp.dissemination.fullSync = function () { stats.fullSyncs++; return fs.apply(this, arguments); };
                // a suspect period refused while suspicion is stopped (lib/swim/suspicion.js:46-51)
                var sstart = rp.suspicion.start;
                rp.suspicion.start = function (member) {
                    if (this.isStoppedAll === true) log.refusedStarts.push([curRound, me, idOf[member.address]]);
                    return sstart.apply(this, arguments);
                };
                rps.push(rp);
            })(i);
        }

        var part = cfg.partition || null;
        function cut(a, b) {
            return !!part && curRound >= part.start && curRound < part.end &&
                ((a < part.split) !== (b < part.split));
        }

        function deliver(m) {
            if (m.type === 'req') {
                if (dead[m.to] || cut(m.from, m.to)) {
                    enqueue({ type: 'resp', to: m.from, cb: m.cb, err: new Error('request timed out') });
                    return;
                }
                if (!gossiping[m.to]) {
                    if (m.endpoint === '/protocol/ping') log.pingsToLeft++;
                    if (m.endpoint === '/protocol/ping-req') log.pingReqsToLeft++;
                }
                ctx.node = m.to;
                var before = stats.fullSyncs;
                var res = {
                    headers: {},
                    sendOk: function (r1, r2) { enqueue({ type: 'resp', to: m.from, cb: m.cb, err: null, ok: true, r1: r1, r2: r2 }); },
                    sendNotOk: function (r1, r2) { enqueue({ type: 'resp', to: m.from, cb: m.cb, err: null, ok: false, r1: r1, r2: r2 }); }
                };
                handlers[m.to][m.endpoint]({ remoteAddr: addr[m.from] }, res, m.head, m.body);
                if (stats.fullSyncs > before && everRejoined[m.from] && gossiping[m.from]) log.fullSyncsToRejoined++;
            } else {
                ctx.node = m.to;
                if (m.err) m.cb(m.err);
                else m.cb(null, { ok: m.ok }, m.r1, m.r2);
            }
        }

        var rounds = [];
        var convergedAt = -1;
        var failAt = cfg.failures || {};
        var leaveAt = cfg.leaves || {}, rejoinAt = cfg.rejoins || {};
        var churnK = cfg.churnK === undefined ? Math.ceil(0.01 * n) : cfg.churnK;
        var dumpRounds = cfg.dumpRounds || [];
        var dumps = {};
        for (var r = 0; r < cfg.maxRounds; r++) {
            ctx.now = common.T0 + common.PERIOD * r;
            curRound = r;
            stats.evaluated = 0; stats.applied = 0; stats.fullSyncs = 0; stats.messages = 0;
            (failAt[r] || []).forEach(function (v) { dead[v] = true; });

            var due = timers.due(ctx.now);
            for (var t = 0; t < due.length; t++) {
                if (dead[due[t].node]) continue;
                ctx.node = due[t].node;
                due[t].fn();
            }

            (joinsAt[r] || []).forEach(function (e) {
                var jn = e[1], rpj = rps[jn];
                if (dead[jn]) return;
                ctx.node = jn;
                rpj.membership.makeAlive(addr[jn], ctx.now);
                var jinc = rpj.membership.localMember.incarnationNumber;
                var responses = e[2].map(function (sd) {
                    if (dead[sd] || !joined[sd]) throw new Error('join seed ' + sd + ' is not a live member');
                    ctx.node = sd;
                    var body = null;
                    handleJoin({ ringpop: rps[sd], source: addr[jn], incarnationNumber: jinc, app: 'sim' },
                               function (err, res) { if (err) throw err; body = res; });
                    return JSON.parse(JSON.stringify({ checksum: body.membershipChecksum, members: body.membership }));
                });
                ctx.node = jn;
                rpj.membership.update(mergeJoinResponses(rpj, responses));
                rpj.membership.set();
                rpj.membership.shuffle();
                rpj.isReady = true;
                joined[jn] = true;
            });

            // 4. leaves, then rejoins, of round r: each touches its own node
            // only.  The handlers answer through process.nextTick: outcomes
            // are read off the node's state around the call.
            (leaveAt[r] || []).forEach(function (v) {
                if (dead[v] || !joined[v]) return;
                var rp = rps[v];
                ctx.node = v;
                if (rp.membership.localMember.status === 'leave') throw new Error('leave: node ' + v + ' has already left');
                var pending = Object.keys(rp.suspicion.timers).length;
                handleAdminLeave({ ringpop: rp }, function () {});
                if (gossiping[v] || rp.suspicion.isStoppedAll !== true || rp.membership.localMember.status !== 'leave' ||
                    Object.keys(rp.suspicion.timers).length !== 0)
                    throw new Error('leave: node ' + v + ' did not leave');
                log.leaves.push([r, v, pending]);
            });
            (rejoinAt[r] || []).forEach(function (v) {
                if (dead[v] || !joined[v]) return;
                var rp = rps[v];
                ctx.node = v;
                // (else the reference runs its join-sender: not modelled)
                if (rp.membership.localMember.status !== 'leave')
                    throw new Error('rejoin: node ' + v + ' is ' + rp.membership.localMember.status + ', not leave');
                handleAdminJoin({ ringpop: rp }, function () {});
                if (!gossiping[v] || rp.suspicion.isStoppedAll === true || rp.membership.localMember.status !== 'alive')
                    throw new Error('rejoin: node ' + v + ' did not rejoin');
                everRejoined[v] = true;
                log.rejoins.push([r, v]);
            });

            var live = [];
            for (i = 0; i < n; i++) if (!dead[i] && joined[i] && gossiping[i]) live.push(i);
            var churned = [];
            if (r < cfg.churnRounds) {
                churned = common.chooseChurn(crng, live, churnK);
                churned.forEach(function (v) {
                    ctx.node = v;
                    rps[v].membership.makeAlive(addr[v], ctx.now);
                });
            }
            var storm = cfg.storm;
            if (storm && r >= storm.start && r < storm.end) {
                common.chooseStorm(srng, live, storm.ppm).forEach(function (p) {
                    ctx.node = p[0];
                    var mem = rps[p[0]].membership;
                    mem.makeSuspect(addr[p[1]], mem.findMemberByAddress(addr[p[1]]).incarnationNumber);
                });
            }

            for (i = 0; i < n; i++) {
                if (dead[i] || !joined[i] || !gossiping[i]) continue;
                ctx.node = i;
                rps[i].pingMemberNow();
            }
            var waves = 0;
            while (next.length) {
                var wave = next; next = [];
                for (var w = 0; w < wave.length; w++) deliver(wave[w]);
                waves++;
            }
            ctx.node = -1;

            var sums = rps.map(function (rp, v) { return dead[v] || !joined[v] ? null : rp.membership.checksum; });
            var liveSums = sums.filter(function (s, v) { return s !== null && gossiping[v]; });
            var converged = liveSums.every(function (s) { return s === liveSums[0]; });
            rounds.push({ round: r, churned: churned, checksums: sums, evaluated: stats.evaluated,
                          applied: stats.applied, fullSyncs: stats.fullSyncs, messages: stats.messages,
                          waves: waves, converged: converged });
            if (dumpRounds.indexOf(r) >= 0) dumps[r] = dumpAll();
            if (converged && r >= cfg.churnRounds && convergedAt < 0) {
                convergedAt = r;
                if (cfg.stopAtConvergence) break;
            }
        }
        return { config: cfg, addresses: addr, rounds: rounds, convergedAt: convergedAt, dumps: dumps,
                 final: cfg.noFinal ? undefined : dumpAll(), log: log };
    } finally {
        Date.now = saved.now; Math.random = saved.random;
        global.setTimeout = saved.st; global.clearTimeout = saved.ct;
    }

    function dumpNode(rp, v) {
        var m = rp.membership;
        var view = new Array(n).fill(null);
        m.members.forEach(function (mem) { view[idOf[mem.address]] = [STATUS_CODE[mem.status], mem.incarnationNumber]; });
        var d = rp.dissemination;
        var keys = Object.keys(d.changes).map(function (a) {
            var c = d.changes[a];
            return [idOf[a], c.piggybackCount === undefined ? -1 : c.piggybackCount,
                    c.source === undefined ? -1 : idOf[c.source],
                    c.sourceIncarnationNumber === undefined ? 0 : c.sourceIncarnationNumber,
                    STATUS_CODE[c.status], c.incarnationNumber];
        });
        var suspects = Object.keys(rp.suspicion.timers).map(function (a) { return idOf[a]; });
        var out = {
            dead: dead[v], checksum: m.checksum, members: m.members.map(function (x) { return idOf[x.address]; }),
            view: view, changes: keys, maxPiggyback: d.maxPiggybackCount,
            ringServers: rp.ring.getServerCount(), ringChecksum: rp.ring.checksum,
            iterIndex: rp.memberIterator.currentIndex, iterRound: rp.memberIterator.currentRound,
            timers: suspects, rng: rngs[v].s.toString()
        };
        if (!cfg.plainDumps) {
            out.gossiping = gossiping[v];
            out.suspicionStopped = rp.suspicion.isStoppedAll === true;
            out.ringIds = Object.keys(rp.ring.servers).map(function (a) { return idOf[a]; }).sort(function (a, b) { return a - b; });
        }
        return out;
    }
    function dumpAll() { return rps.map(dumpNode); }
}

module.exports = { runLifecycle: runLifecycle, STATUS_CODE: STATUS_CODE };

if (require.main === module) {
    process.stdout.write(JSON.stringify(runLifecycle(JSON.parse(process.argv[2]))));
}
