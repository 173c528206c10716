"""Directed tests of the delta store (ks_store.hip), arc by arc.

Small hand-made scheduling networks — tasks with supply 1, aggregators, PUs, one
sink, and for every task an expensive bypass arc into an unscheduled aggregator, so
every case is feasible by construction — are edited by streams sized by the store's
constants: its 64-lane waves, its 256-thread workgroups (SBLK), the 64-position
scan chunk of claim_pos (SCAN) and the segment capacities of the CSR build.

After every stream: the store read back (ks_get_graph) equals the reference state
exactly (store_ref.same_store), the counters of ks_get_store_stats equal the ones
the reference derives from the records, the next solve equals the oracle's
successive shortest path on the restated graph with no certificate repair, and the
oracle's verifier accepts the downloaded flows at that cost.

The removal cases run with the stream applied before any solve (no CSR yet: the
store scans every arc slot, k_kill_scan), after a solve on each solver path (the
removed nodes' own segments, k_kill_nodes, on the tight CSR of a load), and on a
warm-starting engine context, tight and with slack: only a warm re-solve keeps the
flow and the excess the store's kernels hand back, a cold one resets them.

Mutations of ks_store.hip these tests were run against (scratch builds, GPU):
  - kill_node_segment without the tail rule (d.n_lastrm[sl] < 0): case A fails in its
    four post-solve modes (the arc u → v is freed and counted twice);
  - killed also counted in k_kill_nodes for an arc a later record re-creates: both
    halves of case C fail in their post-solve modes;
  - claim_pos returning b + ps without its CAS: the two-chunk case fails on the engine
    (KS_E_VERIFY: a scanned chunk hands out a position a lane of the tail holds);
  - steps = len without the wave-wide max: nothing can fail, here or in the random
    streams — lanes that leave the loop early drop out of the later ballots and every
    result is the same on gfx950; the max is defensive;
  - k_reset_used skipped: nothing can fail — the inserts then find the same inert
    positions through the chunk scan; the kernel buys speed only."""
import pytest

from graphs import graph_from_lists
from ksched_amd import native
from oracle import ko
from store_ref import StoreRef, check_counters, delta, same_store, stream
from test_gpu_parity import flows_by_arc

pytestmark = pytest.mark.gpu

WAVE, SBLK, SCAN = 64, 256, 64          # ks_store.hip: a wave, a workgroup, claim_pos's scan chunk
OTHER, TASK, PU, SINK, MID = 0, 1, 2, 3, 5
ADD_NODE, REMOVE_NODE, ADD_ARC, UPDATE_ARC = 0, 1, 2, 3
BYPASS = 1000


def seg_capacity(deg: int, alive: bool = True, task: bool = False) -> int:
    """A node's segment capacity once the graph is edited incrementally: the rule of
    ks_engine_build.hip (seg_capacity, with slack) restated — tasks and dead slots of
    at most 8 arcs one 8-lane group; other nodes their degree + 50 % (at least + 4)
    rounded up to a power of two up to 64, else to whole 64-position chunks. (The
    build never gives less than the node had before, which after a load is its
    degree.)"""
    if (not alive or task) and deg <= 8:
        return 8
    c = deg + max(deg // 2, 4)
    if c <= 64:
        g = 4
        while g < c:
            g <<= 1
        return g
    return (c + 63) // 64 * 64


class Net:
    """Node and arc lists of a scheduling network: one sink, one unscheduled
    aggregator every task has a bypass arc into, and a spare task and PU that the
    priming stream joins (an insert into two full segments of the tight post-load
    CSR: the next solve rebuilds it with slack)."""

    def __init__(self):
        self.nodes, self.arcs = [], []
        self.sink = self.node(SINK)
        self.unsched = self.node(OTHER)
        self.arc(self.unsched, self.sink, 100_000, 0)
        self.spare_task, self.spare_pu = self.task(), self.pu(1)

    def node(self, ntype, supply=0):
        self.nodes.append((len(self.nodes) + 1, supply, ntype))
        return len(self.nodes)

    def arc(self, s, d, cap=1, cost=0, low=0):
        self.arcs.append((s, d, low, cap, cost))

    def task(self):
        t = self.node(TASK, 1)
        self.arc(t, self.unsched, 1, BYPASS)
        return t

    def pu(self, cap):
        p = self.node(PU)
        self.arc(p, self.sink, cap, 0)
        return p

    def graph(self):
        total = sum(e for _, e, _ in self.nodes)
        nodes = [(i, -total if i == self.sink else e, t) for i, e, t in self.nodes]
        return graph_from_lists(nodes, self.arcs)

    def degree(self, v):
        return sum(v in (s, d) for s, d, *_ in self.arcs)


def arc(kind, s, d, cap=1, cost=0, low=0, type=0):
    return delta(kind=kind, src=s, dst=d, low=low, cap=cap, cost=cost, type=type)


def erase(s, d):
    return arc(UPDATE_ARC, s, d, cap=0)


class Dev:
    """One network on one context, with its reference beside it."""

    def __init__(self, ctx, net, solve_first=True, warm=False):
        self.ctx, self.net, self.warm = ctx, net, warm
        g = net.graph()
        self.ref = StoreRef.from_graph(g)
        ctx.load_graph(g)
        self.csr_valid = False      # a CSR exists and matches the table (as the store sees it at the next apply)
        same_store(ctx, self.ref)
        if solve_first:
            self.solve()

    def solve(self):
        h = self.ref.graph()
        st, cost, fv, _, _ = ko.ssp(h)
        assert st == 0, "the network is feasible by construction"
        r = self.ctx.solve()
        assert (r.cost, r.flow) == (cost, fv)
        assert r.raw["recoveries"] == 0
        if self.warm and self.csr_valid:
            assert r.raw["warm_started"] == 1
        vst, vcost, _ = ko.verify(h, flows_by_arc(self.ctx, h))
        assert vst == 0 and vcost == cost, "the oracle's verifier rejected the downloaded flows"
        self.csr_valid = True
        return r

    def apply(self, recs):
        """→ (the next solve's result, the store's counters, the expected counters)."""
        recs = stream(recs)
        met_csr = self.csr_valid
        self.ctx.apply_deltas(recs)
        want = self.ref.apply(recs)
        same_store(self.ctx, self.ref)
        stats = self.ctx.store_stats()   # (before the solve: its auto-sink edit is a stream of its own)
        r = self.solve()
        check_counters(stats, want, exact=met_csr and r.raw["rebuilt"] == 0)
        return r, stats, want

    def prime(self):
        r, _, want = self.apply([arc(ADD_ARC, self.net.spare_task, self.net.spare_pu, 1, 900)])
        assert r.raw["rebuilt"] == 1 and want["upserts_new"] == 1
        assert self.ctx.store_stats()["rebuilds"] >= 2


@pytest.fixture(scope="module")
def ctx_warm():
    c = native.Context(0, cell_nodes=-1, warm_start=1)
    yield c
    c.close()


@pytest.fixture(params=["scan", "cell", "engine", "warm", "warm-slack"])
def removal_dev(request, ctx, ctx_engine, ctx_warm):
    """net → Dev, in each way the removal cases run (the module docstring)."""
    mode = request.param
    c = {"scan": ctx_engine, "cell": ctx, "engine": ctx_engine, "warm": ctx_warm, "warm-slack": ctx_warm}[mode]

    def make(net):
        d = Dev(c, net, solve_first=mode != "scan", warm=mode.startswith("warm"))
        d.mode = mode
        if mode == "warm-slack":
            d.prime()
        return d
    return make


def removal_only(dev, r):
    """A stream that only removes fits any CSR: met by a valid one, it leaves it valid."""
    assert r.raw["rebuilt"] == (1 if dev.mode == "scan" else 0)


# ------------------------------------------------------------ A, C, D ---
def small_net():
    n = Net()
    n.T = [n.task() for _ in range(8)]
    n.W = n.node(OTHER)                 # the aggregator that survives every case
    n.P = [n.pu(2) for _ in range(6)]
    for t in n.T:
        n.arc(t, n.W, 1, 50)
    for p in n.P:
        n.arc(n.W, p, 1, 1)
    # A: the adjacent pair u ⇄ v, each with in- and out-arcs to survivors; u → v has low = 1.
    # u → v and v → u come first among the arcs of both: a segment holds a node's arcs in
    # arc-slot order, so the lanes of u and v meet each of the two at the same step
    n.u, n.v = n.node(OTHER), n.node(OTHER)
    n.arc(n.u, n.v, 2, 1, low=1)
    n.arc(n.v, n.u, 2, 5)
    for t in n.T[0:3]:
        n.arc(t, n.u, 1, 1)
    for t in n.T[3:5]:
        n.arc(t, n.v, 1, 1)
    n.arc(n.u, n.P[0], 1, 1)
    n.arc(n.v, n.P[1], 3, 1)
    # C: x, whose id is reused
    n.x = n.node(OTHER)
    for t in n.T[5:8]:
        n.arc(t, n.x, 1, 1)
    for p in n.P[3:6]:
        n.arc(n.x, p, 1, 1)
    # D: z has only in-arcs, y only out-arcs
    n.z, n.y = n.node(OTHER), n.node(OTHER)
    n.arc(n.T[0], n.z, 1, 0)
    n.arc(n.T[1], n.z, 1, 0)
    n.arc(n.y, n.P[0], 1, 1)
    n.arc(n.y, n.P[1], 1, 1)
    return n


def test_adjacent_pair_removed_in_one_stream(removal_dev):
    """A. u and v removed in one stream with u → v (low = 1) and v → u both present and
    units routed through them: an arc with both endpoints removed is handled once,
    from its tail's segment (killed counts it once, its slot is freed once), and its
    flow and lower bound go back to its endpoints' excess."""
    n = small_net()
    dev = removal_dev(n)
    if dev.csr_valid:   # the first solve routed units through u and v (the lower bound forces one)
        f = {(int(s), int(d)): int(x) for s, d, x in dev.ctx.flows().tolist()}
        assert f.get((n.u, n.v), 0) >= 1 and f.get((n.v, n.P[1]), 0) + f.get((n.u, n.P[0]), 0) >= 1
    r, stats, want = dev.apply([
        arc(UPDATE_ARC, n.W, n.P[2], 1, 2),             # a survivor's arc, in place
        arc(UPDATE_ARC, n.T[0], n.u, 1, 9, type=1),     # dead: its head goes below
        delta(kind=REMOVE_NODE, id=n.u),
        delta(kind=REMOVE_NODE, id=n.v),
    ])
    assert (want["killed"], want["superseded"], want["upserts_inplace"], want["upserts_new"]) == (9, 0, 1, 0)
    removal_only(dev, r)
    # the freed slots are handed out again, each once: nine new arcs take them
    r, stats, want = dev.apply([arc(ADD_ARC, t, p, 1, 3, type=1) for t, p in zip(n.T + n.T[:1], n.P + n.P[:3])])
    assert want["upserts_new"] == 9


def test_id_reused_in_one_stream(removal_dev):
    """C. x removed and added again under its id with a new type and supply; of its old
    arcs one is re-created with new bounds, one is not, one has its only record
    before the removal, one is deleted again after being re-added, and one key has
    three records."""
    n = small_net()
    dev = removal_dev(n)
    T, P, x = n.T, n.P, n.x
    r, stats, want = dev.apply([
        arc(UPDATE_ARC, x, P[5], 2, 3),                 # its only record precedes the removal: dead
        delta(kind=REMOVE_NODE, id=x),
        delta(kind=ADD_NODE, id=x, excess=1, type=MID),
        arc(ADD_ARC, T[5], x, 2, 2, type=1),            # re-created with new bounds (T[6] → x is not)
        arc(ADD_ARC, x, P[3], 2, 1),
        arc(ADD_ARC, x, P[4], 1, 1),
        erase(x, P[4]),                                 # deleted after the re-add
        arc(ADD_ARC, T[7], x, 1, 4),
        arc(UPDATE_ARC, T[7], x, 2, 3),
        arc(UPDATE_ARC, T[7], x, 3, 2),                 # three records: two superseded
        arc(ADD_ARC, x, n.unsched, 1, BYPASS),          # the bypass of x's own unit
    ])
    assert (want["superseded"], want["killed"], want["upserts_new"], want["upserts_inplace"]) == (3, 3, 4, 0)
    assert dev.ref.nodes[x] == [1, MID]
    if dev.mode == "warm-slack":   # x's own segment is free again and every neighbour has slack
        assert r.raw["rebuilt"] == 0 and stats["inserted"] == 4


def test_id_removed_twice_in_one_stream(removal_dev):
    """C, second half: remove, add, arcs, remove, add, arcs. Only records after the
    LAST removal count; the arcs of the first re-addition die with it."""
    n = small_net()
    dev = removal_dev(n)
    T, P, x = n.T, n.P, n.x
    r, stats, want = dev.apply([
        delta(kind=REMOVE_NODE, id=x),
        delta(kind=ADD_NODE, id=x, excess=0, type=4),
        arc(ADD_ARC, T[5], x, 1, 1),
        arc(ADD_ARC, x, P[3], 1, 1),
        delta(kind=REMOVE_NODE, id=x),
        delta(kind=ADD_NODE, id=x, excess=1, type=MID),
        arc(ADD_ARC, T[6], x, 2, 2),
        arc(ADD_ARC, x, P[3], 2, 2, type=1),
        arc(ADD_ARC, x, n.unsched, 1, BYPASS),
    ])
    assert (want["superseded"], want["killed"], want["upserts_new"], want["upserts_inplace"]) == (1, 4, 3, 0)
    if dev.mode == "warm-slack":
        assert r.raw["rebuilt"] == 0 and stats["inserted"] == 3


def test_head_only_and_tail_only_nodes_removed(removal_dev):
    """D. A node with only in-arcs and one with only out-arcs, removed in one stream."""
    n = small_net()
    dev = removal_dev(n)
    r, stats, want = dev.apply([delta(kind=REMOVE_NODE, id=n.z), delta(kind=REMOVE_NODE, id=n.y)])
    assert want["killed"] == 4
    removal_only(dev, r)


# ------------------------------------------------------------------ B ---
def hub_net():
    """A hub of degree 301 (150 tasks in, 150 PUs out, one leaf in) that carries the
    units of the 90 tasks no leaf serves, and 256 leaves of degree 2..5 (one of the
    first 60 tasks in, PUs out) that undercut it by one cost unit."""
    n = Net()
    n.T = [n.task() for _ in range(150)]
    n.H = n.node(OTHER)
    n.P = [n.pu(1) for _ in range(150)]
    for t in n.T:
        n.arc(t, n.H, 1, 2)
    for p in n.P:
        n.arc(n.H, p, 1, 1)
    n.L = []
    for i in range(256):
        leaf = n.node(OTHER)
        n.L.append(leaf)
        n.arc(n.T[i % 60], leaf, 1, 1)
        for j in range(i % 4 + 1 - (i == 0)):
            n.arc(leaf, n.P[(i + 37 * j) % 150], 1, 1)
    n.arc(n.L[0], n.H, 1, 0)            # the leaf next to the hub
    return n


@pytest.mark.parametrize("ne,hub_at", [(1, 0), (WAVE + 1, 10), (SBLK + 1, 100)])
def test_hub_removed_among_leaves(removal_dev, ne, hub_at):
    """B. One node of degree 301 carrying flow, removed in one stream with ne − 1 leaves
    of degree 2..5, one of them its neighbour: k_kill_nodes has one lane per removed
    node, and the lanes of a wave step together through segments of very different
    lengths. ne = 1: a lone lane; 65: the hub inside the first wave and one leaf alone
    in a second; 257: a second workgroup."""
    n = hub_net()
    assert n.degree(n.H) >= 300 and {n.degree(v) for v in n.L} == {2, 3, 4, 5}
    dev = removal_dev(n)
    if dev.csr_valid:
        f = {(int(s), int(d)): int(x) for s, d, x in dev.ctx.flows().tolist()}
        assert sum(x for (s, d), x in f.items() if s == n.H) >= 90   # (the tasks no leaf serves)
    order = n.L[:hub_at] + [n.H] + n.L[hub_at:ne - 1]
    assert len(order) == ne and (ne == 1 or n.L[0] in order)
    r, stats, want = dev.apply([arc(UPDATE_ARC, n.T[0], n.H, 1, 7)] + [delta(kind=REMOVE_NODE, id=v) for v in order])
    gone = set(order)
    assert want["killed"] == sum(s in gone or d in gone for s, d, *_ in n.arcs)
    removal_only(dev, r)


# ------------------------------------------------------------------ E ---
def seg_net():
    n = Net()
    n.T = [n.task() for _ in range(60)]
    n.W, n.E = n.node(OTHER), n.node(OTHER)
    n.PE = [n.pu(20) for _ in range(4)]
    n.PW = [n.pu(1) for _ in range(16)]
    for t in n.T:
        n.arc(t, n.W, 1, 50)
    for p in n.PW:
        n.arc(n.W, p, 1, 1)
    for t in n.T[:26]:
        n.arc(t, n.E, 1, 1)
    for p in n.PE:
        n.arc(n.E, p, 20, 1)
    return n


def test_segment_filled_then_reused_then_overflowed(any_ctx):
    """E. An aggregator whose segment is one scan chunk (capacity 64 by the build's
    rule for its 30 arcs): filled exactly in place; then k arcs deleted and k new
    ones inserted in one stream, which must land in the positions the deleted ones
    left inert (no rebuild); then more inserts than free positions, which must
    rebuild the CSR and leave the same graph and optimum."""
    n = seg_net()
    deg = n.degree(n.E)
    cap = seg_capacity(deg)
    assert (deg, cap) == (30, SCAN)
    dev = Dev(any_ctx, n)
    dev.prime()                          # from here on the CSR has slack
    r, stats, want = dev.apply([arc(ADD_ARC, t, n.E, 1, 1) for t in n.T[26:26 + cap - deg]])
    assert r.raw["rebuilt"] == 0 and stats["inserted"] == cap - deg == 34   # full: 64 of 64
    k = 10
    r, stats, want = dev.apply([erase(t, n.E) for t in n.T[:k]] + [arc(ADD_ARC, n.E, p, 1, 1) for p in n.PW[:k]])
    assert r.raw["rebuilt"] == 0 and (stats["inserted"], stats["killed"]) == (k, k)
    r, stats, want = dev.apply([erase(t, n.E) for t in n.T[k:k + 3]] +
                               [arc(ADD_ARC, n.E, p, 1, 1) for p in n.PW[k:k + 5]])
    assert r.raw["rebuilt"] == 1 and want["upserts_new"] == 5 and stats["killed"] == 3


def holes_net():
    n = Net()
    n.T = [n.task() for _ in range(50)]
    n.idle = [n.task() for _ in range(80)]       # only their bypass arcs, until the stream
    n.X = n.node(OTHER)
    n.P = [n.pu(15) for _ in range(10)]
    for t in n.T:
        n.arc(t, n.X, 1, 1)
    for p in n.P:
        n.arc(n.X, p, 15, 1)
    return n


def test_tail_and_holes_of_one_segment_claimed_in_one_stream(any_ctx):
    """E, across two scan chunks. A segment of 128 positions, 60 of them used: one stream
    deletes 20 of its arcs and inserts 80. 68 inserts take the never-used tail (one
    atomic per wave hands them consecutive positions), the other 12 must find the holes
    by scanning 64-position chunks — while the tail's positions are being claimed next
    to them: a scanned chunk must not hand out a position a lane of the tail already
    holds. Every new arc is the only cheap route of one task's unit."""
    n = holes_net()
    deg = n.degree(n.X)
    cap = seg_capacity(deg)
    assert (deg, cap) == (60, 2 * SCAN)
    dev = Dev(any_ctx, n)
    dev.prime()
    base = dev.solve()
    holes, ins = 20, 80
    assert cap - deg < ins <= cap - deg + holes
    r, stats, want = dev.apply([erase(t, n.X) for t in n.T[:holes]] + [arc(ADD_ARC, t, n.X, 1, 1) for t in n.idle])
    assert r.raw["rebuilt"] == 0 and (stats["inserted"], stats["killed"]) == (ins, holes)
    assert base.cost - r.cost == (ins - holes) * (BYPASS - 2)


# ------------------------------------------------------------------ F ---
def wave_net():
    n = Net()
    n.T1 = [n.task() for _ in range(140)]
    n.T2 = [n.task() for _ in range(30)]
    n.idle = [n.task() for _ in range(140)]      # only their bypass arcs, until the stream
    n.G1, n.G2 = n.node(OTHER), n.node(OTHER)
    n.P1 = [n.pu(30) for _ in range(10)]
    n.P2 = [n.pu(10) for _ in range(10)]
    n.P3 = [n.pu(1) for _ in range(39)]          # (PUs nothing leads to: the sink's degree)
    for t in n.T1:
        n.arc(t, n.G1, 1, 1)
    for t in n.T2:
        n.arc(t, n.G2, 1, 1)
    for p in n.P1:
        n.arc(n.G1, p, 30, 1)
    for p in n.P2:
        n.arc(n.G2, p, 10, 1)
    return n


def test_shared_and_distinct_segments_in_one_wave(any_ctx):
    """F. One stream whose first 66 arc records interleave three heads — two
    aggregators and the sink — followed by 70 records into a single head. Lanes of
    one wave that insert into the same segment take consecutive positions from one
    atomic per segment (wave_fill). Every new arc is the only cheap route of one
    task's unit, so an arc lost to a position claimed twice changes the optimum."""
    n = wave_net()
    free = {v: seg_capacity(n.degree(v)) - n.degree(v) for v in (n.G1, n.G2, n.sink)}
    assert (free[n.G1], free[n.G2], free[n.sink]) == (106, 24, 67)
    dev = Dev(any_ctx, n)
    dev.prime()
    recs = []
    for i in range(22):
        recs += [arc(ADD_ARC, n.idle[3 * i], n.G1, 1, 1), arc(ADD_ARC, n.idle[3 * i + 1], n.G2, 1, 1),
                 arc(ADD_ARC, n.idle[3 * i + 2], n.sink, 1, 3)]
    assert len(recs) >= WAVE
    recs += [arc(ADD_ARC, t, n.G1, 1, 1) for t in n.idle[66:136]]
    per_head = {v: sum(int(x["dst"]) == v for x in recs) for v in free}
    assert per_head[n.G1] >= WAVE and all(per_head[v] <= free[v] for v in free)
    base = dev.solve()
    r, stats, want = dev.apply(recs)
    assert r.raw["rebuilt"] == 0 and stats["inserted"] == len(recs) == 136
    # each of the 136 units left its bypass arc for its new route
    assert base.cost - r.cost == 92 * (BYPASS - 2) + 22 * (BYPASS - 2) + 22 * (BYPASS - 3)


# ------------------------------------------------------------------ G ---
def churn_net():
    n = Net()
    n.T = [n.task() for _ in range(300)]
    n.G = n.node(OTHER)
    n.P = [n.pu(30) for _ in range(10)]
    for t in n.T:
        n.arc(t, n.G, 1, 1)
    for p in n.P:
        n.arc(n.G, p, 30, 1)
    return n


class HashModel:
    """The size and load of the store's (src, dst) index as ensure_hash
    (ks_engine_io.hip) keeps them: before a stream of narc arc records the index is
    emptied and refilled — sized to 4 × (live + narc) + 1024, a power of two from
    1,024 that never shrinks — unless live + tombstones + narc stay within half of it.
    A deleted key leaves a tombstone; a re-created one takes a fresh entry."""

    def __init__(self):
        self.cap = self.live = self.tombs = self.rehashes = 0

    def stream(self, narc, created, deleted):
        if not self.cap or 2 * (self.live + self.tombs + narc) > self.cap:
            cap = self.cap or 1024
            while cap < 4 * (self.live + narc) + 1024:
                cap <<= 1
            self.cap, self.tombs = cap, 0
            self.rehashes += 1
        self.live += created - deleted
        self.tombs += deleted


def test_rehash_under_tombstones():
    """G. The same 300 keys of a store of ~620 arcs deleted and re-created round after
    round, on a context of its own (its index starts from nothing): the tombstones
    force a rehash by a round the test derives from ensure_hash's rule, and twice
    that many rounds run. Then every surviving arc is updated in place."""
    n = churn_net()
    keys = [(t, n.G) for t in n.T]
    m = HashModel()
    m.stream(len(n.arcs), len(n.arcs), 0)        # the load
    m.stream(1, 1, 0)                            # the priming arc
    loaded, by = m.rehashes, None
    for rnd in range(1, 100):
        m.stream(len(keys), 0, len(keys))
        m.stream(len(keys), len(keys), 0)
        if m.rehashes > loaded:
            by = rnd
            break
    assert by is not None and 2 <= by <= 8, by
    with native.Context(0, cell_nodes=-1, warm_start=1) as c:
        dev = Dev(c, n, warm=True)
        dev.prime()
        for rnd in range(2 * by):
            r, stats, want = dev.apply([erase(s, d) for s, d in keys])
            assert stats["killed"] == len(keys)
            r, stats, want = dev.apply([arc(ADD_ARC, s, d, 1, 1 + rnd % 3, type=rnd % 2) for s, d in keys])
            assert want["upserts_new"] == len(keys)
        every = [arc(UPDATE_ARC, s, d, cap, cost + 1, low, type=dev.ref.atype[(s, d)])
                 for (s, d), (low, cap, cost) in sorted(dev.ref.arcs.items())]
        r, stats, want = dev.apply(every)
        assert r.raw["rebuilt"] == 0
        assert stats["updated"] == stats["live_arcs"] == len(every) == len(n.arcs) + 1
