"""GPU: ks_remove_resources — a resource subtree leaves the device-resident graph, the
tasks bound in it are evicted, the surviving resource arcs get their capacities —
against the rule restated on the host (tests/remove_ref.py), against the store's
reference (tests/store_ref.py) and against the host path it replaces (the same records
through ks_apply_deltas on a twin context). Every case runs before any solve, after a
solve with a commit on the cell path and on the engine path, and with warm_start = 1."""
import ctypes as C

import numpy as np
import pytest

from commit_ref import arc_table
from ksched_amd import gen, native
from oracle import ko, sched_ref
from preempt_ref import table_graph
from remove_ref import (TOY_ARCS, TOY_BINDINGS, TOY_M1, TOY_NTYPE, TOY_R1, TOY_SUPPLY, TOY_U, BelowLowerBound,
                        remove_reference)
from store_ref import StoreRef, check_counters, same_store

pytestmark = pytest.mark.gpu

PLACE, PREEMPT = native.KS_DELTA_PLACE, native.KS_DELTA_PREEMPT
STATES = {"fresh": {}, "cell": dict(cell_nodes=0), "engine": dict(cell_nodes=-1),
          "warm": dict(cell_nodes=-1, warm_start=1)}
EVERY_STATE = pytest.mark.parametrize("state", list(STATES))
BOTH_MODES = pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
PREEMPTION_COST = 200


# ---------------------------------------------------------------------- graphs ---
class Spec:
    """A graph in its two forms: running=False, nothing placed yet (a solve and a commit
    place the tasks); running=True, the state a preemptive commit leaves (the bound tasks'
    running arcs, type 1 with low 0), with .bindings to seed."""

    def __init__(self, ntype, supply, arcs, bindings):
        self.ntype, self.supply, self.arcs, self.bindings = ntype, supply, arcs, bindings

    def graph(self, running: bool) -> gen.Graph:
        rows = [(s, d, *a) for (s, d), a in self.arcs if running or a[3] != 1]
        a = np.asarray(rows, np.int64).reshape(-1, 6)
        return gen.Graph(np.asarray(self.ntype, np.int32), np.asarray(self.supply, np.int64), a[:, 0].copy(),
                         a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), a[:, 4].copy(), a[:, 5].astype(np.int32))


TOY = Spec(TOY_NTYPE, TOY_SUPPLY, list(TOY_ARCS.items()), TOY_BINDINGS)


class Cluster(Spec):
    """SINK 1, X 2, R racks, R·mpr machines (machine k in rack k // mpr), one PU each, one
    unscheduled aggregator U, T tasks. Task i has arcs into U (100), X (50), its machine
    desig[i] (cost 1, when not None) and the racks rack_prefs[i] (30): with room on every
    designated machine the optimum places each task there, so the bindings of a solve
    are those of the running form. interleave: a rack's arcs into its machines alternate
    with the tasks' arcs into the rack in the arc order."""

    def __init__(self, R, mpr, slots, desig, rack_prefs=None, interleave=False):
        T, M = len(desig), R * mpr
        self.SINK, self.X, self.R0 = 1, 2, 3
        self.M0 = self.R0 + R
        self.P0 = self.M0 + M
        self.U = self.P0 + M
        self.T0 = self.U + 1
        n = self.T0 + T - 1
        ntype = [0] * n
        supply = [0] * n
        ntype[0], supply[0] = 3, -T
        for k in range(M):
            ntype[self.M0 + k - 1], ntype[self.P0 + k - 1] = 4, 2
        for i in range(T):
            ntype[self.T0 + i - 1], supply[self.T0 + i - 1] = 1, 1
        rack_prefs = rack_prefs or [()] * T
        into_rack = [[] for _ in range(R)]
        for i, rs in enumerate(rack_prefs):
            for r in rs:
                into_rack[r].append(((self.T0 + i, self.R0 + r), (0, 1, 30, 0)))
        arcs = [((self.U, self.SINK), (0, T, 0, 0))]
        for r in range(R):
            arcs.append(((self.X, self.R0 + r), (0, mpr * slots, 0, 0)))
            down = [((self.R0 + r, self.M0 + r * mpr + j), (0, slots, 0, 0)) for j in range(mpr)]
            if interleave:
                mixed, pref = [], list(into_rack[r])
                per = max(1, len(pref) // max(1, len(down)))
                for a in down:
                    mixed.append(a)
                    mixed += pref[:per]
                    pref = pref[per:]
                arcs += mixed + pref
            else:
                arcs += down + into_rack[r]
        for k in range(M):
            arcs += [((self.M0 + k, self.P0 + k), (0, slots, 0, 0)), ((self.P0 + k, self.SINK), (0, slots, 0, 0))]
        bindings = {}
        for i, m in enumerate(desig):
            t = self.T0 + i
            arcs += [((t, self.U), (0, 1, 100, 0)), ((t, self.X), (0, 1, 50, 0))]
            if m is not None:
                arcs += [((t, self.M0 + m), (0, 1, 1, 0)), ((t, self.P0 + m), (0, 1, 0, 1))]
                bindings[t] = self.P0 + m
        assert all(list(bindings.values()).count(p) <= slots for p in set(bindings.values()))
        super().__init__(ntype, supply, arcs, bindings)

    def machines(self, r):
        mpr = (self.P0 - self.M0) // (self.M0 - self.R0)
        return [self.M0 + r * mpr + j for j in range(mpr)]


# --------------------------------------------------------------------- harness ---
def triples(deltas) -> list:
    return list(zip(deltas["type"].tolist(), deltas["task"].tolist(), deltas["pu"].tolist()))


class Snapshot:
    """The device-resident graph as the rule's and the oracle's input."""

    def __init__(self, ctx):
        self.nodes, self.arcs = ctx.graph()
        n = int(self.nodes["id"].max())
        self.ntype = np.zeros(n, np.int32)
        self.supply = np.zeros(n, np.int64)
        self.ntype[self.nodes["id"].astype(np.int64) - 1] = self.nodes["type"]
        self.supply[self.nodes["id"].astype(np.int64) - 1] = self.nodes["excess"]
        a = self.arcs
        self.table = {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
                      for s, d, lo, c, co, ty in zip(a["src"], a["dst"], a["low"], a["cap"], a["cost"], a["type"])}
        self.alive = set(self.nodes["id"].tolist())

    def graph(self) -> gen.Graph:
        return table_graph(self.ntype, self.supply, self.table)

    def store(self) -> StoreRef:
        nodes = {int(i): [int(e), int(t)] for i, e, t in zip(self.nodes["id"], self.nodes["excess"], self.nodes["type"])}
        return StoreRef(nodes, {k: a[:3] for k, a in self.table.items()}, {k: a[3] for k, a in self.table.items()})


def prepare(ctx, spec, state, preemptive):
    """Bring ctx to the state; → (the graph loaded, the bindings the device keeps)."""
    if state == "fresh":
        g = spec.graph(running=True)
        ctx.load_graph(g)
        ctx.set_bindings(spec.bindings)
        return g, dict(spec.bindings)
    g = spec.graph(running=False)
    ctx.load_graph(g)
    ctx.solve()
    if preemptive:
        deltas, _ = ctx.commit_preemptive(continuation=0, preemption=PREEMPTION_COST)
    else:
        deltas, _ = ctx.commit_schedule(continuation=0)
    assert set(deltas["type"].tolist()) <= {PLACE}
    if state == "warm":
        # a second solve: the call then meets a valid residual CSR with the solution in place
        # (after the commit alone a rebuild is pending: the load's tight segments had no room
        # for the running arcs), and the solve after it starts warm
        ctx.solve()
    return g, dict(zip(deltas["task"].tolist(), deltas["pu"].tolist()))


def remove_and_check(ctx, roots, bindings, preemptive, caps=True):
    """One call against the rule, the store's reference and the host path; → (the rule's
    result, the device's (removed, evicted, stats))."""
    before = Snapshot(ctx)
    ref = remove_reference(before.graph(), roots, bindings, caps, preemptive and caps, alive=before.alive)
    sref = before.store()
    want = sref.apply(ref.stream)
    with native.Context(0) as twin:                               # the host path: the same records
        twin.load_arrays(before.nodes, before.arcs)
        twin.apply_deltas(ref.stream)
        same_store(twin, sref)
        twin_rows = Snapshot(twin).table
    removed, evicted, stats = ctx.remove_resources(roots, resource_caps=caps, preemptive=preemptive and caps)
    assert removed.tolist() == ref.removed
    assert triples(evicted) == [(PREEMPT, t, p) for t, p in ref.evicted]
    assert stats == ref.stats and stats["records"] == stats["nodes_removed"] + stats["cap_updates"]
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == before.alive - set(ref.removed)
    check_counters(ctx.store_stats(), want, exact=True)
    return ref, (removed, evicted, stats)


def resolve_and_check(ctx, g0, ref, state, preemptive):
    """The solve after the call: where a pinned commit deleted them, the evicted tasks'
    arcs come back first (the host's business); then cost, flow, the flows and the
    scheduling deltas against the oracle and the rule's bindings."""
    gone = set(ref.removed)
    evicted = [t for t, _ in ref.evicted]
    if state != "fresh" and not preemptive and evicted:
        mine = set(evicted)
        t0 = arc_table(g0)
        rows = [(native.KS_ADD_ARC, s, d, *a) for (s, d), a in t0.items() if s in mine and d not in gone and a[3] != 1]
        now = Snapshot(ctx).table
        sink = int(np.nonzero(np.asarray(g0.ntype) == 3)[0][0]) + 1
        back: dict = {}
        for _, s, d, *_ in rows:                                  # the +1 on the aggregator → sink arcs
            if (d, sink) in t0 and g0.ntype[d - 1] == 0:
                back[d] = back.get(d, 0) + 1
        for u, k in back.items():
            lo, cap, co, ty = now.get((u, sink), (0, 0, t0[(u, sink)][2], 0))
            rows.append((native.KS_ADD_ARC, u, sink, lo, cap + k, co, ty))
        recs = np.zeros(len(rows), native.DELTA_DT)
        for x, (kind, s, d, lo, cap, co, ty) in zip(recs, rows):
            x["kind"], x["src"], x["dst"], x["low"], x["cap"], x["cost"], x["type"] = kind, s, d, lo, cap, co, ty
        ctx.apply_deltas(recs)
    r = ctx.solve()
    snap = Snapshot(ctx)
    g = snap.graph()
    st, cost, flow, _ = ko.cost_scaling(g)
    assert st == 0 and (r.cost, r.flow) == (cost, flow)
    f = ctx.flows()
    got = dict(zip(zip(f["src"].tolist(), f["dst"].tolist()), f["flow"].tolist()))
    vec = np.asarray([got.pop((int(s), int(d)), 0) for s, d in zip(g.src, g.dst)], np.int64)
    assert not got
    vst, vcost, _ = ko.verify(g, vec)
    assert (vst, vcost) == (0, cost)
    tasks = (np.nonzero(snap.ntype == 1)[0] + 1).tolist()
    d = triples(ctx.scheduling_deltas(commit=False))
    assert d == sched_ref.scheduling_deltas(ref.bindings, ctx.task_mapping(), tasks)
    again = [kind for kind, t, _ in d if t in set(evicted)]
    assert set(again) <= {PLACE}                                   # an evicted task is unbound: never a MIGRATE
    return r, d


def run_case(spec, roots, state, preemptive, caps=True):
    with native.Context(0, **STATES[state]) as ctx:
        g0, bindings = prepare(ctx, spec, state, preemptive)
        ref, dev = remove_and_check(ctx, roots, bindings, preemptive, caps)
        r, d = resolve_and_check(ctx, g0, ref, state, preemptive)
        if state == "warm":
            assert r.raw["warm_started"] == 1
        return ref, dev, r, d


# ----------------------------------------------------------------------- cases ---
@EVERY_STATE
@BOTH_MODES
@pytest.mark.parametrize("caps", [True, False], ids=["caps", "nocaps"])
def test_toy_one_machine(state, preemptive, caps):
    ref, (removed, evicted, stats), _, _ = run_case(TOY, [TOY_M1], state, preemptive, caps)
    # (the walk follows arcs: a pinned commit's capacity rule deletes the arc M1 → P1 once M1 is
    # full, and P1 then stays — run_case held the device to the rule on the device's own arcs)
    if state == "fresh" or preemptive:
        assert removed.tolist() == [5, 9] and stats["pus_removed"] == 1
    assert TOY_M1 in removed.tolist()
    if state == "fresh":                                           # the literals of the CPU suite
        assert triples(evicted) == [(PREEMPT, 14, 9), (PREEMPT, 15, 9)]
        assert stats["arcs_removed"] == 7
        assert stats["cap_updates"] == (0 if not caps else 1 if preemptive else 6)
        if caps:
            assert ref.arcs[(2, 3)] == (0, 2 if preemptive else 1, 0, 0)
            assert ref.arcs[(2, 4)] == (0, 4 if preemptive else 3, 0, 0)
            assert ref.arcs[(3, 6)] == (0, 2 if preemptive else 1, 0, 0)


@EVERY_STATE
@BOTH_MODES
@pytest.mark.parametrize("roots,removed", [([TOY_M1, TOY_R1], [3, 5, 6, 9, 10]), ([TOY_M1, TOY_M1, 8, TOY_M1], [5, 8, 9, 12]),
                                           ([9], [9])], ids=["nested", "duplicate", "pu"])
def test_nested_duplicate_and_pu_roots(state, preemptive, roots, removed):
    _, (got, _, stats), _, _ = run_case(TOY, roots, state, preemptive)
    if state == "fresh" or preemptive:                              # (pinned: a full machine's arc into its PU is gone)
        assert got.tolist() == removed
    assert set(roots) <= set(got.tolist()) <= set(removed)
    assert stats["roots"] == len(set(roots))


def two_chunk_rack() -> Cluster:
    """Rack 0: 70 machines, and 80 task arcs into the rack mixed between its arcs into the
    machines: its forward arcs span two 64-position chunks with in-arcs among them."""
    desig = [i % 140 for i in range(100)]
    return Cluster(2, 70, 2, desig, rack_prefs=[(0,) if i < 80 else (1,) for i in range(100)], interleave=True)


@EVERY_STATE
@BOTH_MODES
def test_only_forward_arcs_are_followed(state, preemptive):
    spec = two_chunk_rack()
    ref, (removed, evicted, stats), _, _ = run_case(spec, [spec.R0], state, preemptive)
    assert removed.tolist() == sorted([spec.R0] + spec.machines(0) + [m + 140 for m in spec.machines(0)])
    assert stats["pus_removed"] == 70
    assert evicted["task"].tolist() == [spec.T0 + i for i in range(70)]   # tasks 0..69 ran in rack 0, the rest in rack 1
    # (X and the 80 tasks with an arc into the rack lie against an arc's direction: none is in the list)


_HUB = {}


def hub_rack() -> Cluster:
    """Rack 0: 100 machines and 4,100 task arcs into it — more than 4,096 residual
    positions, the engine's heavy-hub class."""
    if "spec" not in _HUB:
        T = 4100
        desig = [i % 110 if i < 330 else None for i in range(T)]
        _HUB["spec"] = Cluster(2, 100, 3, desig, rack_prefs=[(0,)] * T)
    return _HUB["spec"]


@EVERY_STATE
@pytest.mark.parametrize("whole", [True, False], ids=["rack", "machine"])
def test_heavy_hub_rack(state, whole):
    spec = hub_rack()
    roots = [spec.R0] if whole else [spec.M0 + 7]
    ref, (removed, evicted, stats), _, _ = run_case(spec, roots, state, True)
    if whole:
        assert stats["nodes_removed"] == 201 and stats["pus_removed"] == 100
        assert stats["arcs_removed"] >= 4100 + 300
    else:
        assert removed.tolist() == [spec.M0 + 7, spec.P0 + 7]
    assert evicted.shape[0] == (300 if whole else 3)


@EVERY_STATE
@BOTH_MODES
def test_eviction_order_across_waves(state, preemptive):
    """200 bound tasks, 130 of them on removed PUs, their ids interleaved with the
    survivors': the eviction scan's positions cross wave boundaries."""
    on_removed = [(i * 13) % 20 < 13 for i in range(200)]
    assert sum(on_removed) == 130
    desig, a, b = [], 0, 0
    for x in on_removed:                                            # rack 0 (10 machines) leaves, rack 1 stays
        if x:
            desig.append(a % 10)
            a += 1
        else:
            desig.append(10 + b % 10)
            b += 1
    spec = Cluster(2, 10, 14, desig)                                # (a slot to spare: no machine → PU arc at capacity 0)
    ref, (removed, evicted, stats), _, d = run_case(spec, [spec.R0], state, preemptive)
    want = [spec.T0 + i for i, x in enumerate(on_removed) if x]
    assert evicted["task"].tolist() == want and stats["tasks_evicted"] == 130
    assert sorted(ref.bindings) == [spec.T0 + i for i, x in enumerate(on_removed) if not x]
    assert all(spec.P0 <= p < spec.P0 + 10 for p in evicted["pu"].tolist())


@EVERY_STATE
def test_an_aggregator_goes_alone(state):
    spec = Cluster(2, 2, 2, [0, 0, 1, 2, None, None])
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        ref, (removed, evicted, stats) = remove_and_check(ctx, [spec.U], bindings, True)
        assert removed.tolist() == [spec.U] and evicted.shape[0] == 0
        assert (stats["pus_removed"], stats["tasks_evicted"], stats["arcs_removed"]) == (0, 0, 7)
        r = ctx.solve()                                             # every task still fits on a machine
        st, cost, flow, _ = ko.cost_scaling(Snapshot(ctx).graph())
        assert st == 0 and (r.cost, r.flow) == (cost, flow)


@EVERY_STATE
def test_every_machine_removed(state):
    """With preemptive bindings the next solve routes every task through its aggregator."""
    spec = Cluster(2, 3, 2, [0, 1, 2, 3, 4, 5, 0, None])
    roots = [spec.M0 + k for k in range(6)]
    ref, (removed, evicted, stats), r, d = run_case(spec, roots, state, True)
    assert stats["nodes_removed"] == 12 and stats["pus_removed"] == 6
    # (a committed task's arc into U carries the preemption cost, the running form's 100)
    assert (r.cost, r.flow) == (8 * (100 if state == "fresh" else PREEMPTION_COST), 8)
    assert d == [] and ref.bindings == {}


@EVERY_STATE
def test_removed_ids_can_be_reused(state):
    """ADD_NODE of three removed ids with new arcs succeeds: the host's node table followed."""
    spec = Cluster(2, 2, 2, [0, 0, 1, 2, None, None])
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        ref, (removed, _, _) = remove_and_check(ctx, [spec.R0], bindings, True)
        assert removed.tolist() == [spec.R0, spec.M0, spec.M0 + 1, spec.P0, spec.P0 + 1]
        rk, m, p = spec.R0, spec.M0, spec.P0                         # a new rack with one machine of 4 slots
        rows = [(native.KS_ADD_NODE, rk, 0, 0, 0, 0, 0, 0), (native.KS_ADD_NODE, m, 0, 0, 0, 0, 0, 4),
                (native.KS_ADD_NODE, p, 0, 0, 0, 0, 0, 2),
                (native.KS_ADD_ARC, 0, spec.X, rk, 0, 4, 0, 0), (native.KS_ADD_ARC, 0, rk, m, 0, 4, 0, 0),
                (native.KS_ADD_ARC, 0, m, p, 0, 4, 0, 0), (native.KS_ADD_ARC, 0, p, spec.SINK, 0, 4, 0, 0)]
        recs = np.zeros(len(rows), native.DELTA_DT)
        for x, (kind, nid, s, d, lo, cap, co, ty) in zip(recs, rows):
            x["kind"], x["id"], x["src"], x["dst"], x["low"], x["cap"], x["cost"], x["type"] = kind, nid, s, d, lo, cap, co, ty
        ctx.apply_deltas(recs)
        snap = Snapshot(ctx)
        assert {rk, m, p} <= snap.alive and snap.table[(m, p)] == (0, 4, 0, 0)
        r = ctx.solve()
        st, cost, flow, _ = ko.cost_scaling(snap.graph())
        assert st == 0 and (r.cost, r.flow) == (cost, flow) and flow == 6
        mp = ctx.task_mapping()
        assert p in set(mp.values())                                # the evicted tasks land on the new machine


# -------------------------------------------------------------------- refusals ---
def test_refusals_change_nothing():
    g = TOY.graph(running=True)
    with native.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        ctx.load_graph(g)
        ctx.set_bindings(TOY_BINDINGS)
        ctx.solve()
        before = Snapshot(ctx)
        d0 = ctx.scheduling_deltas(commit=False)
        s0 = ctx.store_stats()

        def unchanged():
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive
            assert (now.nodes == before.nodes).all()
            assert ctx.store_stats() == s0
            assert (ctx.scheduling_deltas(commit=False) == d0).all()    # the bindings and the solution stand

        nr, ne = C.c_size_t(), C.c_size_t()
        rm = np.zeros(8, np.uint64)
        ev = np.zeros(8, native.SCHED_DELTA_DT)

        def call(flags, roots, rbuf=rm, rcap=8, ebuf=ev, ecap=8):
            ids = np.asarray(roots, np.uint64)
            return L.ks_remove_resources(h, flags, ids.ctypes.data, ids.shape[0], None if rbuf is None else rbuf.ctypes.data,
                                         rcap, C.byref(nr), None if ebuf is None else ebuf.ctypes.data, ecap,
                                         C.byref(ne), None)

        for bad in (14, 1, 10 ** 6, 0):                             # a task, the sink, beyond the graph
            assert call(1, [TOY_M1, bad]) == native.KS_E_INVALID
            assert str(bad) in L.ks_last_error(h).decode()
            unchanged()
        assert call(1, [TOY_M1], rcap=1) == native.KS_E_INVALID     # rcap short: the counts are written
        assert (nr.value, ne.value) == (2, 2)
        unchanged()
        nr.value = ne.value = 0
        assert call(1, [TOY_M1], ecap=1) == native.KS_E_INVALID
        assert (nr.value, ne.value) == (2, 2)
        unchanged()
        nr.value = ne.value = 0
        assert call(1, [TOY_R1], rbuf=None, rcap=0, ebuf=None, ecap=0) == native.KS_OK   # a probe
        assert (nr.value, ne.value) == (5, 3)
        unchanged()
        for flags in (2, 4, 1 | 8):                                 # PREEMPTIVE alone, unknown bits
            assert call(flags, [TOY_M1]) == native.KS_E_INVALID
            unchanged()


def test_a_dead_root_is_refused():
    with native.Context(0) as ctx:
        ctx.load_graph(TOY.graph(running=True))
        ctx.set_bindings(TOY_BINDINGS)
        removed, _, _ = ctx.remove_resources([TOY_M1])
        assert removed.tolist() == [5, 9]
        before = Snapshot(ctx)
        with pytest.raises(native.KsError) as e:
            ctx.remove_resources([6, 9])
        assert e.value.code == native.KS_E_INVALID and "9" in str(e.value)
        now = Snapshot(ctx)
        assert now.table == before.table and now.alive == before.alive


def test_a_capacity_below_its_lower_bound_is_refused():
    arcs = dict(TOY_ARCS)
    arcs[(2, 3)] = (3, 4, 0, 0)                                     # X → R1: lower bound 3, the new capacity would be 2
    spec = Spec(TOY_NTYPE, TOY_SUPPLY, list(arcs.items()), TOY_BINDINGS)
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(TOY_BINDINGS)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        with pytest.raises(BelowLowerBound):
            remove_reference(before.graph(), [TOY_M1], TOY_BINDINGS, True, True)
        with pytest.raises(native.KsError) as e:
            ctx.remove_resources([TOY_M1], preemptive=True)
        assert e.value.code == native.KS_E_VERIFY
        now = Snapshot(ctx)
        assert now.table == before.table and now.alive == before.alive
        assert {k: v for k, v in ctx.store_stats().items() if k not in ("rebuilds", "residual_slots")} == \
               {k: v for k, v in s0.items() if k not in ("rebuilds", "residual_slots")}
        removed, evicted, _ = ctx.remove_resources([TOY_M1], resource_caps=False)   # the bindings stood
        assert removed.tolist() == [5, 9] and evicted["task"].tolist() == [14, 15]


def test_two_sinks_refuse_the_capacities():
    ntype = list(TOY_NTYPE) + [3]
    supply = list(TOY_SUPPLY) + [0]
    spec = Spec(ntype, supply, list(TOY_ARCS.items()) + [((13, 20), (0, 1, 0, 0))], TOY_BINDINGS)
    with native.Context(0, auto_sink=0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        before = Snapshot(ctx)
        with pytest.raises(native.KsError) as e:
            ctx.remove_resources([TOY_M1])
        assert e.value.code == native.KS_E_INVALID
        assert Snapshot(ctx).table == before.table
        removed, _, stats = ctx.remove_resources([TOY_M1], resource_caps=False)
        assert removed.tolist() == [5, 9] and stats["cap_updates"] == 0
