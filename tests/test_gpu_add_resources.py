"""GPU: ks_add_resources — machines, racks and PUs join the device-resident graph, the arcs
above the attach point gain the new slots — against the rule restated on the host
(tests/grow_ref.py), against the store's reference (tests/store_ref.py), against the host path
it replaces (the same records through ks_apply_deltas on a twin context) and against an
independent rule: the capacity refresh of ks_complete_tasks (a BFS from the sink, not this
call's walk up the tree edges) has nothing to write after a call with full chains. Every case
runs before any solve, after a solve, after a pinned commit that filled a machine (its rack's
arc into it left the store), after a preemptive commit and under warm_start = 1."""
import ctypes as C

import numpy as np
import pytest

from grow_ref import EXTRA, TREE, chain, grow_reference, tree_parents
from ksched_amd import gen, native
from store_ref import check_counters, same_store
from test_gpu_add_tasks import resolve_and_check
from test_gpu_complete_tasks import live_tasks
from test_gpu_remove_resources import PREEMPTION_COST, TOY, Cluster, Snapshot

pytestmark = pytest.mark.gpu

# state → (context options, what follows the load, the capacity rule in force: preemptive?)
STATES = {"fresh": ({}, "fresh", True), "solved": ({}, "solved", False), "pinned": (dict(cell_nodes=-1), "pinned", False),
          "preemptive": ({}, "preemptive", True), "warm": (dict(cell_nodes=-1, warm_start=1), "warm", False)}
EVERY_STATE = pytest.mark.parametrize("state", list(STATES))
TWO_STATES = pytest.mark.parametrize("state", ["fresh", "pinned"])
INVALID, RANGE = native.KS_E_INVALID, native.KS_E_RANGE


# ---------------------------------------------------------------------- graphs ---
def grid() -> Cluster:
    """2 racks × 2 machines × 1 PU of 3 slots, 9 tasks: three designated to machine 0 (they fill
    it), one to machine 1, five that go anywhere through X."""
    return Cluster(2, 2, 3, [0, 0, 0, 1] + [None] * 5)


def refresh(ctx, preemptive) -> int:
    """ks_complete_tasks(k = 0, resource caps): the records it wrote."""
    _, st = ctx.complete_tasks([], resource_caps=True, preemptive=preemptive, unsched_ids=[])
    return st["cap_updates"]


def bring(ctx, spec, state) -> bool:
    """Bring ctx to the state with capacities that are consistent under its rule; → preemptive?"""
    _, what, preemptive = STATES[state]
    if isinstance(spec, gen.Graph):
        ctx.load_graph(spec)
    elif what == "fresh":
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(spec.bindings)
    else:
        ctx.load_graph(spec.graph(running=False))
    if what != "fresh":
        ctx.solve()
    if what in ("pinned", "warm"):
        ctx.commit_schedule(continuation=0)
    elif what == "preemptive":
        ctx.commit_preemptive(continuation=0, preemption=PREEMPTION_COST)
    refresh(ctx, preemptive)
    assert refresh(ctx, preemptive) == 0
    if what == "warm":
        ctx.solve()                                                # the call meets a valid residual CSR
    return preemptive


def open_ctx(state):
    return native.Context(0, **STATES[state][0])


def top(ctx) -> int:
    return int(Snapshot(ctx).nodes["id"].max())


# --------------------------------------------------------------------- harness ---
def grow_and_check(ctx, nodes, edges, preemptive, state="fresh", solve=True, full_chain=True):
    """One call against the rule, the store's reference, the host path and the capacity refresh,
    then the solve after it against the oracle; → (the rule's result, the graph after, the solve)."""
    before = Snapshot(ctx)
    ref = grow_reference(before.graph(), nodes, edges, alive=before.alive)
    sref = before.store()
    want = sref.apply(ref.stream)
    assert want["superseded"] == 0
    with native.Context(0) as twin:                               # the host path: the same records
        twin.load_arrays(before.nodes, before.arcs)
        if ref.stream.shape[0]:
            twin.apply_deltas(ref.stream)
        same_store(twin, sref)
        twin_rows = Snapshot(twin).table
    tasks = live_tasks(before)
    bound = ctx.bindings(tasks).tolist()
    builds = ctx.store_stats()["rebuilds"]
    stats = ctx.add_resources(nodes, edges)
    assert stats == ref.stats
    assert stats["records"] == stats["nodes"] + stats["sink_arcs"] + stats["arcs_added"] + stats["cap_updates"]
    assert stats["arcs_added"] + stats["cap_updates"] + stats["arcs_skipped"] == len(edges)
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == ref.alive == before.alive | {x[0] for x in nodes}
    counters = ctx.store_stats()                                  # (before the solve: its auto-sink edit is a stream)
    assert ctx.bindings(tasks).tolist() == bound
    if full_chain:
        assert refresh(ctx, preemptive) == 0                      # the independent rule agrees with every capacity
        assert Snapshot(ctx).table == after.table
    r = resolve_and_check(ctx) if solve else None
    if ref.stream.shape[0]:
        check_counters(counters, want, exact=state == "warm" and solve and ctx.store_stats()["rebuilds"] == builds)
    return ref, after, r


def flow_into_sink(ctx, pu) -> int:
    f = ctx.flows()
    return int(f["flow"][(f["src"] == pu) & (f["dst"] == 1)].sum())


# ----------------------------------------------------------------------- cases ---
@EVERY_STATE
def test_a_machine_with_its_pu_under_a_rack(state):
    spec = grid()
    parents = tree_parents(spec.ntype, dict(spec.arcs))
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        held = Snapshot(ctx).table.get((spec.X, spec.R0))
        nodes = [(n + 1, 4, 0, 0), (n + 2, 2, 4, 3)]
        edges = [(spec.R0, n + 1, 21, TREE), (n + 1, n + 2, 22, TREE)] + chain(parents, spec.R0, {(spec.X, spec.R0): 23})
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert after.table[(n + 2, 1)] == (0, 4, 3, 0) and after.table[(spec.R0, n + 1)] == (0, 4, 21, 0)
        assert after.table[(spec.X, spec.R0)] == ((held[0], held[1] + 4, held[2], held[3]) if held else (0, 4, 23, 0))


@EVERY_STATE
def test_a_rack_with_two_machines_under_the_root(state):
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        rack, m1, m2, p1, p2, p3 = range(n + 1, n + 7)
        nodes = [(rack, 0, 0, 0), (p1, 2, 2, 0), (m1, 4, 0, 0), (m2, 4, 0, 0), (p2, 2, 1, -4), (p3, 2, 5, 0)]
        edges = [(m1, p1, 0, TREE), (rack, m1, 1, TREE), (spec.X, rack, 2, TREE), (m2, p2, 0, TREE), (m2, p3, 0, TREE),
                 (rack, m2, 3, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert after.table[(spec.X, rack)] == (0, 8, 2, 0) and after.table[(rack, m2)] == (0, 6, 3, 0)
        assert ref.stats["arcs_added"] == 6 and ref.stats["cap_updates"] == 0


@EVERY_STATE
def test_a_lone_pu_under_the_machine_that_is_full(state):
    """Machine 0 holds its three designated tasks. After a pinned commit its capacity is 0 and the
    store holds neither rack → machine nor the arcs above it that fell to 0: the store's index
    says so and the arc is re-created with the input cost. Elsewhere the held arc is raised."""
    spec = grid()
    parents = tree_parents(spec.ntype, dict(spec.arcs))
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        m0 = spec.M0
        held = Snapshot(ctx).table.get((spec.R0, m0))
        if state in ("pinned", "warm"):
            assert held is None
        elif state != "solved":
            assert held == (0, 3, 0, 0)
        costs = {(spec.R0, m0): 31, (spec.X, spec.R0): 32}
        ref, after, _ = grow_and_check(ctx, [(n + 1, 2, 2, 9)], [(m0, n + 1, 30, TREE)] + chain(parents, m0, costs), pre, state)
        assert after.table[(m0, n + 1)] == (0, 2, 30, 0)
        assert after.table[(spec.R0, m0)] == ((0, held[1] + 2, 0, 0) if held else (0, 2, 31, 0))
        if state in ("pinned", "warm"):
            assert ref.stats["arcs_added"] >= 2


@EVERY_STATE
def test_an_empty_rack_then_a_machine_under_it(state):
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        ref, after, _ = grow_and_check(ctx, [(n + 1, 0, 0, 0)], [(spec.X, n + 1, 5, TREE)], pre, state, solve=False)
        assert ref.stats == dict(nodes=1, pus=0, slots=0, sink_arcs=0, arcs_added=0, cap_updates=0, arcs_skipped=1, records=1)
        assert (spec.X, n + 1) not in after.table and n + 1 in after.alive
        nodes = [(n + 2, 4, 0, 0), (n + 3, 2, 2, 0)]
        edges = [(n + 2, n + 3, 0, TREE), (n + 1, n + 2, 6, TREE), (spec.X, n + 1, 7, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre)
        assert after.table[(spec.X, n + 1)] == (0, 2, 7, 0) and ref.stats["arcs_added"] == 3


@pytest.mark.parametrize("state", ["fresh", "solved", "pinned"])
def test_trivial_an_arc_from_the_equivalence_class(state):
    """ksched's own topology: coordinator → machine → PU, and the equivalence class's arcs into
    the machines, which are EXTRA: they get the head's capacity and sum nothing."""
    g = gen.trivial(4, 3, 6)
    coord, ec = 2, 3 + 2 * 4 + 1
    with open_ctx(state) as ctx:
        pre = bring(ctx, g, state)
        n = top(ctx)
        nodes = [(n + 1, 4, 0, 0), (n + 2, 2, 3, 0)]
        edges = [(ec, n + 1, 0, EXTRA), (coord, n + 1, 0, TREE), (n + 1, n + 2, 0, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert after.table[(ec, n + 1)] == after.table[(coord, n + 1)] == (0, 3, 0, 0)
        # a PU joins machine 3: the coordinator's and the class's arcs into it both rise (or come back)
        mach = 3
        edges = [(mach, n + 3, 0, TREE), (ec, mach, 0, EXTRA), (coord, mach, 0, TREE)]
        was = [Snapshot(ctx).table.get(k, (0, 0, 0, 0))[1] for k in ((ec, mach), (coord, mach))]
        ref, after, _ = grow_and_check(ctx, [(n + 3, 2, 2, 0)], edges, pre)
        assert [after.table[k][1] for k in ((ec, mach), (coord, mach))] == [was[0] + 2, was[1] + 2]


@pytest.mark.parametrize("state", ["fresh", "pinned", "preemptive"])
@pytest.mark.parametrize("seed", [3, 8])
def test_quincy_a_machine_and_a_rack(state, seed):
    g = gen.quincy(40, 6, 2, 3, seed)
    parents = tree_parents(g.ntype.tolist(), {(int(s), int(d)): 0 for s, d in zip(g.src, g.dst)})
    with open_ctx(state) as ctx:
        pre = bring(ctx, g, state)
        n = top(ctx)
        rack0, mach0 = 3, 3 + 2
        nodes = [(n + 1, 4, 0, 0), (n + 2, 2, 9, 0), (n + 3, 0, 0, 0), (n + 4, 4, 0, 0), (n + 5, 2, 11, 0), (n + 6, 2, 1, 0)]
        edges = [(rack0, n + 1, 0, TREE), (n + 1, n + 2, 0, TREE)] + chain(parents, rack0)
        edges += [(2, n + 3, 0, TREE), (n + 3, n + 4, 0, TREE), (n + 4, n + 5, 0, TREE)]
        edges += [(mach0, n + 6, 0, TREE)] + chain(parents, mach0)[:1]   # (rack 0 → machine 0; X → rack 0 is listed above)
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert ref.S[2] == 21 and ref.S[rack0] == 10


@pytest.mark.parametrize("state", ["fresh", "pinned", "preemptive", "warm"])
def test_toy(state):
    parents = tree_parents(TOY.ntype, dict(TOY.arcs))
    with open_ctx(state) as ctx:
        pre = bring(ctx, TOY, state)
        nodes = [(20, 4, 0, 0), (21, 2, 2, 7), (22, 2, 1, 0)]
        edges = [(3, 20, 5, TREE), (20, 21, 6, TREE), (5, 22, 8, TREE)] + chain(parents, 5, {(3, 5): 9, (2, 3): 10})
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert ref.S == {21: 2, 22: 1, 20: 2, 5: 1, 3: 3, 2: 3}
        if state == "fresh":                                       # the literals of the CPU suite's table
            assert after.table[(2, 3)] == (0, 7, 0, 0) and after.table[(3, 5)] == (0, 3, 0, 0)
        if state in ("pinned", "warm"):                            # M1 ran two tasks on two slots: its arc had left
            assert after.table[(3, 5)] == (0, 1, 9, 0)


@pytest.mark.parametrize("state", ["fresh", "preemptive"])
def test_a_machine_under_a_rack_that_a_removal_emptied(state):
    """The capacity rule takes a type-0 head for a resource only while slots lie beneath it: when a
    rack's last machine leaves, the arc into the rack keeps the capacity it had (no flow can use
    it), and the machine that joins later raises that value instead of starting from 0. The
    refresh sets it: the recipe of include/ksmcmf.h (ks_add_resources) that the round test
    (tests/test_gpu_rounds.py) showed to be needed."""
    spec = Cluster(2, 1, 3, [1, 1] + [None] * 2)
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        mach, pu = spec.M0, spec.P0
        removed, _, _ = ctx.remove_resources([mach], resource_caps=True, preemptive=pre)
        assert removed.tolist() == [mach, pu]
        assert Snapshot(ctx).table[(spec.X, spec.R0)] == (0, 3, 0, 0)   # kept, with nothing beneath it
        nodes = [(mach, 4, 0, 0), (pu, 2, 2, 0)]
        edges = [(spec.R0, mach, 0, TREE), (mach, pu, 0, TREE), (spec.X, spec.R0, 0, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state, solve=False, full_chain=False)
        assert after.table[(spec.X, spec.R0)] == (0, 5, 0, 0)           # raised from the stale 3
        assert refresh(ctx, pre) == 1
        assert Snapshot(ctx).table[(spec.X, spec.R0)] == (0, 2, 0, 0)
        resolve_and_check(ctx)


# ------------------------------------------------------------------ id reuse ---
@pytest.mark.parametrize("state", ["fresh", "pinned", "preemptive"])
def test_ids_freed_by_remove_resources_are_reused(state):
    """A machine leaves through ks_remove_resources and joins again under its old ids: every
    resource arc is as it was; a machine that joins runs nothing, so it comes back empty. (Three
    machines to a rack and two free tasks: no machine beside the one that leaves can be full. A
    rack of type 0 whose machines are all full is no resource to the capacity rule, and the arc
    into it keeps the capacity it had.)"""
    spec = Cluster(2, 3, 3, [0, 0, 0, 1] + [None] * 2)
    parents = tree_parents(spec.ntype, dict(spec.arcs))
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        mach, pu = spec.M0 + 5, spec.P0 + 5
        before = Snapshot(ctx)
        ran = sum(1 for (s, d), a in before.table.items() if d == pu and a[3] == 1)
        removed, evicted, _ = ctx.remove_resources([mach, pu], resource_caps=True, preemptive=pre)
        assert removed.tolist() == [mach, pu] and len(evicted) == ran
        if ran and not pre:                                        # a pinned task has no arc but the running one:
            ctx.complete_tasks(evicted["task"].tolist(), resource_caps=False, unsched_ids=[spec.U])   # evicted, it leaves
            before = Snapshot(ctx)
        nodes = [(pu, 2, 3, 0), (mach, 4, 0, 0)]
        edges = [(mach, pu, 0, TREE)] + chain(parents, mach)
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        res = lambda t: {k: a for k, a in t.items() if before.ntype[k[0] - 1] != 1}
        if pre or not ran:                                         # the capacities are the slots: exactly as before
            assert res(after.table) == res(before.table)
        assert after.table[(spec.R0 + 1, mach)] == after.table[(mach, pu)] == (0, 3, 0, 0)
        assert after.alive == before.alive


@TWO_STATES
def test_ids_beyond_the_node_store_take_the_rebuild_path(state):
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        ctx.solve()
        r0 = ctx.store_stats()["rebuilds"]
        far = 5000                                                 # the node store holds 1,024 slots here
        nodes = [(far + 7, 2, 2, 0), (far, 4, 0, 0)]
        edges = [(far, far + 7, 0, TREE), (spec.R0 + 1, far, 0, TREE), (spec.X, spec.R0 + 1, 0, TREE)]
        ref, after, r = grow_and_check(ctx, nodes, edges, pre)
        assert ctx.store_stats()["rebuilds"] >= r0 + 1              # (by the refresh or by the solve, whichever came first)
        assert {far, far + 7} <= after.alive and not (set(range(far + 1, far + 7)) & after.alive)


# ---------------------------------------------------------------- wave edges ---
@TWO_STATES
@pytest.mark.parametrize("k", [63, 64, 65])
def test_pus_of_one_machine_fill_a_wave(state, k):
    """k new PUs under one new machine: their walks meet on the machine's, the rack's and the
    root's word, one wave exactly (64) and one lane into the next (65). PU i has i % 3 + 1 slots."""
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        mach = n + 1
        nodes = [(mach, 4, 0, 0)] + [(n + 2 + i, 2, i % 3 + 1, 0) for i in range(k)]
        edges = [(mach, n + 2 + i, 0, TREE) for i in range(k)] + [(spec.R0, mach, 0, TREE), (spec.X, spec.R0, 0, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        total = sum(i % 3 + 1 for i in range(k))
        assert after.table[(spec.R0, mach)] == (0, total, 0, 0) and ref.S[spec.X] == total


@TWO_STATES
def test_pus_alternate_between_two_machines(state):
    """130 PUs, the even ones under one new machine, the odd ones under another, both under one
    new rack: two distinct words per wave at the first step, one from the second on."""
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        rack, a, b = n + 1, n + 2, n + 3
        pus = [n + 4 + i for i in range(130)]
        nodes = [(rack, 0, 0, 0), (a, 4, 0, 0)] + [(p, 2, 1 + i % 2, 0) for i, p in enumerate(pus)] + [(b, 4, 0, 0)]
        edges = [((a, b)[i % 2], p, 0, TREE) for i, p in enumerate(pus)]
        edges += [(rack, a, 0, TREE), (rack, b, 0, TREE), (spec.X, rack, 0, TREE)]
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert after.table[(rack, a)][1] == 65 and after.table[(rack, b)][1] == 130 and after.table[(spec.X, rack)][1] == 195


@TWO_STATES
def test_machines_of_one_pu_under_one_rack(state):
    """65 machines of one PU under an existing rack: the lanes part at the first step (65 words)
    and meet at the second."""
    spec = grid()
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        n = top(ctx)
        held = Snapshot(ctx).table.get((spec.X, spec.R0 + 1), (0, 0, 0, 0))
        nodes, edges = [], []
        for i in range(65):
            m, p = n + 1 + 2 * i, n + 2 + 2 * i
            nodes += [(m, 4, 0, 0), (p, 2, 2, 0)]
            edges += [(spec.R0 + 1, m, 0, TREE), (m, p, 0, TREE)]
        edges.append((spec.X, spec.R0 + 1, 0, TREE))
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre, state)
        assert after.table[(spec.X, spec.R0 + 1)][1] == held[1] + 130 and ref.stats["arcs_added"] >= 130


# --------------------------------------------------------------------- depths ---
def tower(spec, first, depth):
    """A PU with depth tree edges above it: depth − 1 new intermediate nodes, the top one under X."""
    ids = list(range(first, first + depth))
    nodes = [(ids[0], 2, 2, 0)] + [(i, 5, 0, 0) for i in ids[1:]]
    edges = [(ids[k + 1], ids[k], 0, TREE) for k in range(depth - 1)] + [(spec.X, ids[-1], 0, TREE)]
    return nodes, edges


@pytest.mark.parametrize("depth", [1, 6, 32])
def test_legal_depths(depth):
    spec = grid()
    with open_ctx("fresh") as ctx:
        pre = bring(ctx, spec, "fresh")
        n = top(ctx)
        nodes, edges = tower(spec, n + 1, depth)
        ref, after, _ = grow_and_check(ctx, nodes, edges, pre)
        assert ref.stats["arcs_added"] == depth and after.table[(spec.X, n + depth)] == (0, 2, 0, 0)


# ------------------------------------------------- a new PU receives the tasks ---
@pytest.mark.parametrize("state", ["pinned", "preemptive"])
def test_a_new_pu_receives_tasks_when_capacity_is_short(state):
    """Four slots, seven tasks: three wait. A machine of two slots joins: two of them are placed
    on it at the next solve (after a pinned commit every arc on the way had left the store)."""
    spec = Cluster(2, 2, 1, [None] * 7)
    parents = tree_parents(spec.ntype, dict(spec.arcs))
    with open_ctx(state) as ctx:
        pre = bring(ctx, spec, state)
        if state == "pinned":
            assert (spec.X, spec.R0) not in Snapshot(ctx).table
        n = top(ctx)
        nodes = [(n + 1, 4, 0, 0), (n + 2, 2, 2, 0)]
        edges = [(spec.R0, n + 1, 0, TREE), (n + 1, n + 2, 0, TREE)] + chain(parents, spec.R0)
        grow_and_check(ctx, nodes, edges, pre)
        assert flow_into_sink(ctx, n + 2) == 2


# -------------------------------------------------------------------- refusals ---
def raw_call(ctx, nodes, edges, flags=0):
    nd = np.zeros(max(len(nodes), 1), native.RES_NODE_DT)
    for i, x in enumerate(nodes):
        nd[i] = tuple(x)
    ar = np.zeros(max(len(edges), 1), native.RES_ARC_DT)
    for j, x in enumerate(edges):
        ar[j] = tuple(x)
    st = native.KsGrowStats()
    rc = ctx._L.ks_add_resources(ctx._h, flags, nd.ctypes.data, len(nodes), ar.ctypes.data, len(edges), C.byref(st))
    return rc, ctx._L.ks_last_error(ctx._h).decode(), st.as_dict()


@pytest.mark.parametrize("solved", [False, True], ids=["fresh", "solved"])
def test_refusals_change_nothing(solved):
    spec = grid()
    X, R0, M0, P0 = spec.X, spec.R0, spec.M0, spec.P0
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(spec.bindings)
        dead = spec.T0 + 8
        ctx.complete_tasks([dead], resource_caps=False)
        task = spec.T0
        if solved:
            ctx.solve()
            d0 = ctx.scheduling_deltas(commit=False)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        tasks0 = live_tasks(before)
        b0 = ctx.bindings(tasks0).tolist()
        n = max(top(ctx), dead)                                      # (the dead id stays dead in every call below)
        a, b, c = n + 1, n + 2, n + 3

        def refused(code, names, nodes, edges, **kw):
            rc, msg, st = raw_call(ctx, nodes, edges, **kw)
            assert rc == code, (rc, msg)
            for x in names:
                assert str(x) in msg, msg
            assert not any(st.values())
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive and (now.nodes == before.nodes).all()
            assert ctx.store_stats() == s0
            assert ctx.bindings(tasks0).tolist() == b0
            if solved:                                               # the valid solution stands
                assert (ctx.scheduling_deltas(commit=False) == d0).all()

        mach, pu = (a, 4, 0, 0), (b, 2, 2, 0)
        ok = (R0, a, 0, TREE)
        refused(INVALID, [f"node {M0} "], [mach, (M0, 4, 0, 0), (0, 4, 0, 0)], [])          # a live id
        refused(INVALID, [f"node {task} "], [mach, (task, 4, 0, 0)], [])                    # a live task
        refused(INVALID, [f"node {a} "], [mach, pu, mach], [])                              # an id listed twice
        refused(RANGE, ["node id 0 "], [mach, (0, 4, 0, 0)], [])
        refused(RANGE, [1 << 30], [mach, (1 << 30, 4, 0, 0)], [])
        for ty in (1, 3, 6, -1):                                                            # a task, a sink, unknown types
            refused(INVALID, [f"node {b} ", "type"], [mach, (b, ty, 0, 0), (0, 9, 0, 0)], [])
        refused(INVALID, [f"node {b} ", "slots"], [mach, (b, 2, 0, 0)], [])                 # a PU without slots
        refused(INVALID, [f"node {b} "], [mach, (b, 4, 1, 0)], [])                          # a machine with slots
        refused(INVALID, [f"node {b} "], [mach, (b, 0, 0, 5)], [])                          # a rack with a sink cost
        refused(RANGE, [f"node {b}"], [mach, (b, 2, (1 << 53) + 1, 0)], [])
        refused(RANGE, [f"node {b}"], [mach, (b, 2, 1, (1 << 40) + 1)], [])
        refused(RANGE, [f"node {b}"], [mach, (b, 2, 1, -(1 << 40) - 1)], [])
        refused(RANGE, [f"node {c}", "summed"], [mach, (b, 2, 1 << 53, 0), (c, 2, 1, 0)], [])
        for p in (0, dead, task, 1, P0, b, n + 500, 10 ** 7):        # 0, dead, a task, the sink, a PU (live, new), beyond
            refused(INVALID, [f"edge {p} -> {a}", f"parent {p} "], [mach, pu], [ok, (p, a, 0, TREE), (0, 0, 0, 9)])
        for ch in (0, dead, task, 1, n + 500, 10 ** 7):
            refused(INVALID, [f"edge {a} -> {ch}", f"child {ch} "], [mach, pu], [ok, (a, ch, 1 << 41, 9)])   # before the cost
        refused(INVALID, [f"edge {a} -> {a}"], [mach, pu], [ok, (a, a, 0, TREE)])
        refused(INVALID, [f"edge {a} -> {b}", "kind 2"], [mach, pu], [ok, (a, b, 0, 2), (0, 0, 0, 0)])
        refused(INVALID, [f"edge {a} -> {b}", "kind -1"], [mach, pu], [ok, (a, b, 1 << 41, -1)])               # before the cost
        refused(INVALID, [f"edge {a} -> {M0}", "does not move"], [mach, pu], [ok, (a, M0, 0, TREE)])
        refused(RANGE, [f"edge {a} -> {b}", "cost"], [mach, pu], [ok, (a, b, (1 << 40) + 1, TREE)])
        refused(RANGE, [f"edge {a} -> {b}", "cost"], [mach, pu], [ok, (a, b, -(1 << 40) - 1, EXTRA)])
        refused(INVALID, [f"edge {R0} -> {a}", "twice"], [mach, pu], [ok, (a, b, 0, TREE), (R0, a, 0, EXTRA), (0, 0, 0, 0)])
        refused(INVALID, [f"edge {R0} -> {a}", "twice"], [mach, pu], [ok, (a, b, 0, TREE), ok])                # (before the parent)
        refused(INVALID, [f"child {a} ", "one parent"], [mach, pu], [ok, (a, b, 0, TREE), (R0 + 1, a, 0, TREE)])
        refused(INVALID, [f"child {M0} ", "one parent"], [mach, pu], [(R0, M0, 0, TREE), ok, (X, M0, 0, TREE)])
        # the first offending edge in input order wins over a later one of a lower class
        refused(RANGE, [f"edge {a} -> {b}", "cost"], [mach, pu], [ok, (a, b, 1 << 41, TREE), (0, a, 0, TREE)])
        # a cycle among new nodes: the first PU beneath it is named; a PU elsewhere is not
        refused(INVALID, [f"PU {c}:", "32"], [mach, (n + 4, 2, 1, 0), (b, 4, 0, 0), (c, 2, 1, 0), (n + 5, 2, 1, 0)],
                [(a, b, 0, TREE), (b, a, 0, TREE), (R0, n + 4, 0, TREE), (a, c, 0, TREE), (b, n + 5, 0, TREE)])
        # a cycle of chain edges between live nodes
        refused(INVALID, [f"PU {b}:"], [pu], [(M0, b, 0, TREE), (R0, M0, 0, TREE), (M0 + 1, R0, 0, TREE), (M0, M0 + 1, 0, TREE)])
        nodes, edges = tower(spec, n + 1, 33)                        # 33 tree edges above the PU
        refused(INVALID, [f"PU {n + 1}:", "32"], nodes, edges)
        refused(INVALID, ["flag"], [mach], [], flags=1)
        # the limits themselves are accepted
        rc, msg, st = raw_call(ctx, [mach, (b, 2, 1 << 40, -(1 << 40))], [ok, (a, b, 1 << 40, TREE)])
        assert rc == native.KS_OK, msg
        assert st == dict(nodes=2, pus=1, slots=1 << 40, sink_arcs=1, arcs_added=2, cap_updates=0, arcs_skipped=0, records=5)
        assert Snapshot(ctx).table[(a, b)] == (0, 1 << 40, 1 << 40, 0)
        # a raised capacity beyond 2^53: R0 → a holds 2^40 now
        rec = np.zeros(1, native.DELTA_DT)
        rec[0]["kind"], rec[0]["src"], rec[0]["dst"], rec[0]["cap"] = native.KS_ADD_ARC, R0, a, 1 << 53
        ctx.apply_deltas(rec)
        before, s0 = Snapshot(ctx), ctx.store_stats()
        tasks0 = live_tasks(before)
        b0 = ctx.bindings(tasks0).tolist()
        solved = False
        refused(RANGE, [f"edge {R0} -> {a}", "capacity"], [(c, 2, 1, 0)], [(a, c, 0, TREE), (R0, a, 0, TREE)])


def test_two_sinks_refuse_a_pu():
    spec = grid()
    n0 = len(spec.ntype)
    two = type(TOY)(list(spec.ntype) + [3], list(spec.supply) + [0], spec.arcs, spec.bindings)
    with native.Context(0, auto_sink=0) as ctx:
        ctx.load_graph(two.graph(running=True))
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        rc, msg, _ = raw_call(ctx, [(n0 + 2, 4, 0, 0), (n0 + 3, 2, 1, 0)], [(spec.R0, n0 + 2, 0, TREE)])
        assert rc == INVALID and "one sink" in msg
        now = Snapshot(ctx)
        assert now.table == before.table and now.alive == before.alive and ctx.store_stats() == s0
        rc, msg, st = raw_call(ctx, [(n0 + 2, 4, 0, 0)], [(spec.R0, n0 + 2, 0, TREE)])   # no PU: legal
        assert rc == native.KS_OK and st["records"] == 1 and n0 + 2 in Snapshot(ctx).alive


@EVERY_STATE
def test_nothing_and_chain_edges_alone_keep_the_solution(state):
    spec = grid()
    with open_ctx(state) as ctx:
        bring(ctx, spec, state)
        ctx.solve()
        mapping = ctx.task_mapping()
        s0 = ctx.store_stats()
        table = Snapshot(ctx).table
        for edges in ([], [(spec.X, spec.R0, 0, TREE), (spec.R0, spec.M0, 0, TREE), (spec.R0, spec.M0 + 1, 0, EXTRA)]):
            stats = ctx.add_resources([], edges)
            assert stats["records"] == 0 and stats["arcs_skipped"] == len(edges)
            assert ctx.task_mapping() == mapping                    # the mapping is still served
            assert ctx.store_stats() == s0 and Snapshot(ctx).table == table
