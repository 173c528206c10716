"""The cell solver (ks_cell.hip: a whole solve in one 1024-thread workgroup) on the
edges of its own layout: its seven node classes by segment capacity (≤ 4, 8, 16,
32, 64, 512 positions, and more), the partial last item of every class dealt from
one counter, empty classes, the second round of a wave's (256 positions) and of
the workgroup's (4,096) walk, the parity of the LDS carve and of the frontier
bitmaps, the two limits (2^18 positions, the LDS's 13,1xx nodes), ε off the powers
of two (floordiv in relax_q), a node that changes class across a rebuild, and a
batch's per-cell offsets.

A cell that does not converge is re-solved on the multi-kernel engine and the
solve still returns KS_OK with solver == 1: only ks_result.cell_fallbacks tells.
So every case here asserts the path that ran (solver), cell_fallbacks == 0 and
recoveries == 0 next to the oracle's cost and flow value (integer equality), the
oracle's verifier on the downloaded flows, and per PU as many mapped tasks as its
arc into the sink carries.

The shapes are those of tests/cell_shapes.py; their premises (degrees, nodes per
class, positions, feasibility; three references that agree) are asserted without
a device by tests/test_cell_shapes_cpu.py. After a load the residual CSR is tight,
so a node's class is that of its residual degree.

Seeded defects this file was run against (scratch builds, never committed; each only
skips work, none changes an address):
  - step counting class 3's items as n3 / p3 (the partial last item dropped): 28 of 39
    cases fail with KS_E_VERIFY or KS_E_INFEASIBLE, every partial-item case among them;
  - cell_class putting a capacity of 9 into class 1 (*_thr<8> ignores the 9th position):
    partial-2 and the repaired batch cell (cell_fallbacks == 1) and
    price_refine0-bound-all (KS_E_VERIFY) fail;
  - sweep_hub stopping after its first CT·UC positions: test_node_limit
    (cell_fallbacks == 1), the config-2 union (KS_E_INFEASIBLE) and stride-hub-6145
    (KS_E_INFEASIBLE) fail; a hub of 4,097 positions is still solved, since every phase's
    saturation pass reaches the one arc the sweep no longer sees."""
import numpy as np
import pytest

import cell_shapes as cs
from conftest import CELL_ANY
from ksched_amd import gen, native
from oracle import ko
from store_ref import StoreRef, delta, stream
from test_gpu_parity import check_mapping, flows_by_arc

pytestmark = pytest.mark.gpu

ADD_ARC, UPDATE_ARC = 2, 3
_REF: dict = {}


def oracle(name, g):
    """(cost, flow value) of g by the oracle's cost scaling, computed once per name."""
    if name not in _REF:
        st, cost, fv, _ = ko.cost_scaling(g)
        assert st == 0
        _REF[name] = (cost, fv)
    return _REF[name]


def check_solved(c, g, r, cost, fv, solver=1):
    """Every assertion of a lone-graph case on the result r of solving g on c."""
    assert r.raw["solver"] == solver
    assert r.raw["cell_fallbacks"] == 0, "a cell gave up and the engine re-solved it"
    assert r.raw["recoveries"] == 0, "the optimality certificate needed a repair"
    assert (r.cost, r.flow) == (cost, fv)
    fl = flows_by_arc(c, g)
    st, vcost, _ = ko.verify(g, fl)
    assert st == 0 and vcost == cost, "the oracle's verifier rejected the downloaded flows"
    mp = c.task_mapping()
    check_mapping(g, mp)
    load = np.bincount(np.fromiter(mp.values(), np.int64, len(mp)), minlength=g.n + 1)
    into_sink = (g.ntype[g.src - 1] == cs.PU_T) & (g.ntype[g.dst - 1] == cs.SINK_T)
    assert load[g.src[into_sink]].tolist() == fl[into_sink].tolist(), "mapped tasks per PU ≠ the flow PU → sink"
    assert int(load.sum()) == int(fl[into_sink].sum())


def solve_case(c, name, g, solver=1):
    cost, fv = oracle(name, g)
    c.load_graph(g)
    r = c.solve()
    check_solved(c, g, r, cost, fv, solver)
    return r


# ------------------------------------------------------------------ lone graphs ---
@pytest.mark.parametrize("case", cs.LONE, ids=lambda c: c.name)
def test_lone_graph(ctx, case):
    """Class bounds (PUs of d and d + 1 positions for d = 4, 8, 16, 32, 64, 512; tasks of
    4, 5, 8, 9; all of them in one graph), partial last items (classes 0–3 with 1, ipw − 1,
    ipw, ipw + 1, 2·ipw + 1 nodes: cell_shapes.PARTIAL says which case holds which count),
    empty classes (only 0 and 6; 4 and 5 empty; 6 empty), walk strides (class-5 nodes of
    256, 257, 512 positions; class-6 nodes of 513, 4,096, 4,097 and 6,145 — the last with
    half of its in-arcs in sweep_hub's second round of CT·UC; two and three class-6 nodes), N mod 32 ∈ {0, 1, 31} with N even and odd, and 256 / 257 tasks around BXC —
    which branch a global update took (bounded or not) cannot be observed, so the bounded
    cases assert the result only, like every other."""
    solve_case(ctx, case.name, cs.built(case))


def quincy_1k():
    return gen.quincy(1000, 100, 5, 10, 1)


@pytest.mark.parametrize("graph", ["bound-all", "quincy-1000x100"])
@pytest.mark.parametrize("opts", [{"alpha": 10}, {"alpha": 6}, {"price_refine": 0}],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_epsilon_not_a_power_of_two(opts, graph):
    """α = 10, α = 6 and price_refine = 0 take ε off the powers of two (ks_engine.hip,
    plan()), so relax_q's arc lengths come from floordiv, not from a shift."""
    g = cs.built(cs.by_name(graph)) if graph == "bound-all" else quincy_1k()
    with native.Context(0, cell_nodes=CELL_ANY, **opts) as c:
        solve_case(c, graph, g)


def test_position_limit():
    """2^18 positions (CELL_MAX_POS: reverse positions are 18 bits, relative to the cell)
    solve on the cell solver, two more are handed to the engine without a fallback, and
    the next small graph on the same context takes the cell solver again. 2^18 positions are
    131,072 arcs (dense(131_072): 511 × 256 complete plus 256 arcs into the sink); dense(65_536),
    2^17 positions, is solved on the way."""
    with native.Context(0, cell_nodes=CELL_ANY) as c:
        for name in ("positions-2^17", "positions-2^18", "positions-2^18-plus-2", "bound-pu-16"):
            case = cs.by_name(name)
            g = cs.built(case)
            assert name == "bound-pu-16" or cs.profile(g).positions == case.positions
            solve_case(c, name, g, solver=case.solver)


def test_node_limit():
    """13,000 nodes fit one workgroup's LDS, 13,300 do not (ks_cell.h gives the limit as
    13,1xx; cell_max_nodes is not exported, so only the two sides are asserted)."""
    with native.Context(0, cell_nodes=CELL_ANY) as c:
        for name in ("nodes-13000", "nodes-13300", "nodes-13000"):
            case = cs.by_name(name)
            solve_case(c, name, cs.built(case), solver=case.solver)


@pytest.mark.parametrize("warm", [0, 1], ids=["cold", "warm"])
def test_class_change_across_a_rebuild(warm):
    """A PU of exactly 8 positions (class 1, tight) gets a 9th arc: the residual CSR is
    rebuilt with slack and its segment holds 16 (class 2); seven more arcs fill it with
    no rebuild; the 17th position rebuilds again (32: class 3). ks_store_stats.rebuilds
    rises exactly where the restated segment rule (cell_shapes.Segments) says."""
    g = cs.built(cs.by_name("bound-all"))
    v, tasks = cs.rebuild_plan(g)
    seg = cs.Segments(g)
    ref = StoreRef.from_graph(g)
    with native.Context(0, cell_nodes=CELL_ANY, warm_start=warm) as c:
        r = solve_case(c, "bound-all", g)
        assert c.store_stats()["rebuilds"] == seg.solve() == 1
        classes = []
        for step, part in enumerate((tasks[:1], tasks[1:8], tasks[8:9])):
            recs = stream([delta(kind=ADD_ARC, src=t, dst=v, low=0, cap=1, cost=7) for t in part])
            for t in part:
                seg.add_arc(t, v)
            ref.apply(recs)
            c.apply_deltas(recs)
            h = ref.graph()
            cost, fv = oracle("rebuild-step-%d" % step, h)
            r = c.solve()
            check_solved(c, h, r, cost, fv)
            assert r.raw["warm_started"] == warm
            want = seg.solve()
            assert c.store_stats()["rebuilds"] == want, "step %d" % step
            assert r.raw["rebuilt"] == (1 if step != 1 else 0)
            classes.append((want, cs.cell_class(int(seg.cap[v - 1]))))
        assert classes == [(2, 2), (2, 2), (3, 3)]


# ----------------------------------------------------------------------- batches ---
def check_batch(b, graphs, names, res):
    r = res[0].raw
    assert (r["cells"], r["solver"], r["cell_fallbacks"], r["recoveries"]) == (len(graphs), 1, 0, 0)
    maxt = max(int(cs.task_ids(g).shape[0]) for g in graphs)
    pu, cost, flow = b.gather(maxt)
    for i, (g, name) in enumerate(zip(graphs, names)):
        assert (int(cost[i]), int(flow[i])) == oracle(name, g), name
        tasks = cs.task_ids(g)
        assert not pu[i, tasks.shape[0]:].any()
        # graph-local ids: the row holds this cell's PUs only, each within its capacity
        check_mapping(g, {int(t): int(p) for t, p in zip(tasks, pu[i]) if p})


def test_batch_mixed_profiles():
    """Five cells with different class profiles in one launch (x0, pb and cb[] per cell):
    one with classes 2 and 3 empty, one with three class-6 nodes; the largest has an odd
    node count (the LDS carve: bmp() at maxn + (maxn + 1) / 2 words) and sits in the middle."""
    graphs = [cs.built(cs.by_name(n)) for n in cs.BATCH_MIXED]
    b = native.Batch(devices=[0])
    try:
        b.load(graphs)
        check_batch(b, graphs, cs.BATCH_MIXED, b.solve())
    finally:
        b.close()


def test_batch_union_past_the_position_limit():
    """Three config-2-sized cells (106,250 positions each): the union passes 2^18
    positions, the third cell's positions all lie beyond it — reverse positions are
    relative to the cell, not to the union."""
    names = ["quincy-config2-s%d" % s for s in cs.BATCH_UNION_SEEDS]
    graphs = [gen.quincy(10_000, 1_000, 25, 100, s) for s in cs.BATCH_UNION_SEEDS]
    assert sum(2 * g.m for g in graphs) > cs.CELL_MAX_POS > max(2 * g.m for g in graphs)
    b = native.Batch(devices=[0])
    try:
        b.load(graphs)
        check_batch(b, graphs, names, b.solve())
    finally:
        b.close()


def test_batch_with_one_infeasible_cell():
    """One infeasible cell among four feasible ones: the solve fails with KS_E_INFEASIBLE
    (which cell the message names is not specified, so the text is not pinned); one
    ks_batch_apply_deltas record that widens U → sink makes it feasible, and the next
    solve gives every cell the oracle's result."""
    bad, (u, sink, cap) = cs.infeasible_cell()
    graphs = [bad if n is None else cs.built(cs.by_name(n)) for n in cs.BATCH_INFEASIBLE]
    k = cs.BATCH_INFEASIBLE.index(None)
    b = native.Batch(devices=[0])
    try:
        b.load(graphs)
        with pytest.raises(native.KsError) as ei:
            b.solve()
        assert ei.value.code == native.KS_E_INFEASIBLE
        fix = stream([delta(kind=UPDATE_ARC, src=u, dst=sink, low=0, cap=cap, cost=0)])
        b.apply_deltas([fix if i == k else None for i in range(len(graphs))])
        ref = StoreRef.from_graph(bad)
        ref.apply(fix)
        graphs[k] = ref.graph()
        names = ["infeasible-repaired" if n is None else n for n in cs.BATCH_INFEASIBLE]
        check_batch(b, graphs, names, b.solve())
    finally:
        b.close()
