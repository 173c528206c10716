"""Both solvers at the edges of the integer range the library declares
(include/ksmcmf.h, "Value ranges"): the sign of the costs, costs and capacities on
both sides of every guard (the cell solver's compact record, the engine's 16-byte
positions, the ABI limits, the solve-time scaled-price limit) and totals at and
beyond int64.

The referee is tests/exact_ref.py (Python integers): the C oracle is int64 too
and its SSP refuses negative costs. Every comparison is an integer equality. A
boundary test names the path it requires (ks_result.solver: 1 cell solver, 0
engine; ks_result.compact: 1 when the engine read its 16-byte positions) and
fails if another one ran. tests/test_exact_ref_cpu.py checks the reference, the
families (24 feasible and 6 infeasible members) and the constants used here."""
import numpy as np
import pytest

import exact_ref
import graphs
from conftest import CELL_ANY
from graphs import (ABI_MAX_CAP, ABI_MAX_COST, CELL_MAX_CAP, CELL_MAX_COST, CPOS_MAX, graph_from_lists, same_graph,
                    scaled)
from ksched_amd import batch, gen, native
from test_gpu_parity import check_mapping

pytestmark = pytest.mark.gpu

CELL, ENGINE = 1, 0


# ----------------------------------------------------------------- helpers ---
def on_engine(c):
    return c.opts.cell_nodes < 0


def require_path(r, solver, compact, what):
    got = (r.raw["solver"], r.raw["compact"])
    msg = f"{what}: required solver={solver} compact={compact}, got solver={got[0]} compact={got[1]}"
    assert solver is None or got[0] == solver, msg
    assert compact is None or got[1] == compact, msg


def check_solution(c, g, r, ref, solver=None, compact=None, what=""):
    """r (the solve of g on c) equals the exact optimum ref, the downloaded flows are
    feasible and cost the same, no certificate repair ran, and the required path ran."""
    feas, cost, flows = ref
    assert feas, f"{what}: the reference calls this graph infeasible"
    assert (r.cost, r.flow) == (cost, exact_ref.flow_value(g, flows)), what
    assert exact_ref.check_flows(g, c.flows()) == cost, what
    assert r.raw["recoveries"] == 0, f"{what}: the optimality certificate needed a repair"
    require_path(r, solver, compact, what)
    return r


def solve_exact(c, g, ref=None, solver=None, compact=None, what="", load=True):
    ref = ref or exact_ref.mcf(g)
    if load:
        c.load_graph(g)
    if not ref[0]:
        with pytest.raises(native.KsError) as ei:
            c.solve()
        assert ei.value.code == native.KS_E_INFEASIBLE, what
        return None
    return check_solution(c, g, c.solve(), ref, solver, compact, what)


def default_path(c, fits_cell=True, fits_compact=True):
    """(solver, compact) a small graph must take on context c."""
    if not on_engine(c) and fits_cell:
        return CELL, 0
    return ENGINE, 1 if fits_compact and c.opts.compact_pos >= 0 else 0


def with_costs(g, cost):
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, g.cap, np.asarray(cost, np.int64), g.atype)


def max_cost_at(g, top):
    """g's costs multiplied by the largest k with k · max|cost| ≤ top, the arcs of the
    largest |cost| then moved to exactly ±top."""
    cost = g.cost.tolist()
    maxc = max(abs(x) for x in cost)
    k = top // maxc
    assert k >= 1
    return with_costs(g, [(top if x > 0 else -top) if abs(x) == maxc else x * k for x in cost])


def max_cap_at(g, top):
    """g's capacities, lower bounds and supplies multiplied by the largest k with
    k · max cap ≤ top, the arcs of the largest capacity then widened to exactly top."""
    k = top // int(g.cap.max())
    assert k >= 1
    h = scaled(g, cap_mul=k)
    cap = [top if x == int(h.cap.max()) else x for x in h.cap.tolist()]
    return gen.Graph(h.ntype, h.supply, h.src, h.dst, h.low, np.asarray(cap, np.int64), h.cost, h.atype)


def snapshot(c):
    """The device-resident graph (ks_get_graph), sorted: what a refused call must leave as it was."""
    nodes, arcs = c.graph()
    return (sorted(zip(nodes["id"].tolist(), nodes["excess"].tolist(), nodes["type"].tolist())),
            sorted(zip(*(arcs[k].tolist() for k in ("src", "dst", "low", "cap", "cost")))))


def holds(c, g):
    """The device-resident arcs are g's (ids, bounds and costs, arc by arc)."""
    assert snapshot(c)[1] == sorted(zip(*(a.tolist() for a in (g.src, g.dst, g.low, g.cap, g.cost))))


def delta(kind, **kw):
    d = np.zeros(1, native.DELTA_DT)
    d[0]["kind"] = kind
    for k, v in kw.items():
        d[0][k] = v
    return d


def update_costs(g, new_cost):
    """UPDATE_ARC records that turn g's costs into new_cost (arc by arc, where they differ)."""
    recs = [delta(native.KS_UPDATE_ARC, src=s, dst=d, low=lo, cap=cp, cost=nc, old_cost=oc)
            for s, d, lo, cp, oc, nc in zip(g.src.tolist(), g.dst.tolist(), g.low.tolist(), g.cap.tolist(),
                                            g.cost.tolist(), new_cost) if oc != nc]
    return np.concatenate(recs)


def signed_member(negative_top=False, lower_bounds=None):
    """A feasible member of the signed family (with its exact optimum); negative_top: its
    largest |cost| sits on a negative arc only."""
    for t, g, ref in graphs.signed_graphs():
        cost = g.cost.tolist()
        maxc = max(abs(x) for x in cost)
        if not ref[0] or g.m < 40 or (lower_bounds is not None and bool(g.low.any()) != lower_bounds):
            continue
        if negative_top and (maxc in cost or -maxc not in cost):
            continue
        return g, ref
    raise AssertionError("no such member")


def quincy_cell(seed=5):
    return gen.quincy(300, 30, 3, 6, seed)


def mult_of(c, g):
    """The cost multiplier of a fresh load of g: the node-slot count + 1
    (ks_engine_build.hip: mult = ncap + 1, no spare slots before the first delta)."""
    c.load_graph(g)
    return c.solve().raw["n_nodes"] + 1


# -------------------------------------------------------------------- a. sign ---
def test_signed_family(any_ctx):
    """Costs in [−100, 100): negative arcs and negative cycles, on both solvers; the
    infeasible members say so."""
    fam = graphs.signed_graphs()
    assert sum(1 for x in fam if x[2][0]) == 24 and len(fam) == 30
    for t, g, ref in fam:
        solve_exact(any_ctx, g, ref, *default_path(any_ctx), what=f"signed graph {t}")


def test_negative_cycle(any_ctx):
    """No supplies at all: the optimum is the cycle's −5 twice (flow value 0)."""
    g = graphs.negative_cycle()
    r = solve_exact(any_ctx, g, (True, -10, [2, 2, 2]), *default_path(any_ctx), what="negative 3-cycle")
    assert (r.cost, r.flow) == (-10, 0)


def test_every_cost_negative(any_ctx):
    g, _ = signed_member()
    solve_exact(any_ctx, with_costs(g, -np.abs(g.cost) - 1), None, *default_path(any_ctx), what="all costs negative")


def test_every_cost_zero(any_ctx):
    """max |cost| = 0 skips the range check and must still give a first ε."""
    g, _ = signed_member()
    r = solve_exact(any_ctx, with_costs(g, np.zeros(g.m)), None, *default_path(any_ctx), what="all costs zero")
    assert r.cost == 0 and r.flow > 0


def test_quincy_negated_unscheduled_costs(any_ctx):
    """A Quincy cell whose task → unscheduled-aggregator arcs pay instead of cost."""
    g = quincy_cell()
    cost = g.cost.copy()
    cost[0:5 * 300:5] *= -1
    g = with_costs(g, cost)
    solve_exact(any_ctx, g, None, *default_path(any_ctx), what="quincy, negated unscheduled costs")
    mp = any_ctx.task_mapping()
    check_mapping(g, mp)
    fl = exact_ref.per_arc(g, any_ctx.flows())
    assert len(mp) == sum(f for f, s in zip(fl, g.src.tolist()) if g.ntype[s - 1] == 2)   # tasks placed = units through PUs


# ------------------------------------------------------------- b. cost ladder ---
def ladder_graphs():
    g, _ = signed_member(negative_top=True)
    return [("quincy", quincy_cell()), ("signed", g)]


@pytest.mark.parametrize("name", ["quincy", "signed"])
def test_cost_at_the_cell_limit(ctx, name):
    """The largest |cost · mult| the cell solver's record holds, and one cost unit more:
    the cell solver must take the first, the engine the second."""
    g = dict(ladder_graphs())[name]
    mult = mult_of(ctx, g)
    top = CELL_MAX_COST // mult
    assert top * mult <= CELL_MAX_COST < (top + 1) * mult
    solve_exact(ctx, max_cost_at(g, top), None, CELL, 0, f"{name}, max |cost|·mult = {top * mult} = limit − "
                f"{CELL_MAX_COST - top * mult}")
    solve_exact(ctx, max_cost_at(g, top + 1), None, ENGINE, 0, f"{name}, max |cost|·mult = {(top + 1) * mult} > limit")


@pytest.mark.parametrize("name", ["quincy", "signed"])
def test_cost_at_the_compact_limit(ctx_engine, name):
    """The same pair on the engine: 16-byte positions up to CPOS_MAX, 32-byte ones beyond."""
    g = dict(ladder_graphs())[name]
    mult = mult_of(ctx_engine, g)
    top = CPOS_MAX // mult
    solve_exact(ctx_engine, max_cost_at(g, top), None, ENGINE, 1, f"{name}, max |cost|·mult = {top * mult} ≤ CPOS_MAX")
    solve_exact(ctx_engine, max_cost_at(g, top + 1), None, ENGINE, 0,
                f"{name}, max |cost|·mult = {(top + 1) * mult} > CPOS_MAX")


@pytest.mark.parametrize("name", ["quincy", "signed"])
def test_cost_ladder_to_the_abi_limit(any_ctx, name):
    """× 2^10 steps: the optimum scales with the costs, up to |cost| = 2^40 exactly."""
    g = dict(ladder_graphs())[name]
    base = exact_ref.mcf(g)
    mult = mult_of(any_ctx, g)
    maxc = int(np.abs(g.cost).max())
    for sh in (10, 20, 30):
        assert maxc << sh <= ABI_MAX_COST
        h = scaled(g, cost_mul=1 << sh)
        ref = exact_ref.mcf(h)
        assert ref[1] == base[1] << sh
        fits = (maxc << sh) * mult <= CELL_MAX_COST
        solve_exact(any_ctx, h, ref, *default_path(any_ctx, fits, fits), what=f"{name}, costs × 2^{sh}")
    solve_exact(any_ctx, max_cost_at(g, ABI_MAX_COST), None, ENGINE, 0, f"{name}, max |cost| = 2^40")


@pytest.mark.parametrize("bad", [ABI_MAX_COST + 1, -ABI_MAX_COST - 1])
def test_cost_beyond_the_abi_limit_is_refused(any_ctx, bad):
    """|cost| = 2^40 + 1 from ks_load_graph, an ADD_ARC and an UPDATE_ARC record:
    KS_E_RANGE, and the context keeps its graph and its optimum."""
    g, ref = signed_member()
    s, d = int(g.src[0]), int(g.dst[0])
    have = set(zip(g.src.tolist(), g.dst.tolist()))
    free = next((a, b) for a in range(1, g.n + 1) for b in range(1, g.n + 1) if a != b and (a, b) not in have)
    solve_exact(any_ctx, g, ref, what="before")
    holds(any_ctx, g)
    before = snapshot(any_ctx)
    cost = g.cost.copy()
    cost[0] = bad
    attempts = {
        "ks_load_graph": lambda: any_ctx.load_graph(with_costs(g, cost)),
        "ADD_ARC": lambda: any_ctx.apply_deltas(delta(native.KS_ADD_ARC, src=free[0], dst=free[1], cap=5, cost=bad)),
        "UPDATE_ARC": lambda: any_ctx.apply_deltas(delta(native.KS_UPDATE_ARC, src=s, dst=d, low=int(g.low[0]),
                                                         cap=int(g.cap[0]), cost=bad, old_cost=int(g.cost[0]))),
    }
    for what, attempt in attempts.items():
        with pytest.raises(native.KsError) as ei:
            attempt()
        assert ei.value.code == native.KS_E_RANGE, what
        assert snapshot(any_ctx) == before, f"the refused {what} changed the device-resident graph"
        solve_exact(any_ctx, g, ref, what=f"after the refused {what}", load=False)


@pytest.mark.parametrize("warm", [0, 1])
def test_solve_time_price_limit(warm):
    """ks_solve's own limit, max|cost| · mult² · 8 ≤ 4e18, on a 12-node network whose
    highest id is 4,000 (mult = 4,001): the largest admissible max|cost| solves exactly
    (the scaled prices come closest to int64 here), twice that is KS_E_RANGE from
    ks_solve, and an UPDATE_ARC that lowers the costs makes the context solve again."""
    with native.Context(0, cell_nodes=-1, warm_start=warm) as c:
        mult = mult_of(c, graphs.sparse_id_network())
        assert mult == graphs.SPARSE_TOP + 1
        maxc = graphs.solve_range_maxc(mult)
        assert 2 * maxc <= ABI_MAX_COST
        g = graphs.sparse_id_network(maxc)
        ref = exact_ref.mcf(g)
        solve_exact(c, g, ref, ENGINE, 0, f"max|cost| = {maxc}, the solve-time limit for mult {mult}")
        g2 = graphs.sparse_id_network(2 * maxc)
        c.load_graph(g2)
        with pytest.raises(native.KsError) as ei:
            c.solve()
        assert ei.value.code == native.KS_E_RANGE
        same_graph(c, g2)
        lowered = [min(x, maxc) for x in g2.cost.tolist()]
        c.apply_deltas(update_costs(g2, lowered))
        h = with_costs(g2, lowered)
        same_graph(c, h)
        solve_exact(c, h, None, ENGINE, 0, "after lowering the costs into range", load=False)
        solve_exact(c, h, None, ENGINE, 0, "solved once more", load=False)


def test_solve_time_price_limit_scales():
    """The optimum at the solve-time limit is the unit network's, scaled (pure scaling
    by maxc / 16 where 16 divides it)."""
    unit = exact_ref.mcf(graphs.sparse_id_network(16))
    with native.Context(0, cell_nodes=-1) as c:
        maxc = graphs.solve_range_maxc(mult_of(c, graphs.sparse_id_network()))
        top = maxc - maxc % 16
        g = graphs.sparse_id_network(top)
        ref = exact_ref.mcf(g)
        assert ref[1] == unit[1] * (top // 16)
        solve_exact(c, g, ref, ENGINE, 0, f"max|cost| = {top}")


@pytest.mark.parametrize("warm", [0, 1])
def test_costs_cross_the_cell_limit_and_return(warm):
    """Costs raised past what the cell solver's record holds send the solve to the
    engine; lowered again, the next solve is the cell solver's once more."""
    g = quincy_cell(9)
    with native.Context(0, cell_nodes=CELL_ANY, warm_start=warm) as c:
        mult = mult_of(c, g)
        r = solve_exact(c, g, None, CELL, 0, "round 0", load=False)
        assert r.raw["warm_started"] == warm
        big = CELL_MAX_COST // mult + 1
        raised = g.cost.tolist()
        for i in range(0, 5 * 40, 5):   # 40 tasks' arcs to their unscheduled aggregators
            raised[i] += big
        c.apply_deltas(update_costs(g, raised))
        h = with_costs(g, raised)
        r = solve_exact(c, h, None, ENGINE, 0, "round 1: costs past the cell limit", load=False)
        assert r.raw["warm_started"] == warm
        c.apply_deltas(update_costs(h, g.cost.tolist()))
        r = solve_exact(c, g, None, CELL, 0, "round 2: costs lowered again", load=False)
        assert r.raw["warm_started"] == warm
        same_graph(c, g)


def three_cells():
    """Three small cells; the middle one holds a cost the cell solver's record cannot."""
    cells = [quincy_cell(21), quincy_cell(22), quincy_cell(23)]
    cost = cells[1].cost.copy()
    cost[0:5 * 25:5] += 1 << 33
    cells[1] = with_costs(cells[1], cost)
    return cells, [exact_ref.mcf(g) for g in cells]


def test_solve_many_with_one_cell_out_of_range():
    cells, refs = three_cells()
    ctxs = [native.Context(0, cell_nodes=CELL_ANY) for _ in cells]
    try:
        for c, g in zip(ctxs, cells):
            c.load_graph(g)
        res = native.solve_many(ctxs, workers=3)
        for i, (c, g, r, ref) in enumerate(zip(ctxs, cells, res, refs)):
            check_solution(c, g, r, ref, ENGINE if i == 1 else CELL, 0, f"solve_many, cell {i}")
    finally:
        for c in ctxs:
            c.close()


def test_union_with_one_cell_out_of_range(ctx):
    cells, refs = three_cells()
    u, noff, _ = batch.union(cells)
    r = solve_exact(ctx, u, (True, sum(x[1] for x in refs), sum((x[2] for x in refs), [])), ENGINE, 0,
                    "union of three cells, one out of the cell solver's range")
    assert r.cost == sum(x[1] for x in refs)
    assert batch.split_costs(u, noff, ctx.flows()).tolist() == [x[1] for x in refs]


# ----------------------------------------------- c. capacity and supply ladder ---
def unit_cost_graph():
    """A signed-family member without lower bounds, its costs reduced to 0 / 1 so that
    totals fit whatever the capacities."""
    g, _ = signed_member(lower_bounds=False)
    return with_costs(g, np.abs(g.cost) & 1)


CAP_LADDER = [(CELL_MAX_CAP, True, True), (CELL_MAX_CAP + 1, False, True), (CPOS_MAX, False, True),
              (CPOS_MAX + 1, False, False), (1 << 45, False, False), (ABI_MAX_CAP, False, False)]


@pytest.mark.parametrize("top,fits_cell,fits_compact", CAP_LADDER, ids=[f"cap{t}" for t, _, _ in CAP_LADDER])
def test_capacity_ladder(any_ctx, top, fits_cell, fits_compact):
    """Capacities with supplies to match (the flow is that large), unit and zero costs."""
    g = unit_cost_graph()
    base = exact_ref.mcf(g)
    k = top // int(g.cap.max())
    ref = exact_ref.mcf(scaled(g, cap_mul=k))
    assert ref[1] == base[1] * k and exact_ref.flow_value(g, base[2]) * k > top // 20
    h = max_cap_at(g, top)
    assert int(h.cap.max()) == top
    solve_exact(any_ctx, h, None, *default_path(any_ctx, fits_cell, fits_compact), what=f"largest capacity {top}")


def test_capacity_beyond_the_abi_limit_is_refused(any_ctx):
    g = unit_cost_graph()
    ref = exact_ref.mcf(g)
    solve_exact(any_ctx, g, ref, what="before")
    holds(any_ctx, g)
    before = snapshot(any_ctx)
    cap = g.cap.copy()
    cap[0] = ABI_MAX_CAP + 1
    bad = gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, cap, g.cost)
    attempts = {
        "ks_load_graph": lambda: any_ctx.load_graph(bad),
        "UPDATE_ARC": lambda: any_ctx.apply_deltas(delta(native.KS_UPDATE_ARC, src=int(g.src[0]), dst=int(g.dst[0]),
                                                         cap=ABI_MAX_CAP + 1, cost=int(g.cost[0]),
                                                         old_cost=int(g.cost[0]))),
    }
    for what, attempt in attempts.items():
        with pytest.raises(native.KsError) as ei:
            attempt()
        assert ei.value.code == native.KS_E_RANGE, what
        assert snapshot(any_ctx) == before, f"the refused {what} changed the device-resident graph"
        solve_exact(any_ctx, g, ref, what=f"after the refused {what}", load=False)


def test_star_fills_the_lane_groups_int32_sum(ctx):
    """200 admissible arcs of capacity CELL_MAX_CAP out of one node, all filled: their
    capacities sum past 2^31 inside the cell solver."""
    g = graphs.star()
    r = solve_exact(ctx, g, None, CELL, 0, "star of 200 arcs at CELL_MAX_CAP")
    assert r.cost == 200 * CELL_MAX_CAP > 1 << 31


@pytest.mark.parametrize("compact_pos", [0, -1])
def test_reverse_residual_grows_to_the_compact_limit(compact_pos):
    """The pack kernel checks ranges before the phases only: a cheap route of capacity
    CPOS_MAX is saturated during the solve, so its reverse residuals grow to CPOS_MAX
    (with compact_pos = −1 the same solve on the 32-byte positions)."""
    g = graph_from_lists([(1, CPOS_MAX + 7, 0), (2, 0, 0), (3, -(CPOS_MAX + 7), 0), (4, 0, 0)],
                         [(1, 2, 0, CPOS_MAX, 1), (2, 3, 0, CPOS_MAX, -1), (1, 4, 0, 9, 5), (4, 3, 0, 9, 5),
                          (3, 2, 0, CPOS_MAX, 3)])
    with native.Context(0, cell_nodes=-1, compact_pos=compact_pos) as c:
        r = solve_exact(c, g, None, ENGINE, 1 if compact_pos == 0 else 0, f"compact_pos={compact_pos}")
        assert r.cost == 70 and r.flow == CPOS_MAX + 7


# ------------------------------------------------------------------ d. totals ---
def path_graph(supply, costs=(1 << 35, 0)):
    return graph_from_lists([(1, supply, 0), (2, 0, 0), (3, -supply, 0)],
                            [(1, 2, 0, supply, costs[0]), (2, 3, 0, supply, costs[1])])


def routes_graph(routes, supply, cost):
    """`routes` disjoint two-arc routes, each carrying `supply` units at `cost` a unit."""
    nodes, arcs = [], []
    for i in range(routes):
        a = 3 * i + 1
        nodes += [(a, supply, 0), (a + 1, 0, 0), (a + 2, -supply, 0)]
        arcs += [(a, a + 1, 0, supply, cost), (a + 1, a + 2, 0, supply, 0)]
    return graph_from_lists(nodes, arcs)


def beyond_int64():
    """(name, graph, exact total): totals the result's int64 cannot hold."""
    cyc = graph_from_lists([(1, 1 << 27, 0), (2, 0, 0), (3, -(1 << 27), 0), (4, 0, 0), (5, 0, 0)],
                           [(1, 2, 0, 1 << 27, 1 << 35), (2, 3, 0, 1 << 27, 0),
                            (3, 4, 0, 1 << 27, -(1 << 35)), (4, 5, 0, 1 << 27, 0), (5, 3, 0, 1 << 27, 0)])
    return [("one product 2^65", path_graph(1 << 30), 1 << 65),
            ("five routes of 2^61", routes_graph(5, 1 << 26, 1 << 35), 5 << 61),
            ("2^62 and -2^62: the sum is 0, the magnitudes 2^63", cyc, 0)]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_total_beyond_int64_is_refused(any_ctx, case):
    """total_cost is exact whenever Σ |flow · cost| < 2^63; otherwise ks_solve returns
    KS_E_RANGE with a message that names the total, never KS_OK with a wrapped number."""
    name, g, total = beyond_int64()[case]
    feas, cost, flows = exact_ref.mcf(g)
    assert feas and cost == total
    assert sum(abs(f * c) for f, c in zip(flows, g.cost.tolist())) >= 1 << 63
    any_ctx.load_graph(g)
    try:
        r = any_ctx.solve()
    except native.KsError as e:
        assert e.code == native.KS_E_RANGE, name
        assert "total cost" in str(e), name
    else:
        pytest.fail(f"{name}: KS_OK with total_cost {r.cost}, the exact total is {cost} (Σ |flow · cost| ≥ 2^63)")
    # the context stays usable
    solve_exact(any_ctx, path_graph(5, (7, 1)), (True, 40, [5, 5]), what="after the refused total")


def test_total_just_inside_int64(any_ctx):
    """Exact totals in (2^62, 2^63): 1.5 · 2^62 on one arc, and 2^63 − 2^35 over three."""
    g = path_graph(3 << 26)
    r = solve_exact(any_ctx, g, None, ENGINE, 0, "1.5 · 2^62")
    assert r.cost == 3 << 61 and 1 << 62 < r.cost < 1 << 63
    g = graph_from_lists([(1, (1 << 28) - 1, 0), (2, 0, 0), (3, 1 - (1 << 28), 0), (4, 0, 0)],
                         [(1, 2, 0, 1 << 28, 1 << 34), (2, 3, 0, 1 << 28, 1 << 34), (1, 4, 0, 1 << 28, 1 << 33),
                          (4, 3, 0, 1 << 28, 1 << 35)])
    r = solve_exact(any_ctx, g, None, ENGINE, 0, "2^63 − 2^35")
    assert r.cost == ((1 << 28) - 1) << 35 == (1 << 63) - (1 << 35)
    r = solve_exact(any_ctx, path_graph(3 << 26, (-(1 << 35), 0)), None, ENGINE, 0, "−1.5 · 2^62")
    assert r.cost == -(3 << 61)


def test_totals_per_cell(ctx):
    """The same two cases as parts of a union: batch.split_costs and the per-cell sums of
    ks_batch_gather (ks_engine_io.hip) are exact for a part just inside int64, and a
    part beyond it fails the union's solve with KS_E_RANGE."""
    small = [quincy_cell(31), quincy_cell(32)]
    inside = path_graph(3 << 26)
    cells = [small[0], inside, small[1]]
    refs = [exact_ref.mcf(g) for g in cells]
    assert refs[1][1] == 3 << 61
    u, noff, _ = batch.union(cells)
    r = solve_exact(ctx, u, (True, sum(x[1] for x in refs), sum((x[2] for x in refs), [])), ENGINE, 0, "union")
    assert batch.split_costs(u, noff, ctx.flows()).tolist() == [x[1] for x in refs]
    b = native.Batch(devices=[0])
    try:
        b.load(cells)
        res = b.solve()
        assert res[0].cost == sum(x[1] for x in refs) and res[0].raw["recoveries"] == 0
        _, cost, flow = b.gather(300)
        assert cost.tolist() == [x[1] for x in refs]
        assert flow.tolist() == [exact_ref.flow_value(g, x[2]) for g, x in zip(cells, refs)]
    finally:
        b.close()
    b = native.Batch(devices=[0])
    try:
        b.load([small[0], path_graph(1 << 30), small[1]])
        with pytest.raises(native.KsError) as ei:
            b.solve()
        assert ei.value.code == native.KS_E_RANGE and "total cost" in str(ei.value)
    finally:
        b.close()
    u2, _, _ = batch.union([small[0], path_graph(1 << 30), small[1]])
    ctx.load_graph(u2)
    with pytest.raises(native.KsError) as ei:
        ctx.solve()
    assert ei.value.code == native.KS_E_RANGE and "total cost" in str(ei.value)


# ---------------------------------------------------- the engine's long lengths ---
def test_lengths_beyond_the_clamps(any_ctx):
    """Arc lengths rc / ε beyond LEN_CAP and FS_DMAX in the ε = 1 phase."""
    g = graphs.long_chain()
    r = solve_exact(any_ctx, g, None, ENGINE, 0, "chain of 2^37 links")
    assert r.cost == 3 * 7 * (1 << 37) + 2 * (1 << 40)
