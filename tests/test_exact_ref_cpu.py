"""The exact big-integer reference (tests/exact_ref.py) and the input families of
the GPU range tests (tests/graphs.py), checked on the CPU: hand-computed answers,
the C oracle wherever the values fit int64, networkx where it imports, and the
family counts a GPU test relies on."""
import os
import re

import numpy as np
import pytest

import exact_ref
import graphs
from graphs import graph_from_lists, scaled
from ksched_amd import gen
from oracle import ko

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ksched_amd", "csrc")


def quincy_negated(seed=5):
    """A Quincy cell with its task → unscheduled-aggregator costs negated (the GPU
    sign test's graph)."""
    g = gen.quincy(300, 30, 3, 6, seed)
    cost = g.cost.copy()
    cost[0:5 * 300:5] *= -1
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, g.cap, cost)


def all_negative():
    _, g, _ = next(x for x in graphs.signed_graphs() if x[2][0])
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, g.cap, -np.abs(g.cost) - 1)


def family_graphs():
    """(name, graph) of every family of tests/graphs.py, at values that fit int64."""
    out = [(f"signed{t}", g) for t, g, _ in graphs.signed_graphs()]
    out += [("negative_cycle", graphs.negative_cycle()), ("star", graphs.star()), ("star_small", graphs.star(5, 7)),
            ("sparse_ids", graphs.sparse_id_network()), ("sparse_ids_big", graphs.sparse_id_network(1 << 34)),
            ("long_chain", graphs.long_chain()), ("quincy_negated", quincy_negated()), ("all_negative", all_negative())]
    _, g, _ = next(x for x in graphs.signed_graphs() if x[2][0])
    out += [("signed_cost_2^33", scaled(g, cost_mul=1 << 33)), ("signed_cap_2^45", scaled(g, cap_mul=1 << 45))]
    return out


# ------------------------------------------------------------ by hand ---
def test_negative_cycle_by_hand():
    g = graphs.negative_cycle()
    feas, cost, flows = exact_ref.mcf(g)
    assert (feas, cost, flows) == (True, -10, [2, 2, 2])
    assert exact_ref.flow_value(g, flows) == 0
    assert exact_ref.check_flows(g, flows) == -10


def test_lower_bound_forces_a_positive_cycle():
    g = graph_from_lists([(1, 0, 0), (2, 0, 0), (3, 0, 0)],
                         [(1, 2, 1, 2, 4), (2, 3, 0, 5, 1), (3, 1, 0, 5, 2)])
    assert exact_ref.mcf(g) == (True, 7, [1, 1, 1])


def test_infeasible_by_hand():
    g = graph_from_lists([(1, 2, 0), (2, -2, 0)], [(1, 2, 0, 1, 3)])
    assert exact_ref.mcf(g) == (False, None, None)
    # an unbalanced supply, and a lower bound nothing can return
    assert not exact_ref.mcf(graph_from_lists([(1, 1, 0), (2, 0, 0)], [(1, 2, 0, 1, 0)]))[0]
    assert not exact_ref.mcf(graph_from_lists([(1, 0, 0), (2, 0, 0)], [(1, 2, 1, 1, 0)]))[0]


def test_two_routes_by_hand():
    """3 units over a cheap route of capacity 2 and a dear one; a negative arc into
    the source that nothing can use stays empty."""
    g = graph_from_lists([(1, 3, 0), (2, 0, 0), (3, -3, 0), (4, 0, 0)],
                         [(1, 2, 0, 2, 1), (2, 3, 0, 2, 1), (1, 3, 0, 5, 10), (4, 1, 0, 9, -7)])
    assert exact_ref.mcf(g) == (True, 2 * 2 + 10, [2, 2, 1, 0])


def test_beyond_int64_by_hand():
    """Supply 2^30 over two arcs of cost 2^35: 2^66 (each arc alone 2^65)."""
    g = graph_from_lists([(1, 1 << 30, 0), (2, 0, 0), (3, -(1 << 30), 0)],
                         [(1, 2, 0, 1 << 30, 1 << 35), (2, 3, 0, 1 << 31, 1 << 35)])
    feas, cost, flows = exact_ref.mcf(g)
    assert feas and cost == 1 << 66 and flows == [1 << 30, 1 << 30]
    assert exact_ref.check_flows(g, np.asarray(flows, np.int64)) == 1 << 66


def test_check_flows_rejects_bad_flows():
    g = graph_from_lists([(1, 3, 0), (2, 0, 0), (3, -3, 0)], [(1, 2, 0, 2, 1), (2, 3, 0, 2, 1), (1, 3, 1, 5, 10)])
    assert exact_ref.check_flows(g, [2, 2, 1]) == 14
    for bad in ([3, 3, 0], [2, 2, 0], [2, 1, 1], [3, 2, 0]):   # capacity, lower bound, conservation
        with pytest.raises(AssertionError):
            exact_ref.check_flows(g, bad)
    rec = np.zeros(2, [("src", "<u8"), ("dst", "<u8"), ("flow", "<i8")])   # ks_flow records: arcs without flow absent
    rec[0], rec[1] = (1, 3, 3), (2, 3, 0)
    assert exact_ref.check_flows(g, rec) == 30


# ------------------------------------------------ against other solvers ---
@pytest.mark.parametrize("name,g", family_graphs(), ids=[n for n, _ in family_graphs()])
def test_families_against_the_oracle(name, g):
    feas, cost, flows = exact_ref.mcf(g)
    st, c, fv, _ = ko.cost_scaling(g)
    if not feas:
        assert st != 0
        return
    assert abs(cost) < 1 << 62, "this family member is not scaled down into int64"
    assert (st, c, fv) == (0, cost, exact_ref.flow_value(g, flows))
    assert exact_ref.check_flows(g, flows) == cost
    if int(g.cost.min()) >= 0:
        assert ko.ssp(g)[:3] == (0, cost, fv)


def test_families_against_networkx():
    nx = pytest.importorskip("networkx")
    checked = 0
    for name, g in family_graphs():
        if g.low.any() or "2^" in name or name in ("sparse_ids_big", "long_chain", "star"):
            continue   # no lower bounds in networkx; its simplex is slow and inexact on huge weights
        G = nx.DiGraph()
        for v, s in enumerate(g.supply.tolist()):
            G.add_node(v + 1, demand=-s)
        for s, d, cap, c in zip(g.src.tolist(), g.dst.tolist(), g.cap.tolist(), g.cost.tolist()):
            G.add_edge(s, d, capacity=cap, weight=c)
        feas, cost, _ = exact_ref.mcf(g)
        try:
            c, _ = nx.network_simplex(G)
        except nx.NetworkXUnfeasible:
            assert not feas, name
        else:
            assert feas and c == cost, name
        checked += 1
    assert checked >= 12


# ------------------------------------------------------------ families ---
def test_signed_family_counts():
    fam = graphs.signed_graphs()
    feas = [x for x in fam if x[2][0]]
    assert len(feas) == graphs.FAMILY_FEASIBLE == 24 and len(fam) - len(feas) == graphs.FAMILY_INFEASIBLE == 6
    assert [t for t, _, _ in fam] == sorted(t for t, _, _ in fam)
    assert any(int(g.cost.min()) < 0 for _, g, _ in fam)
    assert sum(1 for _, g, r in feas if not g.low.any()) >= 8 and sum(1 for _, g, r in feas if g.low.any()) >= 4
    # negative cycles do occur: some optimum is below what the same graph costs with its negative arcs emptied
    assert any(r[1] < 0 for _, _, r in feas)
    # deterministic by seed
    again = graphs.select_family(graphs.signed_candidates(4242, 400))
    assert [(t, r[1]) for t, _, r in again] == [(t, r[1]) for t, _, r in fam]


def test_random_graphs_share_of_feasible():
    """What the selection is for: about half of the raw stream is infeasible."""
    for seed, count, want in ((12345, 40, 23), (7, 60, 22)):
        assert sum(exact_ref.mcf(g)[0] for _, g in graphs.random_graphs(seed, count)) == want


@pytest.mark.parametrize("cost_mul,cap_mul", [(1 << 33, 1), (1, 1 << 48), (1 << 33, 1 << 30)])
def test_scaling_scales_the_optimum(cost_mul, cap_mul):
    for _, g, (feas, cost, flows) in graphs.signed_graphs()[:8]:
        if not feas:
            continue
        f2, c2, fl2 = exact_ref.mcf(scaled(g, cost_mul, cap_mul))
        assert f2 and c2 == cost * cost_mul * cap_mul
        assert exact_ref.check_flows(scaled(g, cost_mul, cap_mul), fl2) == c2


def test_hand_made_networks():
    g = graphs.star()
    assert g.n == 202 and int(g.cap.max()) == graphs.CELL_MAX_CAP
    assert 200 * graphs.CELL_MAX_CAP > 1 << 31       # the admissible capacities of the centre leave int32
    assert exact_ref.mcf(g)[:2] == (True, 200 * graphs.CELL_MAX_CAP)
    g = graphs.sparse_id_network(1 << 20)
    assert g.n == graphs.SPARSE_TOP and len(set(g.src.tolist()) | set(g.dst.tolist())) == 12
    feas, cost, flows = exact_ref.mcf(g)
    assert feas and int(g.cost.max()) == 1 << 20
    assert flows[g.cost.tolist().index(1 << 20)] == 6     # the dearest arc carries flow
    assert cost == exact_ref.mcf(graphs.sparse_id_network(16))[1] << 16
    g = graphs.long_chain()
    mult = g.n + 1
    assert (1 << 37) * mult > graphs.LEN_CAP > graphs.FS_DMAX
    assert exact_ref.mcf(g) == (True, 3 * 7 * (1 << 37) + 2 * (1 << 40), [3] * 7 + [2])


def test_range_constants_match_the_headers():
    """graphs.py restates the library's limits; this reads them out of the sources."""
    def const(fname, name):
        text = open(os.path.join(CSRC, fname)).read()
        m = re.search(r"constexpr long long " + name + r" = ([^;]+);", text)
        assert m, f"{name} not found in {fname}"
        expr = m.group(1).replace("LL", "")
        assert re.fullmatch(r"[0-9a-fx()<\-+ ]+", expr), expr
        return eval(expr)   # noqa: S307 (digits, shifts and parentheses only)
    assert const("ks_cell.h", "CELL_MAX_CAP") == graphs.CELL_MAX_CAP
    assert const("ks_cell.h", "CELL_MAX_COST") == graphs.CELL_MAX_COST
    assert const("ks_pos.h", "CPOS_MAX") == graphs.CPOS_MAX
    assert const("ks_engine_impl.h", "FS_DMAX") == graphs.FS_DMAX
    host = open(os.path.join(CSRC, "ks_host.cpp")).read()
    assert "cap > (uint64_t(1) << 53) || cost > (int64_t(1) << 40) || cost < -(int64_t(1) << 40)" in host
    eng = open(os.path.join(CSRC, "ks_engine.hip")).read()
    assert "(double)maxc * (double)mult * 8.0 * (double)mult > 4.0e18" in eng
    assert const("ks_engine_impl.h", "LEN_CAP") == graphs.LEN_CAP
    build = open(os.path.join(CSRC, "ks_engine_build.hip")).read()
    assert "s.mult = ncap + 1;" in build
    assert graphs.solve_range_maxc(4001) == 31234380857
    c = graphs.solve_range_maxc(4001)
    assert c * 4001 * 4001 * 8 <= 4 * 10 ** 18 < (c + 1) * 4001 * 4001 * 8
