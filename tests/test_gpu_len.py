"""Arc lengths from the per-phase reciprocal (ks_len.h, Ctl::inv): the engine's
Bellman-Ford rounds (k_bf_round, all three modes), its forward search (k_fs_round)
and the applies' overflow limit (Ctl::lim) must leave every result what the division
gave — the oracle's cost and flow, no certificate repair, a valid mapping.

Every graph is solved on the engine (cell_nodes −1) under the default options, with
the refinement forced in the last phase (price_refine 2), without it (0) and with
unbounded updates (bf_bound −1). The shapes: two small Quincy graphs, one of 16,927
nodes (above the 14,336-node LDS search limit: k_bf_round<2> with the multi-launch
search), general digraphs with hubs, and one graph whose lengths leave the
multiply's range: 3,032 nodes, so mult = node capacity + 1 > 2^11, costs 1 and 2^30
mixed, so at ε = 1 an arc of cost 2^30 between nodes of close prices is
2^30 · mult > 2^41 units long and takes the division branch on the device (its
scaled costs do not fit the 16-byte positions either: the 32-byte records are read).
Its optimum comes from tests/exact_ref.py."""
import numpy as np
import pytest

import exact_ref
from graphs import random_hub_graphs
from ksched_amd import gen, native
from oracle import ko
from test_gpu_parity import check_mapping, solve_and_check

pytestmark = pytest.mark.gpu

QUINCY = [((600, 100, 5, 10), 1), ((600, 100, 5, 10), 2), ((2000, 200, 10, 20), 1), ((2000, 200, 10, 20), 2),
          ((14000, 1400, 25, 100), 1)]
CASES = {
    "default": {},
    "final_phase": {"price_refine": 2},
    "no_refine": {"price_refine": 0},
    "unbounded": {"bf_bound": -1},
}


def mixed_cost_graph():
    g = gen.quincy(2500, 250, 10, 20, 3)
    rng = np.random.default_rng(41)
    cost = np.where(rng.random(g.cost.shape[0]) < 0.5, 1, 1 << 30).astype(np.int64)
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, g.cap, cost, g.atype)


@pytest.fixture(scope="module")
def corpus():
    """(graph, oracle status, cost, flow value, Quincy?) — computed once, never changed."""
    out = []
    for shape, seed in QUINCY:
        g = gen.quincy(*shape, seed)
        st, cost, fv, _ = ko.cost_scaling(g)
        assert st == 0
        out.append((g, st, cost, fv, True))
    for _, g in random_hub_graphs(4711, 5, n_lo=300, n_hi=3000):
        st, cost, fv, _, _ = ko.ssp(g)
        out.append((g, st, cost, fv, False))
    g = mixed_cost_graph()
    assert g.n == 3032 and (g.n + 1) << 30 > 1 << 41
    feas, cost, flows = exact_ref.mcf(g)
    assert feas and cost > 1 << 30
    out.append((g, 0, cost, exact_ref.flow_value(g, flows), True))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_same_optimum(corpus, name):
    with native.Context(0, cell_nodes=-1, **CASES[name]) as c:
        for g, st, cost, fv, quincy in corpus:
            if st != 0:
                c.load_graph(g)
                with pytest.raises(native.KsError) as ei:
                    c.solve()
                assert ei.value.code == native.KS_E_INFEASIBLE
                continue
            r = solve_and_check(c, g, cost, fv, check_flows=g.m <= 30000)
            assert r.raw["recoveries"] == 0
            assert r.raw["solver"] == 0
            if quincy:
                check_mapping(g, c.task_mapping())
