"""The block-index layout of the sparse launches (residency and
dispatch order): k_sweep's grid is hub chunks, the class-window blocks, then one
workgroup per chunked-class node; a sparse k_bf_round's is the hub chunks'
workgroups, then the class windows and the chunk items, WPW per wave, strided
across the grid.

A window or chunk item that no wave owns, or that two own, gives a wrong cost, a
failed certificate or a solve that does not converge, so every case solves on the
engine (cell_nodes −1) and must give the oracle's cost and flow with no repair
and a valid mapping. The shapes sit on the boundaries of that mapping; the
degrees below are those of the residual graph (both arc ends), the class rules
those of ks_engine_impl.h (degree_class, win_slots; WPW · WPB = 8 windows per
class block):

  * Quincy (600, 100, 5, 10), (2000, 200, 10, 20), (2000, 100, 5, 20): machines
    of 14, 22 and 42 arcs — the 16-, 32- and 64-lane classes;
  * Quincy (1000, 100, 5, 10): 93 class windows (tasks, PUs, 22-arc machines),
    not a multiple of 8 — the last class block is partly empty (racks and job
    aggregators are chunked);
  * Quincy (3300, 50, 50, 500), many small jobs of 6–7 tasks: 84 chunked nodes
    (racks, machines, the cluster aggregator, the sink) against 34 class
    blocks — more chunked nodes than class blocks, and no hub;
  * general digraphs without a hub and without a chunked node, and one with
    several hubs.
"""
import pytest

from engine_shapes import WPB, WPW, layout as engine_layout   # the rules, restated beside their source lines
from graphs import random_graphs, random_hub_graphs
from ksched_amd import gen, native
from oracle import ko
from test_gpu_parity import check_mapping, solve_and_check

pytestmark = pytest.mark.gpu

QUINCY = [(600, 100, 5, 10), (2000, 200, 10, 20), (2000, 100, 5, 20), (1000, 100, 5, 10), (3300, 50, 50, 500)]
OPTS = [{"compact_pos": cp, "two_hop": th} for cp in (0, -1) for th in (1, 2)]

WINDOWS_PER_BLOCK = WPW * WPB   # 8


def layout(g):
    """(class windows that hold a node, chunked nodes, hubs) of g by the engine's class rules."""
    L = engine_layout(g)
    return sum(L.occupied), L.ncls[5], L.nheavy


@pytest.fixture(scope="module")
def corpus():
    """[(name, graph, cost, flow value, Quincy?)] — the oracle runs once per graph."""
    out = []
    for shape in QUINCY:
        g = gen.quincy(*shape, 1)
        st, cost, fv, _ = ko.cost_scaling(g)
        assert st == 0
        out.append(("quincy%r" % (shape,), g, cost, fv, True))
    plain = []
    for _, g in random_graphs(2718, 40, max_n=400):
        st, cost, fv, _, _ = ko.ssp(g)
        if st == 0 and fv > 0:
            plain.append((g, cost, fv))
    plain.sort(key=lambda e: e[0].n)
    assert len(plain) >= 2
    out.append(("random-small", *plain[0], False))
    out.append(("random-large", *plain[-1], False))
    hubs = None
    for _, g in random_hub_graphs(1618, 12, n_lo=9000, n_hi=12000):
        st, cost, fv, _, _ = ko.ssp(g)
        if st == 0 and layout(g)[2] >= 2:
            hubs = (g, cost, fv)
            break
    assert hubs is not None, "no feasible graph with several hubs in the family"
    out.append(("random-hubs", *hubs, False))
    return out


def test_the_shapes_sit_on_the_boundaries(corpus):
    by = {name: layout(g) for name, g, _, _, _ in corpus}
    for name, lay in by.items():
        print(name, "class windows %d, chunked nodes %d, hubs %d" % lay)
    assert by["quincy(1000, 100, 5, 10)"][0] % WINDOWS_PER_BLOCK != 0
    w, chunked, hubs = by["quincy(3300, 50, 50, 500)"]
    assert chunked > -(-w // WINDOWS_PER_BLOCK) and hubs == 0
    # the same two with the windows build() lays out (every class padded to whole 64-node blocks)
    full = {name: engine_layout(g) for name, g, _, _, _ in corpus}
    assert full["quincy(1000, 100, 5, 10)"].class_windows % WINDOWS_PER_BLOCK != 0
    assert full["quincy(3300, 50, 50, 500)"].ncls[5] > full["quincy(3300, 50, 50, 500)"].sweep_cls_blocks
    assert by["random-small"][2] == 0      # no hub
    assert by["random-large"][1] == 0      # no chunked node
    assert by["random-hubs"][2] >= 2


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "pos%s-hop%d" % ("16" if o["compact_pos"] == 0 else "32", o["two_hop"]))
def test_every_window_has_one_owner(corpus, opts):
    with native.Context(0, cell_nodes=-1, **opts) as c:
        for name, g, cost, fv, quincy in corpus:
            r = solve_and_check(c, g, cost, fv, check_flows=g.m <= 30000)
            assert r.raw["recoveries"] == 0, name
            assert r.raw["solver"] == 0, name
            if quincy:
                check_mapping(g, c.task_mapping())
