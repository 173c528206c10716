"""The multi-kernel engine (ks_engine*.hip: configs 2, 3 and 4 and every cell the cell
solver gives up on) on the edges of its own layout: its degree classes (≤ 4, 8, 16, 32,
64 and 4,096 positions, hubs above), the windows of 32, 16, 8, 4 and 1 node slots that
classes 0-4 are dealt in (two batches of 64 / G nodes for classes 0-3), the 64-position
CItems of the chunked class, the 1,024-position HItems of a hub with their partial tail
(HSPLIT = 4 Bellman-Ford workgroups each), hubs 0-15 whose minima are reduced in LDS
against hub 16 and later (a returning global atomic and the hub flag: offer(),
k_verify_arcs), leaves whose 6th to 8th arc records expand_leaf reads one by one, the
size switches of plan() and of the finish, few excess nodes around fwd_k and BX_CAP, and a
node that changes class — into the chunked class, into the graph's first hub, within the
hubs — across a rebuild, cold and warm.

Every case solves on an engine context (cell_nodes = −1), built once per module and option
set, and asserts through test_gpu_parity.solve_and_check: solver == 0, recoveries == 0
(cell_fallbacks == 0 is solve_and_check's), cost and flow equal to the oracle's, the
downloaded flows through ko.verify, and per PU as many mapped tasks as its arc into the
sink carries. All comparisons are integer equality.

The shapes are those of tests/engine_shapes.py; their premises (nodes per class, windows,
CItems, hub degrees, chunk tails and order, grid residues, nn) are asserted without a device
by tests/test_engine_shapes_cpu.py. After a load the residual CSR is tight, so a node's
class is that of its residual degree.

ks_result does not say which cycle search ran, which α, final_div or fwd_k plan() chose, or
whether an update was bounded: the premise of the size and excess cases is nn (and the task
count) alone. nn is the PADDED id count (every class rounded up to 64 nodes, plus the hubs),
so the 14,336 / 14,337- and 32,767 / 32,768-node graphs lie on one side of their switches;
the cases named by nn lie on both (engine_shapes, test_size_cases_sit_on_both_sides…).

Seeded defects this file was run against (scratch builds, never committed; each only skips
work, none changes an address): see the README paragraph "The engine on the edges of its own
layout"."""
import numpy as np
import pytest

import engine_shapes as es
from ksched_amd import native
from oracle import ko
from store_ref import StoreRef, delta, stream
from test_gpu_parity import check_mapping, flows_by_arc, solve_and_check

pytestmark = pytest.mark.gpu

ADD_ARC = 2
_REF: dict = {}


def oracle(name, g):
    """(cost, flow value) of g by the oracle's cost scaling, computed once per name."""
    if name not in _REF:
        st, cost, fv, _ = ko.cost_scaling(g)
        assert st == 0
        _REF[name] = (cost, fv)
    return _REF[name]


@pytest.fixture(scope="module")
def engines():
    """Engine contexts by option-set name ("default" and engine_shapes.OPTIONS), each made
    when first asked for and closed with the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = native.Context(0, cell_nodes=-1, **({} if name == "default" else es.OPTIONS[name]))
        return made[name]

    yield get
    for c in made.values():
        c.close()


def check_result(c, g, r, cost, fv):
    """What every case asserts beyond solve_and_check's own."""
    assert r.raw["solver"] == 0
    assert r.raw["cell_fallbacks"] == 0
    assert r.raw["recoveries"] == 0, "the optimality certificate needed a repair"   # (also under fault_inject bit 9:
    assert (r.cost, r.flow) == (cost, fv)                                           #  it injects no fault to repair)
    fl = flows_by_arc(c, g)
    st, vcost, _ = ko.verify(g, fl)
    assert st == 0 and vcost == cost, "the oracle's verifier rejected the downloaded flows"
    mp = c.task_mapping()
    check_mapping(g, mp)
    load = np.bincount(np.fromiter(mp.values(), np.int64, len(mp)), minlength=g.n + 1)
    into_sink = (g.ntype[g.src - 1] == es.PU_T) & (g.ntype[g.dst - 1] == es.SINK_T)
    assert load[g.src[into_sink]].tolist() == fl[into_sink].tolist(), "mapped tasks per PU ≠ the flow PU → sink"
    assert int(load.sum()) == int(fl[into_sink].sum())
    return fl


def solve_case(c, name, g):
    cost, fv = oracle(name, g)
    r = solve_and_check(c, g, cost, fv, check_flows=False)    # loads, solves; cost, flow, recoveries, cell_fallbacks
    return r, check_result(c, g, r, cost, fv)                 # … and the flows through ko.verify, once


LONE = [c for c in es.ALL if not c.name.startswith("size-quincy-")]


# ------------------------------------------------------------------ lone graphs ---
@pytest.mark.parametrize("case", LONE, ids=lambda c: c.name)
def test_case(engines, case):
    """Every case of engine_shapes under the default options (the size cases of the cycle
    search are test_cycle_search_sides)."""
    solve_case(engines("default"), case.name, es.built(case))


@pytest.mark.parametrize("case", [c for c in es.ALL if c.kind in es.OPTION_KINDS], ids=lambda c: c.name)
@pytest.mark.parametrize("opt", list(es.OPTIONS))
def test_case_off_the_defaults(engines, opt, case):
    """The bound, chunk, hub-chunk and hub-count cases with 32-byte positions (compact_pos −1),
    one hop per Bellman-Ford launch (two_hop −1), two (two_hop 1) and the 2-entry continuation
    queue (fault_inject 512: almost every enqueue overflows into the frontier flags)."""
    solve_case(engines(opt), case.name, es.built(case))


SIDES = {"n-14336": ["size-quincy-n-14336-seed%d" % s for s in es.SIZE_SEEDS],
         "n-14337": ["size-quincy-n-14337-seed%d" % s for s in es.SIZE_SEEDS]}
SIDES.update({"nn-" + k: ["size-quincy-nn-%s-seed%d" % (k, s) for s in es.SIZE_SEEDS] for k in es.CYC_SIDES})


@pytest.mark.parametrize("side", list(SIDES))
def test_cycle_search_sides(engines, side):
    """Config-2 shaped graphs around the switch between the one-workgroup cycle search
    (k_cyc_lds: nn <= 14,336 and 12·nn bytes within the LDS of one workgroup, 13,653 ids on
    gfx950) and the multi-launch one: 14,336 and 14,337 NODES (nn 14,529 and more: both on the
    multi-launch side), and nn = 13,633 / 13,697 and 14,273 / 14,337 on either side of the two
    limits. Two seeds a side; the finish ran and cancelled cycles on each side (summed).
    Which search ran is not in ks_result: the premise is nn alone."""
    cyc = 0
    for name in SIDES[side]:
        r, _ = solve_case(engines("default"), name, es.built(es.by_name(name)))
        cyc += r.raw["cycles_cancelled"]
    print(side, "cycles_cancelled", cyc)
    assert cyc > 0


# ------------------------------------------------------------------ class moves ---
@pytest.mark.parametrize("warm", [0, 1], ids=["cold", "warm"])
@pytest.mark.parametrize("mv", es.MOVES, ids=lambda m: m.name)
def test_class_move_across_a_rebuild(mv, warm):
    """A PU loaded with 64 positions gains arcs until it is chunked (128 positions, filled in
    place, then 256); an aggregator of 4,096 positions gains one arc more in a graph that had no
    hub (nheavy 0 → 1: the inbox, hub flags and claim slots appear on that rebuild); a hub of
    5,120 positions gains its 5,121st. ks_store_stats.rebuilds rises exactly where the restated
    segment rule (cell_shapes.Segments) says — the first stream switches the CSR to slack — and
    after every step cost, flow, flows and per-PU counts are the oracle's on the model graph.
    Warm, flows and prices are carried across the rebuild by slot while perm changes."""
    g, v, parts = es.move_plan(mv)
    seg = es.Segments(g)
    ref = StoreRef.from_graph(g)
    with native.Context(0, cell_nodes=-1, warm_start=warm) as c:
        solve_case(c, mv.name + "-loaded", g)
        assert c.store_stats()["rebuilds"] == seg.solve() == 1
        for step, part in enumerate(parts):
            recs = stream([delta(kind=ADD_ARC, src=t, dst=v, low=0, cap=1, cost=es.MOVE_COST) for t in part])
            for t in part:
                seg.add_arc(t, v)
            ref.apply(recs)
            c.apply_deltas(recs)
            h = ref.graph()
            cost, fv = oracle("%s-step%d" % (mv.name, step), h)
            r = c.solve()
            check_result(c, h, r, cost, fv)
            assert r.raw["warm_started"] == warm, "step %d" % step
            assert c.store_stats()["rebuilds"] == seg.solve(), "step %d" % step
            assert r.raw["rebuilt"] == mv.rebuilt[step], "step %d" % step
