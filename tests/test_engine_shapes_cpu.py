"""The premises of tests/test_gpu_engine_layout.py, asserted without a device.

Every case of the GPU file claims a shape: residual degrees on a class bound, a
node count per class and the windows that follow, CItems, hubs with their chunk
counts and tails in build()'s order, grid residues, the padded id count nn on one
side of a size switch. Here each claim is checked from engine_shapes.layout, so a
broken generator is found on the CPU, and every case is solved by three references
that must agree: the oracle's cost scaling, its successive shortest paths and,
under 2,000 arcs, the exact reference in Python integers (tests/exact_ref.py). The
restated degree_class, class_lanes, win_batches, win_slots and the constants are
compared with ks_engine_impl.h itself, compiled for the host (tests/engine_host.cpp,
g++); the constants that live in ks_engine.hip are read from its text."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cell_shapes as cs
import engine_shapes as es
import exact_ref
from oracle import ko
from store_ref import StoreRef, delta, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_ARCS = 2000
_REF: dict = {}


def references(name, g):
    """(cost, flow value, the cost scaling's flows) all references agree on; once per name."""
    if name in _REF:
        return _REF[name]
    st, cost, fv, fl = ko.cost_scaling(g)
    assert st == 0
    vst, vcost, _ = ko.verify(g, fl)
    assert vst == 0 and vcost == cost
    st2, cost2, fv2, _, _ = ko.ssp(g)
    assert (st2, cost2, fv2) == (0, cost, fv)
    if g.m < EXACT_ARCS:
        ok, xcost, xfl = exact_ref.mcf(g)
        assert ok and xcost == cost and exact_ref.flow_value(g, xfl) == fv
    _REF[name] = (cost, fv, np.asarray(fl, np.int64))
    return _REF[name]


def through(g, fl) -> np.ndarray:
    """Flow through every node (1-based index): what its in-arcs and out-arcs carry."""
    t = np.zeros(g.n + 1, np.int64)
    np.add.at(t, g.src, fl)
    np.add.at(t, g.dst, fl)
    return t


# ---------------------------------------------------------------- the rules ---
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("engine") / "engine_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "engine_host.cpp"), "-o", so],
                   check=True)
    L = ctypes.CDLL(so)
    L.engine_classes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.engine_windows.argtypes = [ctypes.c_void_p] * 3
    L.engine_constants.argtypes = [ctypes.c_void_p]
    for f in (L.engine_classes, L.engine_windows, L.engine_constants):
        f.restype = None
    return L


def test_rules_equal_the_header(host):
    cap = np.arange(0, 4201, dtype=np.int32)
    out = np.full(cap.shape[0], -1, np.int32)
    host.engine_classes(cap.ctypes.data, out.ctypes.data, cap.shape[0])
    assert out.tolist() == [es.degree_class(int(c)) for c in cap]
    assert out.tolist() == np.searchsorted(es.CLASS_BOUNDS, cap, side="left").tolist()   # layout_of()'s form of it
    lanes, batches, slots = (np.zeros(es.NGC, np.int32) for _ in range(3))
    host.engine_windows(lanes.ctypes.data, batches.ctypes.data, slots.ctypes.data)
    assert lanes.tolist() == [es.class_lanes(c) for c in range(es.NGC)] == [4, 8, 16, 32, 64, 64]
    assert batches.tolist() == [es.win_batches(c) for c in range(es.NGC)]
    assert slots.tolist() == [es.win_slots(c) for c in range(es.NGC)] == [32, 16, 8, 4, 1, 1]
    k = np.zeros(11, np.int32)
    host.engine_constants(k.ctypes.data)
    assert k.tolist() == [es.BLK, es.WAVE, es.WPB, es.NGC, es.HEAVY_MIN, es.CHUNK, es.HSPLIT, es.WPW, es.HUB_LDS,
                          es.BX_CAP, es.CCLS]
    for c, d in enumerate(es.CLASS_BOUNDS):
        assert (es.degree_class(d), es.degree_class(d + 1)) == (c, c + 1)


def test_restated_constants_are_the_sources():
    """What no header exports, read from the source text it restates."""
    csrc = os.path.join(ROOT, "ksched_amd", "csrc")
    eng = open(os.path.join(csrc, "ks_engine.hip")).read()
    bld = open(os.path.join(csrc, "ks_engine_build.hip")).read()
    hdr = open(os.path.join(csrc, "ks_engine_impl.h")).read()
    assert "#define KS_LEAF_REGS %d" % es.LEAF_REGS in eng
    assert "const bool leaf = g.expand && u < g.obeg[2];" in eng            # leaves: classes 0 and 1, ≤ 8 positions
    assert "constexpr int CYC_LDS_T = %d;" % es.CYC_LDS_T in eng
    assert "constexpr int CYC_LDS_K = %d;" % es.CYC_LDS_K in eng
    assert "constexpr int CYC_LDS_MAX = CYC_LDS_K * CYC_LDS_T;" in eng and es.CYC_LDS_MAX == 14336
    assert "return (size_t)3 * sizeof(int) * (size_t)n;" in eng             # cyc_lds_bytes
    assert "fin.lds_search = nn <= CYC_LDS_MAX && cyc_lds_bytes(nn) <= s.lds_limit;" in eng
    assert "fwd_k = o.fwd_nodes > 0 ? (int)o.fwd_nodes : (nn < %d ? %d : %d);" % (es.SMALL_NN, es.FWD_K_SMALL,
                                                                                   es.FWD_K) in eng
    assert "(!s.cell_layout && nn < %d && use_prc) ? 32 : 8;" % es.SMALL_NN in eng
    assert "(s.cell_layout || nn < %d) ? 20 :" % es.SMALL_NN in eng
    assert "nn = s.nn;" in eng
    assert "#define KS_WPW %d" % es.WPW in hdr
    # build(): the padding, the windows, nn; the HItems and the CItems
    for line in ("const int pad = (s.ncls[c] + 63) / 64 * 64;", "wv += pad / win_slots(c);", "s.hub_base = o;",
                 "s.nn = o + s.nheavy;", "for (int b = hf[h]; b < hf[h + 1]; b += CHUNK, ++c)",
                 "for (int b = cf[k]; b < cf[k + 1]; b += %d)" % es.CITEM,
                 "ci.push_back(CItem{c0 + k, b, std::min(b + %d, cf[k + 1]), b == cf[k] ? 1 : 0});" % es.CITEM,
                 "const int64_t spare = s.incremental ? std::max<int64_t>(64, s.nslots / 16) : 0;"):
        assert line in bld, line
    for line in ("int window_grid() const { return nhitems + std::max(1, (wbeg[NGC] + WPB - 1) / WPB); }",
                 "int dense_grid() const { return nhitems * HSPLIT + std::max(1, (wbeg[CCLS] + ncitems + WPB - 1) / WPB); }",
                 "int sweep_cls_blocks() const { return std::max(1, (wbeg[CCLS] + WPW * WPB - 1) / (WPW * WPB)); }",
                 "return nhitems + sweep_cls_blocks() + ncls[CCLS];",
                 "return nhitems * HSPLIT + std::max(1, (wbeg[CCLS] + ncitems + WPW * WPB - 1) / (WPW * WPB));"):
        assert line in hdr, line
    assert es.cyc_lds_limit() == 13653 and es.cyc_lds_limit(1 << 20) == es.CYC_LDS_MAX


def test_layout_of_a_hand_made_capacity_list():
    """65 nodes of 3, one of 5, two of 64, one of 65, one of 130, one of 4,096, hubs of 4,097 and 5,120."""
    cap = [3] * 65 + [5] + [64, 64] + [65, 130, 4096] + [4097] + [2] + [5120]
    L = es.layout_of(cap)
    assert L.ncls == [66, 1, 0, 0, 2, 3, 2]
    assert L.pad == [128, 64, 0, 0, 64, 64]
    assert L.windows == [4, 4, 0, 0, 64, 64] and L.occupied == [3, 1, 0, 0, 2]
    assert L.wbeg == [0, 4, 8, 8, 8, 72, 136] and L.class_windows == 72
    assert L.ncitems == 2 + 3 + 64
    assert [(h.node, h.deg, h.chunks, h.tail) for h in L.hubs] == [(72, 4097, 5, 1), (74, 5120, 5, 1024)]
    assert (L.nhitems, L.hub_base, L.nn) == (10, 320, 322)
    assert L.window_grid == 10 + 34                       # 136 windows, 4 waves a workgroup
    assert L.dense_grid == 40 + (72 + 69 + 3) // 4        # 141 items
    assert L.sparse_grid == 40 + (72 + 69 + 7) // 8
    assert L.sweep_cls_blocks == 9 and L.sweep_grid == 10 + 9 + 3
    empty = es.layout_of([4097])                           # no class window, no CItem: the max(1, …) of every grid
    assert (empty.class_windows, empty.window_grid, empty.dense_grid, empty.sparse_grid, empty.sweep_grid) == \
        (0, 5 + 1, 20 + 1, 20 + 1, 5 + 1 + 0)


# --------------------------------------------------------------- the generators ---
def test_funnel_gives_the_degrees_asked_for():
    aggs = [(5, 3), (1, 7), (9, 9)]
    g = es.funnel(aggs, tasks=11, pus=9, seed=3)
    p = es.profile(g)
    A = es.agg_ids(g)
    assert A.tolist() == [3, 4, 5]
    for a, (i, o) in zip(A.tolist(), aggs):
        assert int((g.dst == a).sum()) == i and int((g.src == a).sum()) == o and p.deg[a - 1] == i + o
        assert set(g.ntype[g.src[g.dst == a] - 1].tolist()) == {es.TASK_T}
        assert set(g.ntype[g.dst[g.src == a] - 1].tolist()) == {es.PU_T}
    assert g.n == 2 + 3 + 9 + 11 and g.m == 15 + 11 + 19 + 9 + 1
    assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == g.m           # simple
    for t in es.task_ids(g).tolist():                                      # every task reaches U
        assert int(((g.src == t) & (g.dst == 2)).sum()) == 1
    assert p.deg[1] == 11 + 1 and p.deg[0] == 9 + 1
    assert g.cap[-1] == 11 and (g.cost[g.dst == 2] == es.UNSCHED_COST).all()
    references("funnel-small", g)
    with pytest.raises(ValueError):
        es.funnel([(12, 1)], tasks=11, pus=9)
    with pytest.raises(ValueError):
        es.funnel([(1, 0)], tasks=11, pus=9)


def test_classed_gives_the_counts_asked_for():
    for cnt in ((16, 16, 4, 3, 3), (31, 1, 5, 5, 1)):
        g = es.classed(cnt, seed=5)
        assert es.layout(g).ncls[:5] == list(cnt)
    with pytest.raises(ValueError):
        es.classed((1, 1, 1, 1, 1))       # a class-4 node needs 32 neighbours


def test_with_pu_caps():
    g = cs.built(cs.by_name("bound-pu-8"))
    v = int(es.pu_ids(g)[0])
    h = es.with_pu_caps(g, {v: 5})
    changed = np.nonzero(h.cap != g.cap)[0]
    assert all(int(h.src[a]) == v and int(h.dst[a]) == 1 for a in changed) and int(h.cap[(h.src == v)][0]) == 5


# ------------------------------------------------------------------- the cases ---
@pytest.mark.parametrize("case", es.ALL, ids=lambda c: c.name)
def test_case_premise_and_references(case):
    g = es.built(case)
    p = es.profile(g)
    L = es.layout(g)
    print(case.name, "n", g.n, "m", g.m, "per class", L.ncls, "windows", L.windows, "CItems", L.ncitems,
          "hubs", [(h.node, h.deg, h.chunks, h.tail) for h in L.hubs], "nn", L.nn,
          "grids", (L.window_grid, L.dense_grid, L.sparse_grid, L.sweep_grid))
    assert sum(L.ncls) == g.n and L.cls.tolist() == [es.degree_class(int(d)) for d in p.deg]
    assert L.nn == sum(L.pad) + L.nheavy and L.nn >= g.n
    if case.ncls is not None:
        assert {c: L.ncls[c] for c in case.ncls} == case.ncls
    for d, k in (case.degrees or {}).items():
        assert int((p.deg == d).sum()) >= k, (d, k)
    if case.hubs is not None:
        assert [(h.deg, h.chunks, h.tail) for h in L.hubs] == case.hubs
    if case.nheavy is not None:
        assert L.nheavy == case.nheavy
    if case.n is not None:
        assert g.n == case.n
    if case.nn is not None:
        assert L.nn == case.nn
    if case.check is not None:
        case.check(g, L)
    cost, fv, fl = references(case.name, g)
    assert fv == int(g.supply.clip(0).sum())          # U holds every task: all of them flow
    if case.used is not None:
        t = through(g, fl)
        idle = [v for v in case.used(g) if t[v] == 0]
        assert not idle, "hubs the optimum does not use: %r" % idle


def test_bound_cases_are_the_cell_file_s():
    """The lone cases of cell_shapes whose class bounds are the engine's: PUs of d and d + 1
    positions for d = 4 … 64 (512/513 is no bound here), the partial-item cases, and the hubs
    of 4,096 (still chunked here), 4,097 and 6,145; the cell file's three-hubs case (513, 600,
    701 positions) has three chunked nodes and no hub on the engine."""
    assert [c.name for c in es.BOUNDS] == es.BOUND_NAMES
    for d in (4, 8, 16, 32, 64):
        p = es.profile(es.built(es.by_name("bound-pu-%d" % d)))
        assert (p.deg[es.pu_ids(es.built(es.by_name("bound-pu-%d" % d))) - 1] == d).sum() == 3
    assert es.layout(es.built(es.by_name("three-hubs"))).ncls[5:] == [3, 0]
    L = es.layout(es.built(es.by_name("stride-hub-4096")))
    assert L.ncls[5:] == [2, 0] and L.ncitems == 2 * 64      # 4,096 positions: 64 full CItems each


def test_every_window_count_occurs():
    """For each class 0 … 4: exactly 1, one batch (64 / G), one batch + 1, WS − 1, WS, WS + 1 and
    2·WS + 1 nodes — where each (class, count) pair is. (Class 4 has one node per window and per
    batch, so its counts are 1, 2 and 3; WS − 1 = 0 there is an empty class, which bound-pu-32
    and bound-pu-64 have between populated ones.)"""
    assert [es.batch_nodes(c) for c in range(5)] == [16, 8, 4, 2, 1]
    where = es.window_pairs()
    for c in range(es.CCLS):
        ws, b = es.win_slots(c), es.batch_nodes(c)
        for k in (1, b, b + 1, ws - 1, ws, ws + 1, 2 * ws + 1):
            if k == 0:
                continue
            L = es.layout(es.built(es.by_name(where[(c, k)])))
            assert L.ncls[c] == k
            assert L.windows[c] == -(-k // 64) * 64 // ws and L.occupied[c] == -(-k // ws)
            print("class %d with %3d nodes (%2d per batch, %2d per window): %s" % (c, k, b, ws, where[(c, k)]))
    for name, gap in (("bound-pu-32", (2,)), ("bound-pu-64", (2, 3))):      # empty classes between populated ones
        n = es.layout(es.built(es.by_name(name))).ncls
        assert all(n[c] == 0 for c in gap) and n[gap[0] - 1] > 0 and n[gap[-1] + 1] > 0


def test_window_totals():
    """wbeg[CCLS] is even whatever the graph (every class owns whole 64-node blocks, and a block
    of class 0 is two windows), so the sweeps' class blocks (8 windows each) can be full (≡ 0), hold
    two windows (≡ 2) or lack two (≡ 6), never ≡ 1 or 7; with the CItems counted, the items the
    Bellman-Ford rounds deal out reach every residue: ≡ 1 mod 4 (dense_grid) and ≡ 1 and 7 mod 8
    (sparse_grid) are built. The graph without any class window takes the max(1, …) of
    sweep_cls_blocks; a graph without class windows AND without CItems would need every node to be a
    hub (16 million arcs), so dense_grid's and sparse_grid's max(1, …) are exercised by
    test_layout_of_a_hand_made_capacity_list alone."""
    for case in es.ALL:
        if case.kind != "size":
            assert es.layout(es.built(case)).class_windows % 2 == 0
    got = {r: es.layout(es.built(es.by_name("window-total-mod8-%d" % r))) for r in (0, 2, 6)}
    assert [got[r].class_windows % 8 for r in (0, 2, 6)] == [0, 2, 6]
    assert [got[r].sweep_cls_blocks for r in (0, 2, 6)] == [1, 11, 1]
    L = es.layout(es.built(es.by_name("window-none-every-degree-65-up")))
    assert (L.class_windows, L.sweep_cls_blocks, L.ncitems > 0, L.nheavy) == (0, 1, True, 0)
    L = es.layout(es.built(es.by_name("window-classes-0-and-5-only")))
    assert L.ncls == [1200, 0, 0, 0, 0, 2, 0]


def test_leaves_are_relaxed_through_the_second_loop():
    """Tasks and PUs of exactly 5, 6 and 8 positions; in every optimum some task is placed through
    a PU's 6th, 7th or 8th position (an in-arc the expansion reads one by one, past LEAF_REGS)."""
    g = es.built(es.by_name("leaf-5-6-8-positions"))
    p = es.profile(g)
    for ids in (es.pu_ids(g), es.task_ids(g)):
        for d in (5, 6, 8):
            assert (p.deg[ids - 1] == d).sum() >= 8
    late = es.late_in_arcs(g)
    assert late.shape[0] >= 8 and (g.cost[late] <= 3).all()
    for v in es.pu_ids(g).tolist():      # a PU's arc into the sink is its last position
        own = np.nonzero((g.src == v) | (g.dst == v))[0]
        assert g.src[own[-1]] == v and (g.dst[own[:-1]] == v).all()
    _, _, fl = references("leaf-5-6-8-positions", g)
    assert int(fl[late].sum()) >= 1
    _, _, _, fl2, _ = ko.ssp(g)
    assert int(np.asarray(fl2)[late].sum()) >= 1


def test_hub_counts_reach_past_the_lds_minima():
    """0, 1, 16, 17 and 21 hubs; which hubs sit at index HUB_LDS and later (build() keeps the order
    of the node ids: the sink, U, then the PUs), and that each carries flow in the optimum — a hub
    the optimum does not use would let a dropped offer go unnoticed."""
    want = {"hubcount-0": 0, "hubcount-1-U-alone": 1, "hubcount-16-all-in-LDS": 16, "hubcount-17-one-past-LDS": 17,
            "hubcount-21-five-past-LDS": 21, "hubcount-21-hub-PUs-last": 21}
    for name, k in want.items():
        g = es.built(es.by_name(name))
        L = es.layout(g)
        assert L.nheavy == k
        if k < 16:
            continue
        _, _, fl = references(name, g)
        t = through(g, fl)
        assert [h.node for h in L.hubs] == sorted(h.node for h in L.hubs)
        carrying = [h.node for h in L.hubs if t[h.node] > 0]
        assert len(carrying) == k                                   # every hub, the sink and U included
        past = [h.node for h in L.hubs[es.HUB_LDS:]]
        assert len(past) == k - es.HUB_LDS and all(g.ntype[v - 1] == es.PU_T for v in past)
        print(name, "hubs at index %d and later:" % es.HUB_LDS, past, "flow through them", t[past].tolist())
        if k == 16:
            assert g.ntype[L.hubs[0].node - 1] != es.SINK_T and L.cls[0] == es.CCLS    # the sink stays chunked
        else:
            assert [h.node for h in L.hubs[:2]] == [1, 2]
    a = es.built(es.by_name("hubcount-21-five-past-LDS"))
    b = es.built(es.by_name("hubcount-21-hub-PUs-last"))
    assert [h.node for h in es.layout(a).hubs[es.HUB_LDS:]] == [17, 18, 19, 20, 21]
    assert [h.node for h in es.layout(b).hubs[es.HUB_LDS:]] == [4117, 4118, 4119, 4120, 4121]


def test_size_cases_sit_on_both_sides_of_the_switches():
    """The switches read nn, the padded id count (see engine_shapes), not the node count: the
    14,336 / 14,337- and 32,767 / 32,768-node graphs all lie on ONE side of theirs (nn 14,529 and
    more: the multi-launch cycle search; nn 32,770: the large-graph schedule). The cases chosen by
    nn lie on both: 13,633 / 13,697 around the 13,653 ids the LDS of gfx950 holds, 14,273 / 14,337
    around CYC_LDS_MAX (the nearest values a graph with one hub has: nn = 64·k + 1), 32,706 /
    32,770 around 32,768."""
    side = {c.name: es.size_side(es.layout(es.built(c)).nn) for c in es.SIZES}
    for n in (14336, 14337):
        for s in es.SIZE_SEEDS:
            assert side["size-quincy-n-%d-seed%d" % (n, s)] == (False, True)
    for s in es.SIZE_SEEDS:
        assert side["size-quincy-nn-lds-13633-seed%d" % s] == (True, True)
        assert side["size-quincy-nn-lds-13697-seed%d" % s] == (False, True)
        for k, v in (("max-14273", True), ("max-14337", False)):
            nn = es.layout(es.built(es.by_name("size-quincy-nn-%s-seed%d" % (k, s)))).nn
            assert es.size_side(nn, lds_bytes=1 << 20)[0] is v      # a device whose LDS holds 14,336 ids
    assert side["size-sparse-n-32767"] == side["size-sparse-n-32768"] == (False, False)
    assert side["size-sparse-nn-32706"] == (False, True) and side["size-sparse-nn-32770"] == (False, False)
    assert es.CYC_SIDES == {"lds-13633": 13633, "lds-13697": 13697, "max-14273": 14273, "max-14337": 14337}
    assert 13633 <= es.cyc_lds_limit() < 13697 and 14273 <= es.CYC_LDS_MAX < 14337


def test_few_excess_nodes():
    for t in (32, 33, 64, 65):
        g = es.built(es.by_name("excess-%d-tasks" % t))
        assert int((g.supply > 0).sum()) == t and es.layout(g).nn < es.SMALL_NN
    assert (es.FWD_K_SMALL, es.BX_CAP) == (32, 64)


def test_option_sets():
    assert es.OPTIONS == {"pos32": {"compact_pos": -1}, "hop-off": {"two_hop": -1}, "hop1": {"two_hop": 1},
                          "queue2": {"fault_inject": 512}}
    kinds = {c.kind for c in es.ALL}
    assert set(es.OPTION_KINDS) <= kinds and len({c.name for c in es.ALL}) == len(es.ALL)


# ------------------------------------------------------------------ class moves ---
@pytest.mark.parametrize("mv", es.MOVES, ids=lambda m: m.name)
def test_move_plan(mv):
    """The node's class and the hub count after the load and after every step's build, from the
    shared segment rule; every step's graph solved by the references."""
    g, v, parts = es.move_plan(mv)
    seg = es.Segments(g)
    L = es.layout(g)
    classes, nheavy, rebuilt = [int(L.cls[v - 1])], [L.nheavy], []
    assert seg.solve() == 1
    ref = StoreRef.from_graph(g)
    references(mv.name + "-loaded", g)
    for step, part in enumerate(parts):
        for t in part:
            seg.add_arc(t, v)
        before = seg.rebuilds
        ref.apply(stream([delta(kind=2, src=t, dst=v, low=0, cap=1, cost=es.MOVE_COST) for t in part]))
        rebuilt.append(seg.solve() - before)
        L = es.layout_slack(seg)
        classes.append(int(L.cls[v - 1]))
        nheavy.append(L.nheavy)
        print(mv.name, "step", step, "degree", int(seg.deg[v - 1]), "segment", int(seg.cap[v - 1]), "class",
              classes[-1], "hubs", nheavy[-1], "rebuilds", seg.rebuilds)
        assert seg.deg[v - 1] <= seg.cap[v - 1]
        references("%s-step%d" % (mv.name, step), ref.graph())
    assert (tuple(classes), tuple(nheavy), tuple(rebuilt)) == (mv.classes, mv.nheavy, mv.rebuilt)
