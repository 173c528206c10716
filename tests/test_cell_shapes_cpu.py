"""The premises of tests/test_gpu_cell_layout.py, asserted without a device.

Every case of the GPU file claims a shape: residual degrees on a class bound, a
node count per class, a number of positions. Here each claim is checked from
cell_shapes.profile, so a broken generator is found on the CPU, and every case is
solved by three references that must agree: the oracle's cost scaling, its
successive shortest paths and, for cases under 2,000 arcs, the exact reference in
Python integers (tests/exact_ref.py). The restated cell_class is compared with
ks_cell.h itself, compiled for the host (tests/cell_host.cpp, g++)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cell_shapes as cs
import exact_ref
from ksched_amd import gen
from oracle import ko
from store_ref import StoreRef, delta, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_ARCS = 2000
ALL = cs.LONE + cs.LIMITS


def references(g):
    """(cost, flow value) all references agree on."""
    st, cost, fv, fl = ko.cost_scaling(g)
    assert st == 0
    vst, vcost, _ = ko.verify(g, fl)
    assert vst == 0 and vcost == cost
    st2, cost2, fv2, _, _ = ko.ssp(g)
    assert (st2, cost2, fv2) == (0, cost, fv)
    if g.m < EXACT_ARCS:
        ok, xcost, xfl = exact_ref.mcf(g)
        assert ok and xcost == cost and exact_ref.flow_value(g, xfl) == fv
    return cost, fv


# ---------------------------------------------------------------- the rules ---
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cell") / "cell_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), os.path.join(ROOT, "tests", "cell_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.cell_classes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.cell_classes.restype = None
    return L


def test_cell_class_equals_the_header(host):
    cap = np.arange(0, 1101, dtype=np.int32)
    out = np.full(cap.shape[0], -1, np.int32)
    host.cell_classes(cap.ctypes.data, out.ctypes.data, cap.shape[0])
    assert out.tolist() == [cs.cell_class(int(c)) for c in cap]
    assert out.tolist() == np.searchsorted(cs.CLASS_BOUNDS, cap, side="left").tolist()   # profile()'s form of it
    assert (host.cell_max_pos(), host.cell_ncls(), host.cell_threads()) == (cs.CELL_MAX_POS, cs.CELL_NCLS,
                                                                            cs.CELL_THREADS)


def test_restated_constants_are_the_sources():
    """The constants that no header exports, read from the source text they restate."""
    src = open(os.path.join(ROOT, "ksched_amd", "csrc", "ks_cell.hip")).read()
    assert "constexpr int UC = %d;" % cs.UC in src
    assert "constexpr int BXC = %d;" % cs.BXC in src
    assert "constexpr int CT = CELL_THREADS;" in src
    assert "return c < THR_CLASSES ? 64 : c < 4 ? (64 / (4 << c)) * ((4 << c) <= 16 ? 4 : 2) : 1;" in src
    assert [cs.items_per_wave(c) for c in range(6)] == [64, 64, 16, 4, 1, 1]


def test_seg_capacity():
    """Tight without slack; with slack the rule of ks_engine_build.hip, value by value."""
    assert [cs.seg_capacity(d, True, False, 0) for d in (0, 1, 8, 513)] == [0, 1, 8, 513]
    assert [cs.seg_capacity(d, True, True, 1) for d in (0, 5, 8, 9)] == [8, 8, 8, 16]
    assert [cs.seg_capacity(d, False, False, 1) for d in (0, 8)] == [8, 8]
    assert [cs.seg_capacity(d, True, False, 1) for d in (0, 4, 5, 8, 9, 12, 13, 17, 40, 43, 44, 100)] == \
        [4, 8, 16, 16, 16, 32, 32, 32, 64, 64, 128, 192]
    import test_gpu_store   # the store tests' restatement (slack only) is the same rule
    for d in range(0, 300):
        for alive, task in ((True, False), (True, True), (False, False)):
            assert cs.seg_capacity(d, alive, task, 1) == test_gpu_store.seg_capacity(d, alive, task)


# --------------------------------------------------------------- the generators ---
def test_ladder_gives_the_degrees_asked_for():
    pus, tasks = [5, 9, 2, 1, 7], [4, 4, 3, 3, 3, 3, 2, 5]
    g = cs.ladder(pus, tasks, pad=3, seed=5)
    p = cs.profile(g)
    assert g.n == 2 + 5 + 8 + 3 and g.m == sum(tasks) + 5 + 1 and p.positions == 2 * g.m
    assert p.deg[cs.pu_ids(g) - 1].tolist() == pus
    assert p.deg[cs.task_ids(g) - 1].tolist() == tasks
    assert p.deg[0] == 5 + 1 and p.deg[1] == 8 + 1              # the sink: #PUs + 1; U: T + 1
    assert p.deg[-3:].tolist() == [0, 0, 0] and g.ntype[-3:].tolist() == [0, 0, 0]
    assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == g.m   # simple: one arc per ordered pair
    assert not np.bincount(g.dst, minlength=g.n + 1)[cs.task_ids(g)].any()   # tasks have no in-arcs
    # every node's arc into the sink is its last one; U → sink holds every task
    for v in cs.pu_ids(g).tolist() + [2]:
        own = np.nonzero((g.src == v) | (g.dst == v))[0]
        assert g.dst[own[-1]] == 1 and g.src[own[-1]] == v
    assert g.cap[-1] == 8 and (g.cost[g.dst == 2] == cs.UNSCHED_COST).all()
    caps = g.cap[(g.dst == 1) & (g.src != 2)]
    assert ((caps >= 1) & (caps <= np.maximum(np.asarray(pus) - 1, 1))).all()
    references(g)


@pytest.mark.parametrize("pus,tasks", [([3, 3], [2, 2, 2]),          # sums differ
                                       ([5], [2, 2, 2, 2]),          # fine: one PU, four tasks
                                       ([4, 1], [4]),                # a task with more preferences than PUs
                                       ([5, 1], [3, 3]),             # a PU with more in-arcs than tasks
                                       ([4, 4, 1, 1], [5, 2, 2])])   # sums agree, no simple graph
def test_ladder_raises_when_the_degrees_cannot_be_met(pus, tasks):
    if (pus, tasks) == ([5], [2, 2, 2, 2]):
        cs.ladder(pus, tasks)
        return
    with pytest.raises(ValueError):
        cs.ladder(pus, tasks)


def test_dense_has_exactly_the_arcs_asked_for():
    for arcs in (300, 511, 512, 513, 65_536, 131_072, 131_073):
        g = cs.dense(arcs)
        assert g.m == arcs and cs.profile(g).positions == 2 * arcs
        assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == arcs
    assert cs.profile(cs.dense(131_072)).positions == cs.CELL_MAX_POS
    with pytest.raises(ValueError):
        cs.dense(200)


# ------------------------------------------------------------------- the cases ---
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_premise_and_references(case):
    g = cs.built(case)
    p = cs.profile(g)
    print(case.name, "n", g.n, "m", g.m, "per class", p.counts, "positions", p.positions)
    assert p.positions == 2 * g.m and sum(p.counts) == g.n
    assert p.cls.tolist() == [cs.cell_class(int(d)) for d in p.deg]
    if case.counts is not None:
        assert {c: p.counts[c] for c in case.counts} == case.counts
    pdeg, tdeg = p.deg[cs.pu_ids(g) - 1], p.deg[cs.task_ids(g) - 1]
    for want, have in ((case.pus, pdeg), (case.tasks, tdeg)):
        for d, k in (want or {}).items():
            assert int((have == d).sum()) == k, (d, k)
    if case.hubs is not None:
        assert sorted(p.deg[p.cls == 6].tolist()) == case.hubs
    for d in case.degrees:
        assert (p.deg == d).any(), d
    if case.n is not None:
        assert g.n == case.n
    if case.positions is not None:
        assert p.positions == case.positions
    references(g)


def test_bounds_sit_on_both_sides_of_every_class():
    """d and d + 1 fall in neighbouring classes for every bound, and the combined graph
    holds PUs on both sides of all six and tasks on both sides of the first two."""
    for c, d in enumerate(cs.CLASS_BOUNDS):
        assert (cs.cell_class(d), cs.cell_class(d + 1)) == (c, c + 1)
    g = cs.built(cs.by_name("bound-all"))
    p = cs.profile(g)
    have = set(p.deg[cs.pu_ids(g) - 1].tolist())
    assert have == {x for d in cs.CLASS_BOUNDS for x in (d, d + 1)}
    assert {4, 5, 8, 9} <= set(p.deg[cs.task_ids(g) - 1].tolist())
    assert all(k > 0 for k in p.counts)          # no class is empty in it


def test_every_partial_item_count_occurs():
    """Classes 0–3 with 1, ipw − 1, ipw, ipw + 1 and 2·ipw + 1 nodes: where each pair is."""
    where = cs.partial_pairs()
    for c in range(4):
        ipw = cs.items_per_wave(c)
        for k in (1, ipw - 1, ipw, ipw + 1, 2 * ipw + 1):
            name = where[(c, k)]
            assert cs.profile(cs.built(cs.by_name(name))).counts[c] == k
            print("class %d with %3d nodes (%d per item): %s" % (c, k, ipw, name))


def test_walk_strides_and_parity():
    """The second round of a walk starts at a node's arc into the sink; the padded graphs
    differ in N mod 32 and in the parity of N."""
    assert (cs.WAVE_ROUND, cs.HUB_ROUND) == (256, 4096)
    for name, d in (("stride-wave-256-257-512", 257), ("stride-hub-4097", 4097)):
        g = cs.built(cs.by_name(name))
        p = cs.profile(g)
        v = int(next(x for x in cs.pu_ids(g) if p.deg[x - 1] == d))
        own = np.nonzero((g.src == v) | (g.dst == v))[0]
        assert own.shape[0] == d and g.src[own[-1]] == v and (g.dst[own[:-1]] == v).all()
    ns = [cs.built(cs.by_name("parity-n-mod32-%d" % r)).n for r in (0, 1, 31)]
    assert [n % 32 for n in ns] == [0, 1, 31] and {n % 2 for n in ns} == {0, 1}
    assert [cs.built(cs.by_name("bounded-%d-tasks" % t)).supply.clip(0).sum() for t in (256, 257)] == \
        [cs.BXC, cs.BXC + 1]


def test_epsilon_cases_leave_the_powers_of_two():
    """ks_engine.hip plan(): ε before the ladder is (mult − 1) / 20 with mult = n + 1,
    rounded down to a power of two only when α is one; without refinement it is
    max|cost| · mult. Neither is a power of two for the two graphs of the ε cases."""
    for g in (cs.built(cs.by_name("bound-all")), gen.quincy(1000, 100, 5, 10, 1)):
        mult = g.n + 1
        for alpha in (10, 6):
            e = max(1, (mult - 1) // 20)
            lo = max(1, int(np.abs(g.cost).max()) * mult // (alpha * alpha))
            while e < lo:
                e *= alpha
            assert e & (e - 1), (mult, alpha)
        e = int(np.abs(g.cost).max()) * mult // 8
        assert e & (e - 1)
    references(gen.quincy(1000, 100, 5, 10, 1))


# ----------------------------------------------------------- rebuild and batch ---
def test_rebuild_plan():
    """A PU of exactly 8 positions: one more arc overflows its tight segment (16 after the
    rebuild), seven more fill it, the next overflows again (32) — classes 1, 2, 3."""
    g = cs.built(cs.by_name("bound-all"))
    v, tasks = cs.rebuild_plan(g)
    seg = cs.Segments(g)
    assert seg.deg[v - 1] == 8 and len(tasks) >= 9
    assert seg.solve() == 1
    ref = StoreRef.from_graph(g)
    want = []
    steps = [tasks[:1], tasks[1:8], tasks[8:9]]
    for part in steps:
        for t in part:
            seg.add_arc(t, v)
        ref.apply(stream([delta(kind=2, src=t, dst=v, low=0, cap=1, cost=7) for t in part]))
        want.append((seg.solve(), int(seg.deg[v - 1]), int(seg.cap[v - 1]), cs.cell_class(int(seg.cap[v - 1]))))
        references(ref.graph())
    assert want == [(2, 9, 16, 2), (2, 16, 16, 2), (3, 17, 32, 3)]


def test_batch_cells():
    graphs = [cs.built(cs.by_name(n)) for n in cs.BATCH_MIXED]
    counts = [cs.profile(g).counts for g in graphs]
    assert any(c[3] == 0 for c in counts) and any(c[6] == 3 for c in counts)
    ns = [g.n for g in graphs]
    big = ns.index(max(ns))
    assert ns[big] % 2 == 1 and 0 < big < len(ns) - 1 and len(set(map(tuple, counts))) == 5
    # the union passes 2^18 positions, each cell stays below it
    T, M, R, J = 10_000, 1_000, 25, 100
    pos = [2 * gen.quincy_sizes(T, M, R, J)[1] for _ in cs.BATCH_UNION_SEEDS]
    assert all(p < cs.CELL_MAX_POS for p in pos) and sum(pos) > cs.CELL_MAX_POS
    assert pos[0] + pos[1] < cs.CELL_MAX_POS < pos[0] + pos[1] + pos[2]   # the third cell's positions pass it
    # the infeasible cell, and the one record that repairs it
    h, (u, sink, cap) = cs.infeasible_cell()
    assert ko.cost_scaling(h)[0] != 0 and ko.ssp(h)[0] != 0 and exact_ref.mcf(h)[0] is False
    ref = StoreRef.from_graph(h)
    ref.apply(stream([delta(kind=3, src=u, dst=sink, low=0, cap=cap, cost=0)]))
    references(ref.graph())
    for n in cs.BATCH_INFEASIBLE:
        if n is not None:
            references(cs.built(cs.by_name(n)))
