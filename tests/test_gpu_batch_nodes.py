"""GPU: class and resource arcs follow the cost model on a batch — ks_batch_update_nodes on the six
cells of tests/test_gpu_batch_tasks.py in one union (one device, world 1, 256 reserved ids per graph;
one case runs world 2 in one process), cold, after a pinned commit and after a preemptive one. Every
expected value comes from the host restatement of ks_update_nodes run per cell on the cell's own graph
in its own ids (tests/batch_nodes_ref.py over nodes_ref); after every call each graph of the batch
(ks_batch_get_graph), the summed statistics and the bindings are compared with the models, and the
next solve with the CPU oracle per cell.

The lists are those of a caller without a shadow of any cell's arcs (batch_nodes_ref): X → rack and
rack → machine with explicit capacities and costs from the load, machine → PU and PU → sink with
KS_CAP_KEEP, a PU's new slot count on its arc into the sink. Cells 0 and 1 share every graph-local
id, so a head that picked up another graph's base, or none, lands on a live node of the wrong cell."""
import os

import numpy as np
import pytest

from batch_nodes_ref import NodeCellModel
from batch_tasks_ref import KS_COST_ADD, offsets, sum_stats
from commit_ref import MACHINE, OTHER, PU
from ksched_amd import _build, churn, native
from nodes_ref import CAP_KEEP, offsets3
from test_gpu_batch_resources import grow, machine, refresh, relist, remove
from test_gpu_batch_tasks import CELLS, MAXT, SPARE, STATES, commit, compare, device_graph, refused, snapshot, \
    solve_and_check

pytestmark = pytest.mark.gpu

RANGE, INVALID = native.KS_E_RANGE, native.KS_E_INVALID
ZERO = dict(nodes=0, arcs_added=0, arcs_updated=0, arcs_unchanged=0, arcs_skipped=0, arcs_zeroed=0, arcs_removed=0,
            records=0)


# ----------------------------------------------------------------------- helpers ---
def make(state="cold", devices=(0,), **opts):
    cells = [churn.Cell(*p) for p in CELLS]
    b = native.Batch(devices=list(devices), **opts)
    b.reserve(SPARE)
    b.load([c.graph() for c in cells])
    models = [NodeCellModel(c) for c in cells]
    if state != "cold":
        b.solve()
        commit(b, models, state == "preemptive")
        compare(b, models)
    return b, models


def arg_of(per, n=6):
    arg = [None] * n
    for g, (tails, lists) in per.items():
        arg[g] = (tails, *offsets3(lists))
    return arg


def update(b, models, per, keep=False):
    """per {g: (tails, lists)} through ks_batch_update_nodes and the models: the summed statistics,
    every graph and the bindings. → the device's stats."""
    st = b.update_nodes(arg_of(per, len(models)), keep_unlisted=keep)
    want = sum_stats([ZERO] + [models[g].update_nodes(tails, lists, keep) for g, (tails, lists) in per.items()])
    assert st == want, (st, want)
    compare(b, models)
    return st


def held(m, u) -> list:
    """Tail u's arcs as the model holds them: listing them generates no record."""
    return [(d, a[2], a[1]) for (s, d), a in m.arcs.items() if s == u]


def span(m) -> int:
    return m.n0 + SPARE


def resize(m, p, n, preemptive, freed=()) -> tuple:
    """UpdateResourceTopology for PU p → n slots, as a caller without a shadow lists it: the whole
    sweep of the cell with the new slot count, the chain that was blocked listed explicitly (and
    freed: the nodes a completion gave room since the commit blocked them)."""
    was = set(freed) | (m.blocked_chain(p, preemptive) if n > m.slots[p] else set())
    m.slots[p] = n
    tails, lists = m.cost_lists(preemptive, was)
    rt, rl = m.pu_lists(preemptive, {p: n}, was)
    return tails + rt, lists + rl


# ------------------------------------------------------------------------- cases ---
@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
@pytest.mark.parametrize("state", STATES)
def test_three_graphs_in_one_wave(state, keep):
    """Graphs 0, 3 and 5 each list a rack (4 arcs: three of its machines and one of another rack), a
    machine (1 arc) and a PU (1 arc): 18 arcs, so one wave translates heads of three graphs; the first
    and the last graph are listed and unlisted graphs lie between listed ones."""
    pre = state == "preemptive"
    b, models = make(state)
    try:
        per = {}
        for g in (0, 3, 5):
            m = models[g]
            rack = m.racks()[g % 2]
            other = next(x for x in m.machines() if m.parent[x] != rack)
            mach = m.children(rack)[1]
            pu = m.children(mach)[0]
            lists = [m.class_list(m.children(rack)[:3], 4 + g, pre) + m.class_list([other], 9, pre, was_blocked=[other]),
                     [(pu, 3 + g, 1 if m.blocked(pu, pre) else CAP_KEEP)],
                     [(m.sink, g, CAP_KEEP)]]
            assert m.ntype[rack - 1] == OTHER and m.ntype[mach - 1] == MACHINE and m.ntype[pu - 1] == PU
            per[g] = ([rack, mach, pu], lists)
        assert sum(len(x) for _, ls in per.values() for x in ls) == 18
        st = update(b, models, per, keep)
        assert st["nodes"] == 9 and st["arcs_added"] >= 3 and st["records"] > st["arcs_added"]
        assert not (keep and st["arcs_removed"])
        assert st["arcs_removed"] or keep or state == "pinned"     # (pinned: the full machines' arcs were gone already)
        solve_and_check(b, models)
    finally:
        b.close()


def test_same_local_ids_in_cells_0_and_1():
    """Cells 0 and 1 share every graph-local id: the same tails and heads are listed in both with
    other costs and capacities, and each cell gets its own. The other four cells are untouched bit
    for bit."""
    b, models = make()
    try:
        m0, m1 = models[0], models[1]
        c = m0.cell
        assert m0.n0 == m1.n0 and m0.racks() == m1.racks() and m0.machines() == m1.machines()
        rack, mach = c.RACK0 + 1, m0.children(c.RACK0 + 1)[0]
        pu = m0.children(mach)[0]
        tails = [c.X, rack, mach, pu]
        heads = [m0.racks(), m0.children(rack)[:4] + [m0.children(c.RACK0)[0]], [pu], [m0.sink]]
        per = {}
        for g in (0, 1):
            per[g] = (tails, [[(h, 100 * (g + 1) + 7 * i + j, 2 + g + j) for j, h in enumerate(hs)]
                              for i, hs in enumerate(heads)])
        before = snapshot(b)
        st = update(b, models, per)
        assert st["nodes"] == 8 and st["arcs_added"] == 2 and st["arcs_removed"] == 2 * (len(m0.children(rack)) - 4 + 0)
        assert snapshot(b)[2:] == before[2:]
        for g in (0, 1):
            arcs = device_graph(b, g)[1]
            assert arcs[(pu, 1)][1:3] == (2 + g, 100 * (g + 1) + 21)
            assert arcs[(rack, heads[1][4])][1:3] == (2 + g + 4, 100 * (g + 1) + 7 + 4)
        solve_and_check(b, models)
    finally:
        b.close()


def test_unlisted_arcs_go_in_their_own_cell_only():
    """Cell 0's first rack and its first unscheduled aggregator listed with empty lists: the rack loses
    every arc into its machines, the aggregator keeps its arc into its cell's sink. The same-numbered
    rack and aggregator of cell 1 are untouched, as is every other cell."""
    b, models = make()
    try:
        m = models[0]
        rack, agg = m.cell.RACK0, m.aggs[0]
        assert (agg, m.sink) in m.arcs and (agg, models[1].sink) in models[1].arcs
        n = len(held(m, rack))
        assert n == len(m.children(rack)) == len(held(models[1], rack)) > 0
        before = snapshot(b)
        st = update(b, models, {0: ([rack, agg], [[], []])})
        assert st == dict(ZERO, nodes=2, arcs_removed=n, records=n)
        assert snapshot(b)[1:] == before[1:]
        arcs = device_graph(b, 0)[1]
        assert (agg, m.sink) in arcs and not [k for k in arcs if k[0] == rack]
        assert len([k for k in device_graph(b, 1)[1] if k[0] == rack]) == n
        solve_and_check(b, models)
    finally:
        b.close()


@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
def test_the_update_resource_topology_recipe(preemptive):
    """Cold, three PUs of cells 2 and 4 each are cut to 3 slots through the recipe itself (the cells
    then have fewer slots than tasks, so the solve fills every PU), then the solve and the commit.
    Cell 2: a PU with 3 slots and 3 bound tasks goes to 5. Cell 4: two of a PU's tasks complete
    (ks_batch_complete_tasks), then it goes from 3 slots to 1. Both in one ks_batch_update_nodes, then
    ks_batch_complete_tasks with every k == 0 and the caps flag carries the counts up the chains.
    Pinned, the full PU's chain arcs went with the commit's capacity rule: KS_CAP_KEEP on them is
    refused naming the graph, and the recipe lists them with an explicit capacity (ADD_ARC)."""
    b, models = make()
    try:
        up, down = models[2], models[4]
        per = {}
        for g, m in ((2, up), (4, down)):
            cut = {p: 3 for p in sorted(m.slots)[4:7]}
            m.slots.update(cut)
            tails, lists = m.cost_lists(preemptive)
            rt, rl = m.pu_lists(preemptive, cut)
            per[g] = (tails + rt, lists + rl)
            assert sum(m.slots.values()) < len(m.tasks())
        st = update(b, models, per)
        assert st["arcs_updated"] >= 6 and st["arcs_added"] == st["arcs_removed"] == 0
        refresh(b, models, preemptive)
        solve_and_check(b, models)
        commit(b, models, preemptive)
        compare(b, models)
        a, z = sorted(up.slots)[4], sorted(down.slots)[4]
        load = down.load()
        assert up.slots[a] == down.slots[z] == 3 and up.load().get(a, 0) == 3 and load.get(z, 0) == 3
        done = [None] * 6
        done[4] = [t for t in down.tasks(bound=True) if down.bind[t] == z][:load[z] - 1]
        left, st = b.complete_tasks(done, resource_caps=True, preemptive=preemptive,
                                    unsched_ids=[down.aggs if g == 4 else None for g in range(6)])
        wl, wst = down.complete(done[4], True, preemptive, down.aggs)
        assert left[4].tolist() == wl == [z] * len(done[4]) and st == wst
        compare(b, models)
        chain = [(up.parent[v], v) for v in (a, up.parent[a], up.parent[up.parent[a]])]
        assert chain[2][0] == up.cell.X
        if not preemptive:
            assert not [k for k in chain[:2] if k in up.arcs]                  # the rule deleted machine → PU, rack → machine
            before = snapshot(b)
            mach = up.parent[a]
            refused(lambda: b.update_nodes(arg_of({2: ([a, mach], [[(up.sink, 0, 5)], [(a, 1, CAP_KEEP)]])})), INVALID,
                    "KS_CAP_KEEP", "graph 2", f"node {mach}", f"into {a}")
            assert snapshot(b) == before
        was = up.blocked_chain(a, preemptive)
        assert not was if preemptive else {a, up.parent[a]} <= was
        per = {2: resize(up, a, 5, preemptive), 4: resize(down, z, 1, preemptive)}
        st = update(b, models, per)
        assert st["arcs_added"] == len(was)
        assert device_graph(b, 2)[1][(a, up.sink)][1] == 5 and device_graph(b, 4)[1][(z, down.sink)][1] == 1
        refresh(b, models, preemptive)
        for m in (up, down):
            assert m.stale_caps(preemptive) == 0 and m.dangling() == []
        arcs = device_graph(b, 2)[1]
        for u, v in chain:
            assert arcs[(u, v)][1] == up.room(v, preemptive), (u, v)
        arcs = device_graph(b, 4)[1]
        for v in (z, down.parent[z]):
            room = down.room(v, preemptive)
            assert arcs.get((down.parent[v], v), (0, 0))[1] == room == (1 if preemptive else 0)
        solve_and_check(b, models)
    finally:
        b.close()


def raw(b, entries, flags=0, n=6):
    """The C call on hand-made entries {g: (nodes, k, arc_off, arcs)} (arrays or None) → (rc, message)."""
    ls = (native.KsBatchNodeList * max(n, 1))()
    keep = []
    for g, (nodes, k, off, arcs) in entries.items():
        for name, x in (("nodes", nodes), ("arc_off", off), ("arcs", arcs)):
            if x is not None:
                keep.append(x)
                setattr(ls[g], name, x.ctypes.data)
        ls[g].k = k
    rc = b._L.ks_batch_update_nodes(b._h, flags, n, ls, None)
    return rc, b._L.ks_batch_last_error(b._h).decode()


def test_id_bounds_and_refusals():
    """Every refusal changes nothing on any graph (a good list of graph 0 rides in most calls): the
    host's range check of the tails, the device's range check of the heads (first in input order,
    before every other refusal), the lone call's refusals with the graph named, and the malformed
    calls."""
    b, models = make()
    try:
        m = models[3]
        c = m.cell
        sp = span(m)
        good = ([models[0].cell.X], [models[0].class_list(models[0].racks(), 6, False)])
        before = snapshot(b)

        def one(g, tails, lists, **kw):
            per = {0: good} if g != 0 else {}
            per[g] = (tails, lists)
            return lambda: b.update_nodes(arg_of(per), **kw)

        def unchanged():
            assert snapshot(b) == before

        # tails: the host, before any device is asked
        refused(one(3, [0], [[]]), RANGE, "graph 3", "node 0")
        unchanged()
        refused(one(3, [c.X, sp + 1], [[], []]), RANGE, "graph 3", f"node {sp + 1}")
        unchanged()
        # heads: the device's range check; span + 1 of graph 0 is graph 1's sink in the union's ids
        m0 = models[0]
        sp0 = span(m0)
        x = m0.cell.X
        msg = refused(one(0, [x], [[(sp0 + 1, 3, 2)]], keep_unlisted=True), RANGE, "graph 0", f"node {x}", f"head {sp0 + 1}",
                      f"1..{sp0}")
        unchanged()
        # span itself is a reserved id, in range and dead: the lone call's refusal
        refused(one(0, [x], [[(sp0, 3, 2)]], keep_unlisted=True), INVALID, "graph 0", f"node {x}", f"head {sp0}",
                "not a legal head")
        unchanged()
        # a dead tail in range is the lone call's as well, and no union id shows
        msg = refused(one(3, [sp], [[]]), INVALID, "graph 3", f"node {sp}")
        assert str(sp + sum(span(mm) for mm in models[:3])) not in msg
        unchanged()
        # three graphs: an offender in the LAST graph's first arc and one in the FIRST graph's last arc
        m5 = models[5]
        per = {0: ([x], [m0.class_list(m0.racks(), 6, False)[:-1] + [(sp0 + 2, 1, 1)]]),
               3: ([c.X], [m.class_list(m.racks(), 6, False)]),
               5: ([m5.cell.X], [[(span(m5) + 9, 1, 1)] + m5.class_list(m5.racks(), 6, False)])}
        msg = refused(lambda: b.update_nodes(arg_of(per)), RANGE, "graph 0", f"head {sp0 + 2}")
        assert "graph 5" not in msg and str(span(m5) + 9) not in msg
        unchanged()
        # ... and it comes before the device's other refusals: a task tail earlier in the input
        per[0] = ([m0.tasks()[0], x], [[], per[0][1][0]])
        refused(lambda: b.update_nodes(arg_of(per)), RANGE, "graph 0", f"head {sp0 + 2}")
        unchanged()
        # the lone call's refusals, each once through the batch, each naming its graph
        rack = c.RACK0
        refused(one(3, [rack, c.X, rack], [[], [], []]), INVALID, "graph 3", f"node {rack}", "listed once")
        unchanged()
        refused(one(3, [m.tasks()[0]], [[]]), INVALID, "graph 3", f"node {m.tasks()[0]}")
        refused(one(3, [m.sink], [[]]), INVALID, "graph 3", f"node {m.sink}")
        unchanged()
        mach = m.children(rack)[0]
        refused(one(3, [rack], [[(mach, 1, 1), (mach + 1, 1, 1), (mach, 2, 1)]]), INVALID, "graph 3", f"node {rack}",
                f"head {mach}", "listed twice")
        unchanged()
        far = next(v for v in m.machines() if m.parent[v] != rack)
        refused(one(3, [rack], [[(far, 1, CAP_KEEP)]]), INVALID, "graph 3", f"node {rack}", "KS_CAP_KEEP", f"into {far}")
        unchanged()
        refused(one(3, [mach], [[(m.sink, 1, 1)]]), INVALID, "graph 3", f"node {mach}", "not a legal head")
        refused(one(3, [rack], [[(mach, (1 << 40) + 1, 1)]]), RANGE, "graph 3", f"node {rack}", "the cost")
        refused(one(3, [rack], [[(mach, 1, (1 << 53) + 1)]]), RANGE, "graph 3", f"node {rack}", "the capacity")
        unchanged()
        refused(one(3, [rack], [[]], flags=2), INVALID, "flag")
        refused(one(3, [rack], [[]], flags=3), INVALID, "flag")
        unchanged()
        # the malformed calls, through the C entry point
        ids = np.asarray([rack, c.X], np.uint64)
        off = np.asarray([0, 1, 2], np.uint64)
        arcs = np.zeros(2, native.NODE_ARC_DT)
        arcs["dst"], arcs["cap"] = [mach, rack], 1
        assert raw(b, {3: (ids, 2, off, arcs)}, n=5)[0] == INVALID                 # a list count other than the graphs
        assert raw(b, {3: (ids, 2, off, arcs)}, n=7)[0] == INVALID
        rc, msg = raw(b, {3: (None, 2, off, arcs)})
        assert rc == INVALID and "graph 3" in msg and "null" in msg
        rc, msg = raw(b, {3: (ids, 2, None, arcs)})
        assert rc == INVALID and "graph 3" in msg and "null" in msg
        rc, msg = raw(b, {3: (ids, 2, off, None)})
        assert rc == INVALID and "graph 3" in msg and "null arc array" in msg
        rc, msg = raw(b, {3: (ids, 2, np.asarray([1, 1, 2], np.uint64), arcs)})
        assert rc == INVALID and "graph 3" in msg and "arc_off[0]" in msg
        rc, msg = raw(b, {3: (ids, 2, np.asarray([0, 2, 1], np.uint64), arcs)})
        assert rc == INVALID and "graph 3" in msg and "decreases" in msg and f"node {c.X}" in msg
        unchanged()
        compare(b, models)
        # the legal call after all of them, and every list empty
        st = b.update_nodes([None] * 6)
        assert st == ZERO
        assert raw(b, {3: (ids, 2, off, arcs)})[0] == 0
        models[3].update_nodes([rack, c.X], [[(mach, 0, 1)], [(rack, 0, 1)]])
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_a_class_outgrows_its_segment():
    """Cell 2's first rack gains an arc to every machine of its cell, 40 more than it held and more
    than its segment's slack; the neighbours' segments and the next solve stay right."""
    b, models = make()
    try:
        m = models[2]
        rack = m.cell.RACK0
        have = len(held(m, rack))
        lst = m.class_list(m.machines(), 8, False)
        st = update(b, models, {2: ([rack], [lst])})
        assert st["arcs_added"] == len(m.machines()) - have == 40 and st["arcs_updated"] == have
        solve_and_check(b, models)
        # in place now: a second sweep of the same tail
        st = update(b, models, {2: ([rack], [[(h, co + 1, cap) for h, co, cap in lst]])})
        assert st["arcs_updated"] == st["records"] == len(lst)
        solve_and_check(b, models)
    finally:
        b.close()


def test_no_record_no_change():
    """Listing what the store holds returns records == 0, keeps the mapping readable, and under
    warm_start = 1 the next solve has no cell to run."""
    b, models = make(warm_start=1)
    try:
        r0, pu0, cost0, flow0 = solve_and_check(b, models)
        assert r0.raw["cells_run"] == 6
        per = {}
        for g in (0, 4):
            m = models[g]
            rack = m.racks()[0]
            mach = m.children(rack)[0]
            tails = [m.cell.X, rack, mach, m.children(mach)[0], m.aggs[0]]
            lists = [held(m, u) for u in tails]
            lists[1] = [(d, co, CAP_KEEP if i % 2 else cap) for i, (d, co, cap) in enumerate(lists[1])]
            per[g] = (tails, lists)
        for keep in (False, True):
            st = update(b, models, per, keep)
            assert st["records"] == 0 and st["arcs_unchanged"] == sum(len(x) for _, ls in per.values() for x in ls) > 20
            pu, cost, flow = b.gather(MAXT)                           # the mapping is still served
            assert np.array_equal(pu, pu0) and np.array_equal(cost, cost0) and np.array_equal(flow, flow0)
        assert b.update_nodes([None] * 6) == ZERO
        r1, pu1, cost1, flow1 = solve_and_check(b, models)
        assert r1.raw["cells_run"] == 0
        assert np.array_equal(pu1, pu0) and np.array_equal(cost1, cost0)
    finally:
        b.close()


def test_warm_start_runs_the_touched_cells():
    """warm_start = 1: after an update in cells 0 and 5, two cells run and the other four cells'
    gather rows are bit-identical."""
    b, models = make(warm_start=1)
    try:
        r0, pu0, cost0, flow0 = solve_and_check(b, models)
        assert r0.raw["cells_run"] == 6
        per = {}
        for g in (0, 5):
            m = models[g]
            tails, lists = m.cost_lists(False)
            per[g] = (tails, [[(h, co + 3 * (i + 1), cap) for i, (h, co, cap) in enumerate(lst)] for lst in lists])
        st = update(b, models, per)
        assert st["arcs_updated"] == st["records"] > 0
        r1, pu1, cost1, flow1 = solve_and_check(b, models)
        assert r1.raw["cells_run"] == 2
        for g in (1, 2, 3, 4):
            assert np.array_equal(pu1[g], pu0[g]) and cost1[g] == cost0[g] and flow1[g] == flow0[g], g
    finally:
        b.close()


def test_two_local_devices():
    """World 2 in one process (the test build with the in-process communicator; graph g on rank g mod
    2): lists for graphs of both ranks go in one call. A tail out of range in a graph of rank 1 is found
    on the host before any device is asked, so rank 0's graphs are unchanged too; then the good call
    and a solve."""
    if not os.path.exists(_build.variant_path(_build.FAKE_COMM_TAG)):
        pytest.fail("ksched_amd/libksmcmf_fakecomm.so is not built (__graft_entry__.build())")
    b, models = make("preemptive", devices=(0, 0), variant=_build.FAKE_COMM_TAG)
    try:
        per = {}
        for g in (0, 1, 3, 4):
            tails, lists = models[g].cost_lists(True)
            rt, rl = models[g].pu_lists(True)
            per[g] = (tails + rt[:7], lists + rl[:7])
        before = snapshot(b)
        bad = dict(per)
        bad[3] = (per[3][0] + [span(models[3]) + 1], per[3][1] + [[]])
        refused(lambda: b.update_nodes(arg_of(bad)), RANGE, "graph 3", f"node {span(models[3]) + 1}")
        assert snapshot(b) == before                  # rank 1's list refused on the host: rank 0 did not run
        # a head out of range on rank 1: its device's refusal, all or nothing there
        bad[3] = ([models[3].cell.X], [[(span(models[3]) + 1, 1, 1)]])
        bad = {3: bad[3]}
        refused(lambda: b.update_nodes(arg_of(bad), keep_unlisted=True), RANGE, "graph 3", f"head {span(models[3]) + 1}")
        assert snapshot(b) == before
        st = update(b, models, per)
        assert st["nodes"] == sum(len(t) for t, _ in per.values()) and st["arcs_updated"] > 0
        solve_and_check(b, models)
    finally:
        b.close()


@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
def test_three_full_rounds(preemptive):
    """commit → remove → complete → add resources → refresh → add → update tasks → update nodes →
    costs → solve, three times in both commit modes, every step through the batch calls only. Each
    round every cell's X → rack and rack → machine costs follow the machines' load, every machine → PU
    and PU → sink arc is re-costed, and one PU of one cell changes its slot count (followed by the
    capacity refresh). Nothing read from the device enters a model except the commits' deltas and the
    removals' outputs."""
    b, models = make(warm_start=1)
    state = "preemptive" if preemptive else "pinned"
    rng = np.random.default_rng(177 + preemptive)
    seen = dict(removed=0, grown=0, raised=0, lowered=0, added=0)
    try:
        for rnd in range(3):
            solve_and_check(b, models)
            commit(b, models, preemptive)
            compare(b, models)
            marked = [m.blocked_nodes(preemptive) for m in models]      # pinned: the arcs into these went with the commit
            # remove: a machine in about half of the cells
            per = {}
            for g, m in enumerate(models):
                ms = m.machines()
                if rng.random() < 0.5 and len(ms) > 6:
                    per[g] = [int(rng.choice(ms))]
            evicted = remove(b, models, per, state) if per else {}
            returning = {g: set(t) for g, t in evicted.items()}
            seen["removed"] += len(per)
            # complete: bound tasks and one waiting task per cell, in four of the six cells
            done, want = [None] * 6, []
            for g in (0, 1, 3, 4):
                m = models[g]
                waiting = [t for t in m.tasks(bound=False) if t not in returning.get(g, ())]
                done[g] = m.tasks(bound=True)[rnd::7][:max(2, m.cell.T0 // 20)] + waiting[:1]
            left, st = b.complete_tasks(done, resource_caps=True, preemptive=preemptive,
                                        unsched_ids=[m.aggs if done[g] is not None else None
                                                     for g, m in enumerate(models)])
            for g in (0, 1, 3, 4):
                wl, wst = models[g].complete(done[g], True, preemptive, models[g].aggs)
                assert left[g].tolist() == wl, (rnd, g)
                want.append(wst)
            assert st == sum_stats(want), (rnd, st, sum_stats(want))
            compare(b, models)
            # add resources: a machine in some cells, then the refresh
            per = {g: machine(m, rack=m.cell.RACK0 + int(rng.integers(m.cell.R)), slots=1 + g % 3)
                   for g, m in enumerate(models) if rng.random() < 0.5}
            if per:
                seen["grown"] += len(per)
                grow(b, models, per)
                refresh(b, models, preemptive)
            # add tasks: freed ids first, then fresh ones, in five cells
            arrive, want = [None] * 6, []
            for g in (0, 1, 2, 4, 5):
                m = models[g]
                tasks = m.new_ids(m.cell.T0 // 20 + 2)
                ls = m.relist(tasks, base_cost=30 + rnd)
                arrive[g] = (tasks, *offsets(ls))
                want.append((g, tasks, ls))
            st = b.add_tasks(arrive, unsched_ids=[m.aggs if arrive[g] is not None else None
                                                  for g, m in enumerate(models)], unsched_sink_cost=11)
            assert st == sum_stats(models[g].arrive(tasks, ls, models[g].aggs, 11) for g, tasks, ls in want)
            compare(b, models)
            # update tasks: pinned, the evicted tasks get their lists back
            relist(b, models, {g: sorted(t for t in ts if t in models[g].alive) for g, ts in returning.items()}, state)
            # update nodes: the whole sweep of every cell from the caller's own knowledge, one PU resized
            g = (2 * rnd + 1) % 6
            m = models[g]
            load = m.load()
            shrink = sorted((p for p in m.slots if m.slots[p] - 1 >= max(load.get(p, 0), 1)),
                            key=lambda p: (m.slots[p] - 1 != load.get(p, 0), p))     # down to its bound tasks first
            per = {}
            if rnd % 2 and shrink:
                p = shrink[0]
                per[g] = resize(m, p, m.slots[p] - 1, preemptive, m.freed(marked[g], preemptive))
                seen["lowered"] += 1
            else:
                full = [p for p in sorted(m.slots) if load.get(p, 0) >= m.slots[p]] or sorted(m.slots)
                p = full[rnd % len(full)]
                per[g] = resize(m, p, m.slots[p] + 2, preemptive, m.freed(marked[g], preemptive))
                seen["raised"] += 1
            for h, mm in enumerate(models):
                if h != g:
                    was = mm.freed(marked[h], preemptive)
                    tails, lists = mm.cost_lists(preemptive, was)
                    rt, rl = mm.pu_lists(preemptive, None, was)
                    per[h] = (tails + rt, lists + rl)
            st = update(b, models, per)
            seen["added"] += st["arcs_added"]
            assert st["arcs_updated"] > 0 and st["arcs_removed"] == 0
            refresh(b, models, preemptive)
            for mm in models:
                assert mm.stale_caps(preemptive) == 0 and mm.dangling() == []
            # costs: every aggregator of every graph ages
            changed = b.update_unsched_costs(10, mode=KS_COST_ADD, continuation=0 if preemptive else 3,
                                             unsched_ids=[m.aggs for m in models])
            assert changed == sum(m.age(10, KS_COST_ADD, 0 if preemptive else 3) for m in models)
            compare(b, models)
        solve_and_check(b, models)
        assert seen["removed"] and seen["grown"] and seen["raised"] and seen["lowered"], seen
        if not preemptive:
            assert seen["added"], seen                # the arcs into a full PU's chain came back with its new slots
    finally:
        b.close()
