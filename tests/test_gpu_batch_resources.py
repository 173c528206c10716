"""GPU: the resource side of a round on a batch — ks_batch_remove_resources and
ks_batch_add_resources on the six cells of tests/test_gpu_batch_tasks.py in one union (one device,
world 1, 256 reserved ids per graph; one case runs world 2 in one process), cold, after a pinned commit and after a preemptive one. Every
expected value comes from the host restatements of the lone calls run per cell on the cell's own
graph in its own ids (tests/batch_resources_ref.py over remove_ref and grow_ref); after every call
each graph of the batch (ks_batch_get_graph), the summed statistics and the bindings are compared
with the models, and the next solve with the CPU oracle per cell.

The refresh sequence of a round is part of every case that solves: after a pinned commit an evicted
task has no arc left and gets its list back, its aggregator's among it, through
ks_batch_update_tasks with explicit unsched_ids; after a growth with an edge the capacities are
refreshed by ks_batch_complete_tasks with every k == 0 (tests/test_batch_resources_cpu.py shows on
the host that every cell is feasible then)."""
import ctypes as C
import os

import numpy as np
import pytest

from batch_resources_ref import ResCellModel
from batch_tasks_ref import KS_COST_ADD, offsets, sum_stats
from commit_ref import MACHINE, PU, SINK
from grow_ref import TREE
from ksched_amd import _build, churn, native
from test_gpu_batch_tasks import CELLS, MAXT, SPARE, STATES, commit, compare, device_graph, refused, snapshot, \
    solve_and_check

pytestmark = pytest.mark.gpu

RANGE, INVALID = native.KS_E_RANGE, native.KS_E_INVALID
PREEMPT = native.KS_DELTA_PREEMPT


# ----------------------------------------------------------------------- helpers ---
def make(state="cold", devices=(0,), **opts):
    cells = [churn.Cell(*p) for p in CELLS]
    b = native.Batch(devices=list(devices), **opts)
    b.reserve(SPARE)
    b.load([c.graph() for c in cells])
    models = [ResCellModel(c) for c in cells]
    if state != "cold":
        b.solve()
        commit(b, models, state == "preemptive")
        compare(b, models)
    return b, models


def grow(b, models, per):
    """per {g: (nodes, edges)} through ks_batch_add_resources and the models; → the device's stats."""
    arg = [None] * len(models)
    for g, e in per.items():
        arg[g] = e
    st = b.add_resources(arg)
    want = [models[g].grow(*e) for g, e in per.items()]
    assert st == sum_stats(want), (st, sum_stats(want))
    compare(b, models)
    return st


def refresh(b, models, pre):
    """The capacity refresh after a growth: every k == 0, the caps flag, the mode's rule."""
    left, st = b.complete_tasks([None] * len(models), resource_caps=True, preemptive=pre)
    assert all(x is None for x in left)
    want = sum_stats(m.refresh_caps(pre) for m in models)
    assert st == want, (st, want)
    compare(b, models)
    return st


def remove(b, models, per, state, caps=True):
    """per {g: roots} (in pinned state the unreachable nodes beneath them are named too) through
    ks_batch_remove_resources and the models: removed per graph, the evictions grouped by graph in
    task order, the stats, every graph and the bindings. → {g: evicted tasks}."""
    pre = state == "preemptive" and caps
    arg = [None] * len(models)
    for g, roots in per.items():
        arg[g] = models[g].named_roots(roots)
    removed, ev, st = b.remove_resources(arg, resource_caps=caps, preemptive=pre)
    want_ev, want_st, out = [], [], {}
    for g, m in enumerate(models):
        if g not in per:
            assert removed[g].size == 0, f"graph {g} is untouched"
            continue
        rm, e, s = m.remove(arg[g], caps, pre)
        assert removed[g].tolist() == rm and rm == sorted(rm), f"graph {g}"
        want_ev += [(PREEMPT, g, t, p) for t, p in e]
        want_st.append(s)
        out[g] = [t for t, _ in e]
    assert list(zip(ev["type"].tolist(), ev["graph"].tolist(), ev["task"].tolist(), ev["pu"].tolist())) == want_ev
    assert st == sum_stats(want_st), (st, sum_stats(want_st))
    compare(b, models)
    for g, tasks in out.items():
        assert not b.bindings(g, tasks).any()
    return out


def relist(b, models, evicted, state):
    """Pinned: the evicted tasks' arcs come back, their aggregator among them."""
    if state != "pinned" or not any(evicted.values()):
        return
    lists, ids, want = [None] * len(models), [None] * len(models), []
    for g, tasks in evicted.items():
        if not tasks:
            continue
        m = models[g]
        ls = m.relist(tasks)
        lists[g], ids[g] = (tasks, *offsets(ls)), m.aggs
        want.append(m.refresh(tasks, ls, m.aggs, 0))
    st = b.update_tasks(lists, unsched_ids=ids, unsched_sink_cost=0)
    assert st == sum_stats(want), (st, sum_stats(want))
    compare(b, models)


def machine(m, rack=None, fresh=False, slots=3):
    c = m.cell
    return m.machine(c.RACK0 + 1 if rack is None else rack, m.new_res_ids(2, fresh), slots)


def root_lists(per, n=6):
    ls = (native.KsBatchResList * n)()
    keep = []
    for g, r in per.items():
        a = np.ascontiguousarray(r, np.uint64)
        keep.append(a)
        ls[g].roots, ls[g].k = a.ctypes.data, a.shape[0]
    return ls, keep


# ------------------------------------------------------------------------- growth ---
@pytest.mark.parametrize("state", STATES)
def test_machines_join_three_graphs(state):
    """A machine + PU joins graphs 0, 3 and 5 in one call, the chains listed up to the cluster node: 6
    node records and 9 edge records, so three graphs' records share one wave in the translation and
    in the sums; the first and the last graph are listed and unlisted graphs lie between them."""
    b, models = make(state)
    try:
        per = {g: machine(models[g]) for g in (0, 3, 5)}
        assert sum(len(n) for n, _ in per.values()) == 6 and sum(len(e) for _, e in per.values()) == 9
        st = grow(b, models, per)
        assert st["nodes"] == 6 and st["pus"] == 3 and st["sink_arcs"] == 3 and st["arcs_skipped"] == 0
        refresh(b, models, state == "preemptive")
        solve_and_check(b, models)
    finally:
        b.close()


def test_same_local_id_in_two_cells():
    """Cells 0 and 1 share every graph-local id: each receives a PU with the same local id in one
    call, and each PU → sink arc ends at its own cell's sink (both sinks are local id 1)."""
    b, models = make()
    try:
        assert models[0].sink == models[1].sink == 1 and models[0].n0 == models[1].n0
        per = {0: machine(models[0], slots=2), 1: machine(models[1], slots=5)}
        pid = per[0][0][1][0]
        assert per[1][0][1][0] == pid
        grow(b, models, per)
        for g, slots in ((0, 2), (1, 5)):
            assert device_graph(b, g)[1][(pid, 1)] == (0, slots, 0, 0)
        refresh(b, models, False)
        solve_and_check(b, models)
    finally:
        b.close()


def test_first_and_last_cell():
    """A PU in the first cell and one in the last cell in one call: the bisection's ends."""
    b, models = make("pinned")
    try:
        grow(b, models, {0: machine(models[0]), 5: machine(models[5])})
        refresh(b, models, False)
        solve_and_check(b, models)
    finally:
        b.close()


@pytest.mark.parametrize("state", STATES)
def test_freed_ids_next_to_fresh_ids(state):
    """A machine leaves graph 3; the growth that follows reuses its two ids for one machine and takes
    fresh ids for another, beneath the other rack."""
    b, models = make(state)
    try:
        m = models[3]
        ev = remove(b, models, {3: [m.cell.MACH0 + 2]}, state)
        relist(b, models, ev, state)
        freed = list(m.res_free)
        assert len(freed) == 2
        n1, e1 = machine(m, rack=m.cell.RACK0)
        n2, e2 = machine(m, rack=m.cell.RACK0 + 1, fresh=True)
        assert [x[0] for x in n1] == freed and all(x[0] > m.n0 for x in n2)
        grow(b, models, {3: (n1 + n2, e1 + e2)})
        refresh(b, models, state == "preemptive")
        solve_and_check(b, models)
    finally:
        b.close()


def test_id_bounds_and_refusals():
    """A node id equal to span is accepted. A node id of span + 1, an edge parent of 0 and an edge
    child of span + 1 are KS_E_RANGE naming the graph and the id; an edge child that is in range, dead
    in its graph and live under the same local id in another graph is the device's KS_E_INVALID naming
    the graph. Every graph is byte-identical after a refusal, a good list in the same call included."""
    b, models = make()
    try:
        m = models[3]
        c = m.cell
        span = m.n0 + SPARE
        good = machine(models[0])

        def one(g, nodes, edges):
            arg = [None] * 6
            arg[0] = good
            arg[g] = (nodes, edges)
            return lambda: b.add_resources(arg)

        rack = c.RACK0
        before = snapshot(b)
        pu = lambda i: [(i, PU, 2, 0)]
        refused(one(3, pu(span + 1), [(c.MACH0, span + 1, 1, TREE)]), RANGE, "graph 3", str(span + 1))
        assert snapshot(b) == before
        refused(one(3, [(span, MACHINE, 0, 0)], [(0, span, 2, TREE)]), RANGE, "graph 3", "parent 0")
        assert snapshot(b) == before
        refused(one(3, [(span, MACHINE, 0, 0)], [(rack, span, 2, TREE), (span, span + 1, 1, TREE)]), RANGE, "graph 3",
                f"child {span + 1}")
        assert snapshot(b) == before
        # dead in graph 5, live in graph 4: the local id of a task of the larger cell
        dead = models[5].n0 + 7
        assert dead <= models[4].n0 and dead not in models[5].alive and dead in models[4].alive
        msg = refused(one(5, [], [(models[5].cell.RACK0, dead, 2, TREE)]), INVALID, "graph 5", f"child {dead}")
        assert str(dead + sum(mm.n0 + SPARE for mm in models[:5])) not in msg       # no union id
        assert snapshot(b) == before
        compare(b, models)
        # the legal one: the PU's id is span itself
        nodes = [(span - 1, MACHINE, 0, 0), (span, PU, 2, 0)]
        edges = [(rack, span - 1, 2, TREE), (span - 1, span, 1, TREE), (c.X, rack, 0, TREE)]
        grow(b, models, {0: good, 3: (nodes, edges)})
        assert device_graph(b, 3)[1][(span, m.sink)] == (0, 2, 0, 0)
        refresh(b, models, False)
        solve_and_check(b, models)
    finally:
        b.close()


def test_a_cell_with_two_sinks():
    """A cell given a second sink through ks_batch_apply_deltas refuses a new PU, naming the graph,
    and nothing changes anywhere; the same call without that cell's PU passes; the cell still accepts
    a machine with no PU."""
    b, models = make()
    try:
        m = models[2]
        extra = m.n0 + 1
        d = np.zeros(1, native.DELTA_DT)
        d["kind"], d["type"], d["id"] = native.KS_ADD_NODE, SINK, extra
        streams = [None] * 6
        streams[2] = d
        b.apply_deltas(streams)
        m.ntype.append(SINK)
        m.supply.append(0)
        m.alive.add(extra)
        compare(b, models)
        before = snapshot(b)
        per = {0: machine(models[0]), 2: m.machine(m.cell.RACK0, (extra + 1, extra + 2))}
        arg = [None] * 6
        for g, e in per.items():
            arg[g] = e
        refused(lambda: b.add_resources(arg), INVALID, "graph 2", f"PU {extra + 2}", "sink")
        assert snapshot(b) == before
        compare(b, models)
        grow(b, models, {0: per[0]})
        nodes, edges = per[2]
        st = grow(b, models, {2: (nodes[:1], [edges[0]] + edges[2:])})
        assert st["nodes"] == 1 and st["pus"] == 0 and st["arcs_skipped"] == 2 and st["records"] == 1
    finally:
        b.close()


@pytest.mark.parametrize("state", STATES)
def test_emptied_rack_gains_a_machine(state):
    """Every machine of one rack of cell 2 leaves (the rack stays, with no slot beneath it), then a
    machine joins beneath it with the chain listed, then the refresh: every capacity equals the model's."""
    b, models = make(state)
    try:
        m = models[2]
        c = m.cell
        ev = remove(b, models, {2: [c.MACH0 + k for k in range(c.M) if k % c.R == 0]}, state)
        relist(b, models, ev, state)
        assert c.RACK0 in m.alive and not [v for v, p in m.parent.items() if p == c.RACK0]
        stale = m.arcs.get((c.X, c.RACK0), (0, 0))[1]      # a rack with no slot beneath it keeps its arc's capacity
        grow(b, models, {2: machine(m, rack=c.RACK0, slots=4)})
        assert m.arcs[(c.X, c.RACK0)][1] == stale + 4
        st = refresh(b, models, state == "preemptive")
        assert st["cap_updates"] == (1 if stale else 0)
        assert device_graph(b, 2)[1][(c.X, c.RACK0)][1] == m.arcs[(c.X, c.RACK0)][1] == 4
        solve_and_check(b, models)
    finally:
        b.close()


# ------------------------------------------------------------------------ removal ---
@pytest.mark.parametrize("state", STATES)
def test_machines_and_a_rack_leave(state):
    """One machine of graphs 0, 3 and 5 and a whole rack of graph 4 leave in one call (pinned: the full
    machines and PUs beneath the roots are named too). removed per graph is ascending and the
    model's, the untouched graphs' parts are empty, the evictions are grouped by graph in task order
    and the evicted tasks read unbound."""
    b, models = make(state)
    try:
        per = {g: [models[g].cell.MACH0 + 1] for g in (0, 3, 5)}
        per[4] = [models[4].cell.RACK0 + 1]
        ev = remove(b, models, per, state)
        assert len(models[4].res_free) == 41
        if state != "cold":
            assert sum(len(v) for v in ev.values()) > 0
        relist(b, models, ev, state)
        solve_and_check(b, models)
    finally:
        b.close()


def test_probe_and_room():
    """A probe changes nothing and returns the counts; rcap one short is KS_E_INVALID with both counts
    written and nothing changed; with room the same call goes through."""
    b, models = make("preemptive")
    try:
        L, h = b._L, b._h
        per = {1: [models[1].cell.MACH0 + 3], 4: [models[4].cell.RACK0]}
        want = [models[g].subtree(r[0]) for g, r in per.items()]
        nrm = sum(len(w) for w in want)
        nev = sum(1 for g, w in zip(per, want) for p in models[g].bind.values() if p in w)
        assert nev > 0
        ls, keep = root_lists(per)
        before = snapshot(b)
        nr, ne = C.c_size_t(), C.c_size_t()
        assert L.ks_batch_remove_resources(h, 3, 6, ls, None, 0, C.byref(nr), None, None, 0, C.byref(ne), None) == 0
        assert (nr.value, ne.value) == (nrm, nev)
        assert snapshot(b) == before
        compare(b, models)
        rm = np.zeros(nrm, np.uint64)
        evd = np.zeros(nev, native.BATCH_DELTA_DT)
        off = np.zeros(7, np.uintp)
        nr, ne = C.c_size_t(), C.c_size_t()
        rc = L.ks_batch_remove_resources(h, 3, 6, ls, rm.ctypes.data, nrm - 1, C.byref(nr), off.ctypes.data,
                                         evd.ctypes.data, nev, C.byref(ne), None)
        assert rc == INVALID and (nr.value, ne.value) == (nrm, nev)
        assert snapshot(b) == before and not rm.any()
        rc = L.ks_batch_remove_resources(h, 3, 6, ls, rm.ctypes.data, nrm, C.byref(nr), off.ctypes.data,
                                         evd.ctypes.data, nev, C.byref(ne), None)
        assert rc == 0 and (nr.value, ne.value) == (nrm, nev)
        assert off.tolist() == [0, 0, len(want[0]), len(want[0]), len(want[0]), nrm, nrm]
        for g, w in zip(per, want):
            r, e, _ = models[g].remove(per[g], True, True)
            assert rm[int(off[g]):int(off[g + 1])].tolist() == r == sorted(w)
        compare(b, models)
    finally:
        b.close()


def test_bad_roots_and_flags():
    """A dead root and a task root are KS_E_INVALID naming graph and id, a root of span + 1 is
    KS_E_RANGE, KS_REMOVE_PREEMPTIVE without the caps flag, non-zero flags on the add call and a list
    count other than the loaded graphs are KS_E_INVALID; nothing changes on any graph. A root listed
    twice, or inside another root's subtree, is removed once."""
    b, models = make()
    try:
        m = models[3]
        c = m.cell
        span = m.n0 + SPARE
        before = snapshot(b)

        def one(root, **kw):
            arg = [None] * 6
            arg[0] = [models[0].cell.MACH0]              # a good list in the same call
            arg[3] = [root]
            return lambda: b.remove_resources(arg, **kw)

        dead, task = m.n0 + 5, m.tasks()[0]
        msg = refused(one(dead), INVALID, "graph 3", f"root {dead}")
        assert str(dead + sum(mm.n0 + SPARE for mm in models[:3])) not in msg
        refused(one(task), INVALID, "graph 3", f"root {task}")
        refused(one(span + 1), RANGE, "graph 3", str(span + 1))
        refused(one(0), RANGE, "graph 3")
        refused(one(c.MACH0, flags=native.KS_REMOVE_PREEMPTIVE), INVALID, "KS_REMOVE_RESOURCE_CAPS")
        L, h = b._L, b._h
        res = (native.KsBatchResList * 6)()
        nr, ne = C.c_size_t(), C.c_size_t()
        assert L.ks_batch_add_resources(h, 1, 6, res, None) == INVALID
        assert L.ks_batch_add_resources(h, 0, 5, res, None) == INVALID
        assert L.ks_batch_remove_resources(h, 1, 5, res, None, 0, C.byref(nr), None, None, 0, C.byref(ne), None) == INVALID
        assert snapshot(b) == before
        compare(b, models)
        mach = c.MACH0 + 1
        rm, ev, st = b.remove_resources([None, None, None, [mach, mach, c.PU0 + 1], None, None])
        wrm, wev, wst = m.remove([mach, mach, c.PU0 + 1], True, False)
        assert rm[3].tolist() == wrm == [mach, c.PU0 + 1] and st == wst and ev.size == 0
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_two_local_devices():
    """World 2 in one process (the test build with the in-process communicator; graph g on rank g mod
    2): both ranks remove and grow in one call each. Every device is probed before any changes, so
    rcap one short leaves both unions as they were; removed and the evictions come back in graph
    order although each rank holds every other graph."""
    if not os.path.exists(_build.variant_path(_build.FAKE_COMM_TAG)):
        pytest.fail("ksched_amd/libksmcmf_fakecomm.so is not built (__graft_entry__.build())")
    b, models = make("preemptive", devices=(0, 0), variant=_build.FAKE_COMM_TAG)
    try:
        per = {g: [models[g].cell.MACH0 + 1] for g in (0, 3, 5)}
        per[4] = [models[4].cell.RACK0 + 1]
        ls, keep = root_lists(per)
        before = snapshot(b)
        nr, ne = C.c_size_t(), C.c_size_t()
        rm = np.zeros(64, np.uint64)
        evd = np.zeros(2000, native.BATCH_DELTA_DT)
        rc = b._L.ks_batch_remove_resources(b._h, 3, 6, ls, rm.ctypes.data, 46, C.byref(nr), None, evd.ctypes.data, 2000,
                                            C.byref(ne), None)
        assert rc == INVALID and nr.value == 47 and ne.value > 0
        assert snapshot(b) == before
        refused(lambda: b.remove_resources([None, [models[1].tasks()[0]], None, None, [models[4].cell.MACH0], None],
                                           preemptive=True), INVALID, "graph 1", "root")
        assert snapshot(b) == before                  # rank 1 refused: rank 0's machine stays
        ev = remove(b, models, per, "preemptive")
        assert sum(len(v) for v in ev.values()) == ne.value
        grow(b, models, {0: machine(models[0]), 5: machine(models[5])})
        refresh(b, models, True)
        solve_and_check(b, models)
    finally:
        b.close()


# ------------------------------------------------------------------ rounds and solves ---
def test_warm_start_runs_the_touched_cells():
    """warm_start = 1: after a growth in two cells and a removal in a third, three cells run and the
    other three cells' gather rows are bit-identical."""
    b, models = make(warm_start=1)
    try:
        r0, pu0, cost0, flow0 = solve_and_check(b, models)
        assert r0.raw["cells_run"] == 6
        grow(b, models, {0: machine(models[0]), 5: machine(models[5])})
        refresh(b, models, False)
        remove(b, models, {3: [models[3].cell.MACH0]}, "cold")
        r1, pu1, cost1, flow1 = solve_and_check(b, models)
        assert r1.raw["cells_run"] == 3
        for g in (1, 2, 4):
            assert np.array_equal(pu1[g], pu0[g]) and cost1[g] == cost0[g] and flow1[g] == flow0[g], g
    finally:
        b.close()


@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
def test_three_full_rounds(preemptive):
    """commit → remove → complete → add resources → refresh → add → update → costs → solve, three
    times in both commit modes, with seeded random events per cell and another event count in every
    cell; after every call every graph, the statistics and the bindings equal the models', and every
    solve the oracle's. No graph of the batch is read back into a model."""
    b, models = make(warm_start=1)
    state = "preemptive" if preemptive else "pinned"
    rng = np.random.default_rng(77 + preemptive)
    seen = dict(removed=0, evicted=0, grown=0, reused=0)
    try:
        for rnd in range(3):
            solve_and_check(b, models)
            commit(b, models, preemptive)
            compare(b, models)
            # remove: 1 + g % 2 machines in about half of the cells
            per = {}
            for g, m in enumerate(models):
                ms = sorted(i for i in m.alive if m.ntype[i - 1] == MACHINE)
                if rng.random() < 0.6 and len(ms) > 6:
                    per[g] = sorted(int(x) for x in rng.choice(ms, 1 + g % 2, replace=False))
            evicted = remove(b, models, per, state) if per else {}
            returning = {g: set(t) for g, t in evicted.items()}
            seen["removed"] += sum(len(r) for r in per.values())
            seen["evicted"] += sum(len(t) for t in evicted.values())
            # complete: bound tasks and one waiting task per cell, in four of the six cells
            done, want = [None] * 6, []
            for g in (0, 1, 3, 4):
                m = models[g]
                waiting = [t for t in m.tasks(bound=False) if t not in returning.get(g, ())]
                done[g] = m.tasks(bound=True)[:max(1, m.cell.T0 // 20)] + waiting[:1]
            left, st = b.complete_tasks(done, resource_caps=True, preemptive=preemptive,
                                        unsched_ids=[m.aggs if done[g] is not None else None
                                                     for g, m in enumerate(models)])
            for g in (0, 1, 3, 4):
                wl, wst = models[g].complete(done[g], True, preemptive, models[g].aggs)
                assert left[g].tolist() == wl, (rnd, g)
                want.append(wst)
            assert st == sum_stats(want), (rnd, st, sum_stats(want))
            compare(b, models)
            # add resources: a machine in some cells (a removal's ids first), then the refresh
            per = {g: machine(m, rack=m.cell.RACK0 + int(rng.integers(m.cell.R)), slots=1 + g % 3)
                   for g, m in enumerate(models) if rng.random() < 0.6}
            if per:
                seen["grown"] += len(per)
                seen["reused"] += sum(1 for g, (nodes, _) in per.items() if nodes[0][0] <= models[g].n0)
                grow(b, models, per)
                refresh(b, models, preemptive)
            # add: freed ids first, then fresh ones, in five cells
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
            # update: pinned, the evicted tasks get their lists back (they had no arc left; after a
            # preemptive commit they kept theirs and wait like the rest); waiting tasks get new costs,
            # lose their last preference and gain another machine
            lists, ids, want = [None] * 6, [None] * 6, []
            for g, m in enumerate(models):
                back = [] if preemptive else sorted(t for t in returning.get(g, ()) if t in m.alive)
                ms = sorted(i for i in m.alive if m.ntype[i - 1] == MACHINE)
                tasks = [t for t in m.tasks(bound=False) if t not in back][2:8] if g in (1, 2, 5) else []
                ls = m.relist(back) if back else []
                for t in tasks:
                    held = [(hd, a[2]) for (s, hd), a in m.arcs.items() if s == t]
                    extra = ms[(t + rnd) % len(ms)]
                    ls.append([(hd, co + 3) for hd, co in held[:-1] if hd != extra] + [(extra, 21)])
                if back or tasks:
                    lists[g], ids[g] = (back + tasks, *offsets(ls)), m.aggs
                    want.append(m.refresh(back + tasks, ls, m.aggs, 11))
            st = b.update_tasks(lists, unsched_ids=ids, unsched_sink_cost=11)
            assert st == sum_stats(want), (rnd, st, sum_stats(want))
            compare(b, models)
            # costs: every aggregator of every graph ages
            changed = b.update_unsched_costs(10, mode=KS_COST_ADD, continuation=0 if preemptive else 3,
                                             unsched_ids=[m.aggs for m in models])
            assert changed == sum(m.age(10, KS_COST_ADD, 0 if preemptive else 3) for m in models)
            compare(b, models)
        solve_and_check(b, models)
        assert all(seen.values()), seen             # the rounds did remove, evict, grow and reuse a freed id
    finally:
        b.close()
