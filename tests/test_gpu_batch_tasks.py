"""GPU: the task side of a round on a batch — ks_batch_add_tasks, ks_batch_complete_tasks,
ks_batch_update_tasks, ks_batch_get_bindings and ks_batch_update_unsched_costs on six cells in one
union (one device, world 1, 256 reserved ids per graph). Every expected value comes from the host
restatements of the lone calls run per cell on the cell's own graph in its own ids
(tests/batch_tasks_ref.py over arrive_ref, complete_ref, refresh_ref); after every call each graph of
the batch (ks_batch_get_graph), the summed statistics and the bindings are compared with the models,
and the next solve with the CPU oracle per cell.

Cells 0 and 1 have the same parameters and different seeds, so their aggregators and sinks share
graph-local ids; the other four differ in size, so a wrong offset cannot cancel out."""
import numpy as np
import pytest

from batch_tasks_ref import KS_COST_ADD, CellModel, offsets, sum_stats
from ksched_amd import churn, native
from oracle import ko
from test_gpu_parity import check_mapping

pytestmark = pytest.mark.gpu

CELLS = [(300, 30, 3, 3, 1600), (300, 30, 3, 3, 1601), (500, 50, 5, 5, 1602), (200, 20, 2, 4, 1603),
         (1000, 100, 5, 10, 1604), (120, 12, 2, 2, 1605)]
SPARE = 256
MAXT = 1000 + SPARE
STATES = ["cold", "pinned", "preemptive"]
RANGE, INVALID = native.KS_E_RANGE, native.KS_E_INVALID


# ----------------------------------------------------------------------- helpers ---
def make(state="cold", **opts):
    """A batch of the six cells and their models: before any solve, after a solve plus
    commit_schedule, or after a solve plus commit_preemptive (the models take the device's deltas)."""
    cells = [churn.Cell(*p) for p in CELLS]
    b = native.Batch(devices=[0], **opts)
    b.reserve(SPARE)
    b.load([c.graph() for c in cells])
    models = [CellModel(c) for c in cells]
    if state != "cold":
        b.solve()
        commit(b, models, state == "preemptive")
        compare(b, models)
    return b, models


def commit(b, models, preemptive: bool):
    if preemptive:
        deltas, _ = b.commit_preemptive(continuation=0, preemption=150, resource_caps=True)
    else:
        deltas, _ = b.commit_schedule(continuation=3, resource_caps=True)
    per = [[] for _ in models]
    for ty, g, t, p in zip(deltas["type"].tolist(), deltas["graph"].tolist(), deltas["task"].tolist(),
                           deltas["pu"].tolist()):
        per[g].append((ty, t, p))
    for m, d in zip(models, per):
        if preemptive:
            m.commit_preemptive(d, 0, 150)
        else:
            m.commit_pinned({t: p for _, t, p in d}, 3)


def device_graph(b, g):
    nodes, a = b.get_graph(g)
    nd = {int(i): (int(t), int(e)) for i, t, e in zip(nodes["id"], nodes["type"], nodes["excess"])}
    arcs = {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
            for s, d, lo, c, co, ty in zip(a["src"], a["dst"], a["low"], a["cap"], a["cost"], a["type"])}
    return nd, arcs


def compare(b, models):
    """Every graph of the batch, untouched ones included, equals its model: nodes with type and supply,
    arcs with bounds, cost and type; and every live task's binding."""
    for g, m in enumerate(models):
        nd, arcs = device_graph(b, g)
        assert nd == m.nodes(), f"graph {g}: nodes"
        assert arcs == m.arcs, f"graph {g}: arcs"
        tasks = m.tasks()
        assert b.bindings(g, tasks).tolist() == [m.bind.get(t, 0) for t in tasks], f"graph {g}: bindings"


def snapshot(b, k=6):
    return [tuple(x.tobytes() for x in b.get_graph(g)) for g in range(k)]


def solve_and_check(b, models):
    """The next solve plus gather against the oracle on every model's graph, the mapping checked."""
    res = b.solve()[0]
    pu, cost, flow = b.gather(MAXT)
    for g, m in enumerate(models):
        graph = m.graph()
        st, c, f, fl = ko.cost_scaling(graph)
        assert st == 0
        vst, vcost, _ = ko.verify(graph, fl)
        assert vst == 0 and vcost == c
        assert (int(cost[g]), int(flow[g])) == (c, f), f"cell {g}"
        tasks = m.tasks()
        assert np.all(pu[g][len(tasks):] == 0)
        check_mapping(graph, {t: int(p) for t, p in zip(tasks, pu[g]) if p})
    return res, pu, cost, flow


def add(b, models, per_graph, unsched=False, sink_cost=0):
    """per_graph {g: (tasks, lists)} through ks_batch_add_tasks and the models; → the device's stats."""
    lists = [None] * len(models)
    ids = [None] * len(models) if unsched else None
    want = []
    for g, (tasks, ls) in per_graph.items():
        lists[g] = (tasks, *offsets(ls))
        if unsched:
            ids[g] = models[g].aggs
    st = b.add_tasks(lists, unsched_ids=ids, unsched_sink_cost=sink_cost)
    for g, (tasks, ls) in per_graph.items():
        want.append(models[g].arrive(tasks, ls, models[g].aggs if unsched else None, sink_cost))
    assert st == sum_stats(want), (st, sum_stats(want))
    return st


def refused(call, code, *words):
    with pytest.raises(native.KsError) as e:
        call()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


# ------------------------------------------------------------------------- cases ---
@pytest.mark.parametrize("state", STATES)
def test_three_graphs_in_one_wave(state):
    """Lists of 3, 2 and 4 tasks with 5, 3 and 1 arcs each for graphs 0, 3 and 5 (25 arcs: one wave
    holds arcs of three graphs): the first and the last graph are listed and unlisted graphs lie
    between listed ones. Cold, each listed graph also goes through the lone call on a lone context."""
    b, models = make(state)
    try:
        shape = {0: (3, 5), 3: (2, 3), 5: (4, 1)}
        per = {}
        for g, (k, narcs) in shape.items():
            tasks = models[g].new_ids(k)
            per[g] = (tasks, models[g].lists(tasks, narcs))
        lone = {}
        if state == "cold":
            for g, (tasks, ls) in per.items():
                with native.Context(0) as ctx:
                    ctx.load_graph(models[g].graph())
                    lone[g] = ctx.add_tasks(tasks, *offsets(ls), unsched_ids=models[g].aggs)
                    _, a = ctx.graph()
                    lone[g] = (lone[g], sorted(zip(a["src"].tolist(), a["dst"].tolist(), a["cap"].tolist(),
                                                   a["cost"].tolist())))
        st = add(b, models, per, unsched=True)
        assert st["tasks"] == 9 and st["arcs_added"] == 25
        compare(b, models)
        for g, (lst, arcs) in lone.items():
            _, a = b.get_graph(g)
            assert arcs == sorted(zip(a["src"].tolist(), a["dst"].tolist(), a["cap"].tolist(), a["cost"].tolist()))
        assert sum_stats(x for x, _ in lone.values()) == st or not lone
        solve_and_check(b, models)
    finally:
        b.close()


def test_same_id_aggregators_in_two_cells():
    """Cells 0 and 1 share every graph-local id: each gains units at the same aggregator id in one
    call, 3 and 5 of them, under the NULL rule. A merge across cells would give one record of 8."""
    b, models = make()
    try:
        assert models[0].aggs == models[1].aggs and models[0].sink == models[1].sink
        u = models[0].aggs[1]
        per = {}
        for g, k in ((0, 3), (1, 5)):
            tasks = models[g].new_ids(k)
            per[g] = (tasks, [[(u, 77 + i), (models[g].cell.X, 9)] for i in range(k)])
        caps = [models[g].arcs[(u, models[g].sink)][1] for g in (0, 1)]
        st = add(b, models, per)
        assert st["unsched_updates"] == 2 and st["unsched_added"] == 0
        compare(b, models)
        for g, k, c in ((0, 3, caps[0]), (1, 5, caps[1])):
            assert device_graph(b, g)[1][(u, models[g].sink)][1] == c + k
        solve_and_check(b, models)
    finally:
        b.close()


def drain(b, models, g, j):
    """Every task of job j of graph g completes: the aggregator's arc into the sink goes."""
    m = models[g]
    u = m.aggs[j]
    tasks = [t for t in m.tasks() if (t, u) in m.arcs]
    done = [None] * len(models)
    done[g] = tasks
    left, st = b.complete_tasks(done, resource_caps=False)
    wl, wst = m.complete(tasks, False, False)
    assert left[g].tolist() == wl and st == wst
    assert (u, m.sink) not in m.arcs
    return u


def test_drained_aggregator_in_the_last_cell_add():
    """The last cell's aggregator has lost its arc into the sink; arrivals with the ids passed
    explicitly re-create it as an ADD_ARC that ends at THAT cell's sink with unsched_sink_cost.
    Cell 0 gains in the same call on an arc it still holds."""
    b, models = make()
    try:
        u = drain(b, models, 5, 0)
        compare(b, models)
        per = {}
        for g, agg in ((0, models[0].aggs[0]), (5, u)):
            tasks = models[g].new_ids(2)
            per[g] = (tasks, [[(agg, 60), (models[g].cell.X, 8)] for _ in tasks])
        st = add(b, models, per, unsched=True, sink_cost=4321)
        assert st["unsched_added"] == 1 and st["unsched_updates"] == 1
        assert device_graph(b, 5)[1][(u, models[5].sink)] == (0, 2, 4321, 0)
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_drained_aggregator_in_the_last_cell_update():
    """The same through ks_batch_update_tasks, in the shape of a task evicted after a pinned commit: a
    live task without its arc into the aggregator, whose arc into the sink is gone; the refresh lists
    the aggregator, the unit comes back and the re-created arc ends at the last cell's own sink."""
    b, models = make()
    try:
        m = models[5]
        u = m.aggs[0]
        mine = [t for t in m.tasks() if (t, u) in m.arcs]
        keep = mine[0]
        done = [None] * 6
        done[5] = mine[1:]
        b.complete_tasks(done, resource_caps=False)
        m.complete(mine[1:], False, False)
        # the eviction's shape: the task's arc into the aggregator and the aggregator's into the sink go
        d = np.zeros(2, native.DELTA_DT)
        d["kind"] = native.KS_UPDATE_ARC
        d["src"], d["dst"] = [keep, u], [u, m.sink]
        streams = [None] * 6
        streams[5] = d
        b.apply_deltas(streams)
        del m.arcs[(keep, u)], m.arcs[(u, m.sink)]
        compare(b, models)
        lst = [[(u, 55)] + [(h, a[2] + 1) for (s, h), a in m.arcs.items() if s == keep]]
        lists = [None] * 6
        lists[5] = ([keep], *offsets(lst))
        ids = [None] * 6
        ids[5] = m.aggs
        st = b.update_tasks(lists, unsched_ids=ids, unsched_sink_cost=999)
        assert st == m.refresh([keep], lst, m.aggs, 999)
        assert st["unsched_added"] == 1 and st["arcs_added"] == 1
        assert device_graph(b, 5)[1][(u, m.sink)] == (0, 1, 999, 0)
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_large_cell_and_a_single_task():
    """Cell 4 receives 300 tasks × 5 arcs (1,500 arcs: six workgroups of the head pass; 100 ids freed
    by completions come back first) while cell 2 receives one task in the same call."""
    b, models = make()
    try:
        done = [None] * 6
        done[4] = models[4].tasks()[:100]
        left, st = b.complete_tasks(done, resource_caps=False)
        wl, wst = models[4].complete(done[4], False, False)
        assert left[4].tolist() == wl and st == wst and left[0] is None
        per = {}
        for g, k in ((2, 1), (4, 300)):
            tasks = models[g].new_ids(k)
            per[g] = (tasks, models[g].lists(tasks, 5))
        assert per[4][0][:100] == done[4] and per[4][0][-1] == models[4].n0 + 200
        st = add(b, models, per)
        assert st["tasks"] == 301 and st["arcs_added"] == 1505
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_id_bounds_and_refusals():
    """A task whose id is span is legal; span + 1 is KS_E_RANGE, as is a head of span + 1; a dead
    head inside the range is KS_E_INVALID. Every message names the graph and the graph-local id,
    and every graph is byte-identical after a refusal."""
    b, models = make()
    try:
        m = models[3]
        span = m.n0 + SPARE
        x, u = m.cell.X, m.aggs[0]

        def one(g, task, heads):
            lists = [None] * 6
            lists[0] = ([models[0].n0 + 1], *offsets([[(models[0].aggs[0], 5)]]))   # a good list in the same call
            lists[g] = ([task], *offsets([[(h, 5) for h in heads]]))
            return lambda: b.add_tasks(lists)

        before = snapshot(b)
        refused(one(3, span + 1, [u, x]), RANGE, "graph 3", str(span + 1))
        assert snapshot(b) == before
        refused(one(3, span, [u, span + 1]), RANGE, "graph 3", str(span + 1), f"task {span}")
        assert snapshot(b) == before
        refused(one(3, span, [u, 0]), RANGE, "graph 3")
        assert snapshot(b) == before
        dead = m.n0 + 5                                 # inside the range, never added
        msg = refused(one(3, span, [u, dead]), INVALID, "graph 3", f"head {dead}", f"task {span}")
        assert str(dead + sum(mm.n0 + SPARE for mm in models[:3])) not in msg     # no union id
        assert snapshot(b) == before
        # the same bounds through the refresh and the completion
        t = m.tasks()[0]
        lists = [None] * 6
        lists[3] = ([t], *offsets([[(u, 5), (span + 1, 5)]]))
        refused(lambda: b.update_tasks(lists), RANGE, "graph 3", str(span + 1))
        done = [None] * 6
        done[3] = [span + 1]
        refused(lambda: b.complete_tasks(done, resource_caps=False), RANGE, "graph 3", str(span + 1))
        done[3] = [dead]
        refused(lambda: b.complete_tasks(done, resource_caps=False), INVALID, "graph 3", f"task {dead}")
        refused(lambda: b.bindings(3, [span + 1]), RANGE, "graph 3")
        assert snapshot(b) == before
        compare(b, models)
        # the legal one: id == span
        lists = [None] * 6
        lst = [[(u, 5), (x, 6)]]
        lists[3] = ([span], *offsets(lst))
        st = b.add_tasks(lists)
        assert st == m.arrive([span], lst)
        compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


@pytest.mark.parametrize("state", STATES)
def test_completions(state):
    """left is graph-local, a duplicate gets the same value twice, and the capacity refresh runs in
    the mode of the commit before it (cold and pinned: slots − running; preemptive: slots), with and
    without KS_COMPLETE_RESOURCE_CAPS, on the union's six sinks."""
    b, models = make(state)
    try:
        pre = state == "preemptive"
        for caps in (True, False):
            done = [None] * 6
            want_left, want_st = {}, []
            for g in (1, 2, 5):
                m = models[g]
                bound, waiting = m.tasks(bound=True), m.tasks(bound=False)
                pick = bound[:4] + waiting[:3]
                done[g] = pick + pick[:1]                      # the first id twice
                wl, wst = m.complete(done[g], caps, pre and caps)
                want_left[g] = wl
                want_st.append(wst)
            left, st = b.complete_tasks(done, resource_caps=caps, preemptive=pre and caps)
            for g in range(6):
                if g in want_left:
                    assert left[g].tolist() == want_left[g], f"graph {g}"
                    assert left[g][0] == left[g][-1]
                    assert all(p == 0 or models[g].cell.PU0 <= p < models[g].cell.PU0 + models[g].cell.M
                               for p in left[g].tolist())
                else:
                    assert left[g] is None
            assert st == sum_stats(want_st), (st, sum_stats(want_st))
            if state != "cold":
                assert st["bound"] > 0
            compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()


def test_auto_sink_follows_the_touched_cells_only():
    """After arrivals in cells 1 and 4 only, those two sinks' supplies are −(their live tasks) and no
    other cell's changed."""
    b, models = make()
    try:
        sinks = lambda: [device_graph(b, g)[0][models[g].sink][1] for g in range(6)]
        before = sinks()
        per = {}
        for g, k in ((1, 4), (4, 6)):
            tasks = models[g].new_ids(k)
            per[g] = (tasks, models[g].lists(tasks, 2))
        add(b, models, per)
        after = sinks()
        for g in range(6):
            assert after[g] == before[g] - {1: 4, 4: 6}.get(g, 0), g
            assert after[g] == -len(models[g].tasks())
        compare(b, models)
    finally:
        b.close()


def test_warm_start_runs_the_touched_cells():
    """warm_start = 1: lists for 2 of the 6 cells; the untouched cells' gather rows are bit-identical,
    and when no rebuild intervened only the two touched cells run."""
    b, models = make(warm_start=1)
    try:
        r0, pu0, cost0, flow0 = solve_and_check(b, models)
        assert r0.raw["cells_run"] == 6
        per = {}
        for g in (1, 4):
            tasks = models[g].new_ids(5)
            per[g] = (tasks, models[g].lists(tasks, 5))
        add(b, models, per)
        compare(b, models)
        r1, pu1, cost1, flow1 = solve_and_check(b, models)
        for g in (0, 2, 3, 5):
            assert np.array_equal(pu1[g], pu0[g]) and cost1[g] == cost0[g] and flow1[g] == flow0[g], g
        if not r1.raw["rebuilt"]:
            assert r1.raw["cells_run"] == 2
    finally:
        b.close()


@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
def test_three_full_rounds(preemptive):
    """commit → complete → add → update → update_unsched_costs → solve, three times, in both commit
    modes; after every call every graph, the statistics and the bindings equal the models', and
    every solve the oracle's."""
    b, models = make(warm_start=1)
    try:
        for rnd in range(3):
            solve_and_check(b, models)
            commit(b, models, preemptive)
            compare(b, models)
            # complete: bound tasks and one waiting task per cell, in four of the six cells
            done, want = [None] * 6, []
            for g in (0, 1, 3, 4):
                m = models[g]
                done[g] = m.tasks(bound=True)[:max(1, m.cell.T0 // 20)] + m.tasks(bound=False)[:1]
            left, st = b.complete_tasks(done, resource_caps=True, preemptive=preemptive,
                                        unsched_ids=[m.aggs if done[g] is not None else None
                                                     for g, m in enumerate(models)])
            for g in (0, 1, 3, 4):
                wl, wst = models[g].complete(done[g], True, preemptive, models[g].aggs)
                assert left[g].tolist() == wl, (rnd, g)
                want.append(wst)
            assert st == sum_stats(want), (rnd, st, sum_stats(want))
            compare(b, models)
            # add: freed ids first, then fresh ones, in five cells
            per = {}
            for g in (0, 1, 2, 4, 5):
                tasks = models[g].new_ids(models[g].cell.T0 // 20 + 2)
                per[g] = (tasks, models[g].lists(tasks, 5, base_cost=30 + rnd))
            add(b, models, per, unsched=True, sink_cost=11)
            compare(b, models)
            # update: waiting tasks get new costs, lose their last preference and gain another machine
            lists, ids, want = [None] * 6, [None] * 6, []
            for g in (1, 2, 5):
                m = models[g]
                tasks = m.tasks(bound=False)[2:8]
                ls = []
                for t in tasks:
                    held = [(h, a[2]) for (s, h), a in m.arcs.items() if s == t]
                    extra = m.cell.MACH0 + ((t + rnd) % m.cell.M)
                    new = [(h, c + 3) for h, c in held[:-1] if h != extra]
                    ls.append(new + [(extra, 21)])
                lists[g], ids[g] = (tasks, *offsets(ls)), m.aggs
                want.append(m.refresh(tasks, ls, m.aggs, 11))
            st = b.update_tasks(lists, unsched_ids=ids, unsched_sink_cost=11)
            assert st == sum_stats(want), (rnd, st, sum_stats(want))
            compare(b, models)
            # costs: every aggregator of every graph ages
            changed = b.update_unsched_costs(10, mode=KS_COST_ADD, continuation=0 if preemptive else 3,
                                             unsched_ids=[m.aggs for m in models])
            assert changed == sum(m.age(10, KS_COST_ADD, 0 if preemptive else 3) for m in models)
            compare(b, models)
        solve_and_check(b, models)
    finally:
        b.close()
