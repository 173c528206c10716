"""GPU: scheduling rounds on a batch — ks_batch_reserve, ks_batch_apply_deltas,
ks_batch_get_graph, the re-solve of the changed cells only (ks_result.cells_run) and
both commits on a union — against the CPU oracle on every cell's own full graph
(churn.Cell.graph()), never against another run of the library.

The six cells have deliberately different sizes, so a wrong node or task offset cannot
cancel out, and every batch reserves 256 ids per graph."""
import os

import numpy as np
import pytest

from commit_ref import commit_reference
from graphs import same_graph
from ksched_amd import _build, churn, gen, native
from oracle import ko
from preempt_ref import preempt_reference, table_graph
from test_gpu_parity import check_mapping

pytestmark = pytest.mark.gpu

CELLS = [(2000, 200, 10, 20, 1500), (1000, 100, 5, 10, 1501), (500, 50, 5, 5, 1502), (2000, 200, 10, 20, 1503),
         (300, 30, 3, 3, 1504), (1000, 100, 5, 10, 1505)]
SPARE = 256
MAXT = 2000 + SPARE          # row length of the gathers: no cell ever has more live tasks


def make_cells(params=CELLS, **kw):
    return [churn.Cell(*p, **kw) for p in params]


def make_batch(cells, spare=SPARE, **opts):
    b = native.Batch(devices=[0], **opts)
    b.reserve(spare)
    b.load([c.graph() for c in cells])
    return b


class GraphOf:
    """graph g of a batch with the .graph() of a Context (for graphs.same_graph)."""

    def __init__(self, b, g):
        self.b, self.g = b, g

    def graph(self):
        return self.b.get_graph(self.g)


def table(b, g) -> dict:
    """{(src, dst): (low, cap, cost, type)} of graph g as the device holds it."""
    _, a = b.get_graph(g)
    return {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
            for s, d, lo, c, co, ty in zip(a["src"], a["dst"], a["low"], a["cap"], a["cost"], a["type"])}


def snapshot(b, k):
    return [tuple(x.tobytes() for x in b.get_graph(g)) for g in range(k)]


def mapping_of(graph, row) -> dict:
    """A gather row (the i-th live task in id order → its PU, 0: none) as {task: pu}."""
    tasks = np.nonzero(graph.ntype == 1)[0] + 1
    assert np.all(row[tasks.shape[0]:] == 0)
    return {int(t): int(p) for t, p in zip(tasks, row) if p}


def oracle(graph):
    """(cost, flow) of the CPU cost-scaling oracle, its own flow accepted by its verifier."""
    st, cost, flow, fl = ko.cost_scaling(graph)
    assert st == 0
    vst, vcost, _ = ko.verify(graph, fl)
    assert vst == 0 and vcost == cost
    return cost, flow


def check_cells(b, cells, which=None):
    """Gathered cost, flow and mapping of the cells (all, or `which`) against the oracle."""
    pu, cost, flow = b.gather(MAXT)
    for g, cell in enumerate(cells):
        if which is not None and g not in which:
            continue
        graph = cell.graph()
        assert (int(cost[g]), int(flow[g])) == oracle(graph), f"cell {g}"
        mp = mapping_of(graph, pu[g])
        assert mp
        check_mapping(graph, mp)
    return pu, cost, flow


def step_all(b, cells, pu, which=None, frac=20, extra=10):
    """One round's streams: gather rows → each cell's step (5 % completions, 5 % + 10
    arrivals), for all cells or only `which` (the others get no stream)."""
    streams = []
    for g, cell in enumerate(cells):
        if which is not None and g not in which:
            streams.append(None)
            continue
        mp = mapping_of(cell.graph(), pu[g])
        streams.append(cell.step(mp, done=cell.T0 // frac, arrive=cell.T0 // frac + extra))
    return streams


def run_rounds(b, cells, rounds, warm, solver=1):
    res = b.solve()[0]
    assert res.raw["solver"] == solver
    pu, _, _ = check_cells(b, cells)
    for rnd in range(rounds):
        b.apply_deltas(step_all(b, cells, pu))
        res = b.solve()[0]
        pu, cost, _ = check_cells(b, cells)
        for g, cell in enumerate(cells):
            same_graph(GraphOf(b, g), cell.graph())
        assert res.raw["solver"] == solver, f"round {rnd + 1}"
        assert res.raw["cells"] == (len(cells) if solver else 0)
        assert res.raw["warm_started"] == (1 if warm else 0)
        assert int(res.cost) == int(cost.sum())
    return res


@pytest.mark.parametrize("warm", [0, 1], ids=["cold", "warm"])
def test_three_rounds_all_cells_changing(warm):
    """1. Every cell goes through three rounds of pins, completions, arrivals (10 new
    ids per round: 30 of the 256 reserved), ageing and capacity refresh; after each
    apply + solve every cell's gathered cost, flow and mapping equal the oracle on its
    full graph and ks_batch_get_graph equals that graph."""
    cells = make_cells()
    b = make_batch(cells, warm_start=warm)
    try:
        res = run_rounds(b, cells, 3, warm)
        assert res.raw["cells_run"] == 6          # every cell changed in every round
    finally:
        b.close()


@pytest.mark.parametrize("order", [list(range(6)), [0, 1, 2, 4, 5, 3]], ids=["issue-order", "largest-last"])
def test_cell_solver_kept_after_deltas(order):
    """2. The partition ends at its last offset. Once deltas arrive the store keeps
    max(64, slots/16) spare slots past the union (about 600 here); counted into the last
    cell they push it over ks_opts.cell_nodes and the whole union leaves the cell solver.
    cell_nodes sits just above the largest range (2432 + 256 ids). With the largest cell
    last, the old boundary (last cell = its range + the spare slots ≈ 3,300) fails this."""
    cells = make_cells([CELLS[i] for i in order])
    largest = max(c.graph().n for c in cells) + SPARE
    assert largest == 2432 + 256
    b = make_batch(cells, warm_start=1, cell_nodes=largest + 8)
    try:
        res = run_rounds(b, cells, 1, 1)
        assert res.raw["solver"] == 1 and res.raw["cells"] == 6
    finally:
        b.close()


@pytest.mark.parametrize("warm", [1, 0], ids=["warm", "cold"])
def test_only_dirty_cells_run(warm):
    """3. After a solve, streams for cells 1 and 4 only: a warm batch launches those two
    cells, the rows of the others are bit-identical to the previous gather, and 1 and 4
    equal the oracle; an empty apply then launches nothing and cost and flow stay. A cold
    batch (warm_start 0) runs all six cells every time."""
    cells = make_cells()
    b = make_batch(cells, warm_start=warm)
    try:
        r0 = b.solve()[0]
        assert r0.raw["cells_run"] == 6 and r0.raw["cells"] == 6
        pu0, cost0, flow0 = check_cells(b, cells)
        b.apply_deltas(step_all(b, cells, pu0, which={1, 4}))
        r1 = b.solve()[0]
        assert r1.raw["solver"] == 1 and r1.raw["cells"] == 6
        assert r1.raw["cells_run"] == (2 if warm else 6), r1.raw["rebuilt"]
        pu1, cost1, flow1 = check_cells(b, cells)             # every cell, the changed two included
        if warm:
            for g in (0, 2, 3, 5):
                assert np.array_equal(pu1[g], pu0[g]) and cost1[g] == cost0[g] and flow1[g] == flow0[g], g
        b.apply_deltas([None] * 6)
        r2 = b.solve()[0]
        assert r2.raw["cells_run"] == (0 if warm else 6)
        assert (r2.cost, r2.flow) == (r1.cost, r1.flow)
        pu2, cost2, flow2 = b.gather(MAXT)
        assert np.array_equal(cost2, cost1) and np.array_equal(flow2, flow1)
        if warm:
            assert np.array_equal(pu2, pu1)
    finally:
        b.close()


def refused(b, streams):
    with pytest.raises(native.KsError) as e:
        b.apply_deltas(streams)
    assert e.value.code == native.KS_E_RANGE, e.value
    return str(e.value)


def test_refusals_leave_everything_as_it_was():
    """4. A record whose id leaves its graph's range is KS_E_RANGE: an arc into the next
    cell's ids, a new node beyond the reserved ids, and a good stream in the same call as
    a bad one — nothing changes, and a solve returns the previous costs."""
    cells = make_cells()
    b = make_batch(cells)
    try:
        b.solve()
        pu, cost, _ = b.gather(MAXT)
        before = snapshot(b, 6)
        n2 = cells[2].graph().n
        bad = np.zeros(1, native.DELTA_DT)
        bad["kind"], bad["src"], bad["dst"], bad["cap"] = native.KS_ADD_ARC, cells[2].TASK0, n2 + SPARE + 1, 1
        msg = refused(b, [None, None, bad, None, None, None])
        assert "graph 2" in msg and str(n2 + SPARE + 1) in msg
        assert snapshot(b, 6) == before
        # a valid stream for cell 0 together with a bad one for cell 3: cell 0 must not change
        good = churn.Cell(*CELLS[0]).step(mapping_of(cells[0].graph(), pu[0]), done=100, arrive=110)
        bad3 = bad.copy()
        bad3["src"], bad3["dst"] = 0, 5
        msg = refused(b, [good, None, None, bad3, None, None])
        assert "graph 3" in msg
        assert snapshot(b, 6) == before
        b.solve()
        _, cost2, _ = b.gather(MAXT)
        assert cost2.tolist() == cost.tolist()
    finally:
        b.close()
    # 16 reserved ids, 100 arrivals without a completion: the 17th new id is refused
    cells = make_cells()
    b = make_batch(cells, spare=16)
    try:
        b.solve()
        _, cost, _ = b.gather(MAXT)
        before = snapshot(b, 6)
        n1 = cells[1].graph().n
        msg = refused(b, [None, cells[1].step({}, done=0, arrive=100), None, None, None, None])
        assert "graph 1" in msg and str(n1 + 17) in msg
        assert snapshot(b, 6) == before
        b.solve()
        _, cost2, _ = b.gather(MAXT)
        assert cost2.tolist() == cost.tolist()
    finally:
        b.close()


def with_second_sink(g, demand=0):
    """g plus one isolated sink that takes `demand` units of the first sink's demand: a
    graph with two sinks (node 1 is the first)."""
    supply = np.append(g.supply, -demand)
    supply[0] += demand
    return gen.Graph(np.append(g.ntype, 3).astype(np.int32), supply, g.src, g.dst, g.low, g.cap, g.cost,
                     g.arc_types())


def test_per_graph_auto_sink():
    """5. After a round with arrivals but no completions every one-sink graph's sink
    supply in ks_batch_get_graph is −(its live tasks); a graph loaded with two sinks is
    left alone."""
    cells = make_cells(CELLS[:3])
    b = native.Batch(devices=[0])
    b.reserve(SPARE)
    graphs = [c.graph() for c in cells]
    graphs[1] = with_second_sink(graphs[1], demand=7)
    b.load(graphs)
    try:
        # (graph 1's stream only ages its tasks: its second sink sits on the next task id)
        arrive = [10, 0, 20]
        b.apply_deltas([c.step({}, done=0, arrive=a) for c, a in zip(cells, arrive)])
        for g, cell in enumerate(cells):
            nodes, _ = b.get_graph(g)
            sinks = nodes[nodes["type"] == 3]
            tasks = int((nodes["type"] == 1).sum())
            assert tasks == cell.T0 + arrive[g]
            if g == 1:
                assert sinks["excess"].tolist() == [-(cell.T0 - 7), -7]       # as loaded, not −tasks
            else:
                assert sinks["excess"].tolist() == [-tasks]
    finally:
        b.close()


def test_engine_path_rounds():
    """6. ks_opts.cell_nodes −1: the same rounds on the multi-kernel engine."""
    cells = make_cells()
    b = make_batch(cells, cell_nodes=-1)
    try:
        res = run_rounds(b, cells, 2, 0, solver=0)
        assert res.raw["solver"] == 0 and res.raw["cells_run"] == 0
    finally:
        b.close()


def split_deltas(deltas, cells):
    """BATCH_DELTA_DT records → per graph [(type, task, pu)], checking the grouping and
    that the ids are graph-local task ids."""
    assert deltas["graph"].tolist() == sorted(deltas["graph"].tolist())
    out = [[] for _ in cells]
    for ty, g, t, p in zip(deltas["type"].tolist(), deltas["graph"].tolist(), deltas["task"].tolist(),
                           deltas["pu"].tolist()):
        cell = cells[g]
        assert cell.TASK0 <= t < cell.TASK0 + cell.n_slots, (g, t)
        assert cell.PU0 <= p < cell.PU0 + cell.M, (g, p)
        out[g].append((ty, t, p))
    return out


def arrivals_with_room(b, g, cell, k):
    """k new tasks for graph g (arcs into their job's aggregator and the cluster node) and
    room for them on the first k PUs."""
    t = table(b, g)
    cap = lambda s, d: t.get((s, d), (0, 0, 0, 0))[1]
    recs = []
    for i in range(k):
        tid = cell.TASK0 + cell.n_slots + i
        recs.append((native.KS_ADD_NODE, 1, tid, 0, 0, 0, 0, 0, 0, 1))
        recs.append((native.KS_ADD_ARC, 0, 0, tid, cell.U0, 0, 1, 500, 0, 0))
        recs.append((native.KS_ADD_ARC, 0, 0, tid, cell.X, 0, 1, 7, 0, 0))
    # one more slot on each of the first k PUs (a PU's segment has room for its slots'
    # running arcs and two more), opened along X → rack → machine → PU → sink
    add = {(cell.U0, cell.SINK): k}
    for m in range(k):
        rack = cell.RACK0 + int(cell.rack_of[m])
        for s_, d_ in ((cell.X, rack), (rack, cell.MACH0 + m), (cell.MACH0 + m, cell.PU0 + m),
                       (cell.PU0 + m, cell.SINK)):
            add[(s_, d_)] = add.get((s_, d_), 0) + 1
    for (s_, d_), extra in add.items():
        recs.append((native.KS_ADD_ARC, 0, 0, s_, d_, 0, cap(s_, d_) + extra, 0, 0, 0))
    d = np.zeros(len(recs), native.DELTA_DT)
    for name, col in zip(native.DELTA_DT.names, zip(*recs)):
        d[name] = np.asarray(col, dtype=native.DELTA_DT[name])
    return d


def test_commit_schedule_on_a_batch():
    """7a. ks_batch_commit_schedule with the capacity refresh: every graph equals the
    pin rule (tests/commit_ref.py) arc for arc, types included; the deltas carry their
    graph and graph-local ids; bindings are set (the next commit places nothing twice);
    the next solve equals the oracle on the committed graph. Then only cells 1 and 4 get
    arrivals: the commit's generated records mark exactly those cells on the device."""
    cells = make_cells()
    b = make_batch(cells, warm_start=1)
    try:
        b.solve()
        pu, _, _ = b.gather(MAXT)
        before = [c.graph() for c in cells]
        deltas, st = b.commit_schedule(continuation=3, resource_caps=True)
        per = split_deltas(deltas, cells)
        committed = []
        for g, cell in enumerate(cells):
            placed = {t: p for _, t, p in per[g]}
            assert all(ty == native.KS_DELTA_PLACE for ty, _, _ in per[g])
            assert placed == mapping_of(before[g], pu[g])
            assert [t for _, t, _ in per[g]] == sorted(placed)
            want = commit_reference(before[g], placed, 3, True)
            assert table(b, g) == want, f"graph {g}"
            committed.append(table_graph(before[g].ntype, before[g].supply, want))
        assert st["placed"] == deltas.shape[0] == sum(len(p) for p in per)
        r = b.solve()[0]
        assert r.raw["cells_run"] == 6
        _, cost, flow = b.gather(MAXT)
        for g in range(6):
            assert (int(cost[g]), int(flow[g])) == oracle(committed[g]), f"graph {g}"
        again, _ = b.commit_schedule(continuation=3, resource_caps=True)
        first = set(zip(deltas["graph"].tolist(), deltas["task"].tolist()))
        assert not first & set(zip(again["graph"].tolist(), again["task"].tolist()))   # placed tasks are bound
        b.solve()
        # arrivals in cells 1 and 4 only: the solve runs those two, and so does the one
        # after the commit whose records exist only on the device
        streams = [None] * 6
        for g in (1, 4):
            streams[g] = arrivals_with_room(b, g, cells[g], 5)
        b.apply_deltas(streams)
        assert b.solve()[0].raw["cells_run"] == 2
        deltas, st = b.commit_schedule(continuation=3, resource_caps=True)
        assert sorted(set(deltas["graph"].tolist())) == [1, 4] and st["records"] > 0
        r = b.solve()[0]
        assert r.raw["cells_run"] == 2, r.raw["rebuilt"]
    finally:
        b.close()


def test_commit_preemptive_on_a_batch():
    """7b. ks_batch_commit_preemptive on two rounds of preemptive cells against the rule
    (tests/preempt_ref.py), graph by graph, from the device's own deltas."""
    params = [CELLS[1], CELLS[2], CELLS[4]]
    cells = make_cells(params, preemption=True, preemption_cost=150)
    b = make_batch(cells)
    bindings = [{} for _ in cells]
    try:
        kinds = set()
        for rnd in range(2):
            b.solve()
            pu, cost, flow = b.gather(MAXT)
            graphs = [c.graph() for c in cells]
            for g in range(len(cells)):
                assert (int(cost[g]), int(flow[g])) == oracle(graphs[g]), (rnd, g)
            before = [table_graph(graphs[g].ntype, graphs[g].supply, table(b, g)) for g in range(len(cells))]
            deltas, st = b.commit_preemptive(continuation=0, preemption=150, resource_caps=True)
            per = split_deltas(deltas, cells)
            records = 0
            for g, cell in enumerate(cells):
                want, bindings[g], wst = preempt_reference(before[g], per[g], bindings[g], 0, 150, True)
                assert table(b, g) == want, (rnd, g)
                records += wst["records"]
                kinds |= {ty for ty, _, _ in per[g]}
                # the cell's own state follows the commit, then a churn round without a mapping
                cell.step(mapping_of(graphs[g], pu[g]), 0, 0, age_cost=0, seed=100 + rnd)
                same_graph(GraphOf(b, g), cell.graph())
            assert st["records"] == records
            b.apply_deltas([c.step(None, c.T0 // 20, c.T0 // 20 + 5, seed=200 + rnd) for c in cells])
        assert native.KS_DELTA_PLACE in kinds
        b.solve()
        _, cost, flow = b.gather(MAXT)
        for g, cell in enumerate(cells):
            assert (int(cost[g]), int(flow[g])) == oracle(cell.graph()), g
    finally:
        b.close()


def test_one_sink_commit_is_unchanged():
    """7c. A lone context (one sink, no partition) through ks_topology_stats and
    ks_commit_schedule with the capacity refresh still equals the rule: the sinks'
    seeding kernel is the partition's path only."""
    cell = churn.Cell(*CELLS[0])
    g = cell.graph()
    with native.Context(0) as ctx:
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        slots, running = ctx.topology_stats(1)
        assert int(slots[cell.X - 1]) == cell.M and int(running.sum()) == 0
        deltas, _ = ctx.commit_schedule(continuation=3, resource_caps=True)
        assert dict(zip(deltas["task"].tolist(), deltas["pu"].tolist())) == mp
        _, a = ctx.graph()
        got = {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
               for s, d, lo, c, co, ty in zip(a["src"], a["dst"], a["low"], a["cap"], a["cost"], a["type"])}
        assert got == commit_reference(g, mp, 3, True)
    # several sinks without a partition: the refresh still refuses
    with native.Context(0) as ctx:
        ctx.load_graph(with_second_sink(g))
        ctx.solve()
        with pytest.raises(native.KsError) as e:
            ctx.commit_schedule(continuation=3, resource_caps=True)
        assert e.value.code == native.KS_E_INVALID and "one sink" in str(e.value)


def test_world2_round_on_one_gpu():
    """8. Four cells over two in-process ranks (the test build with the in-process
    communicator): one round applied, solved and gathered; rank 0's rows equal the
    oracle for all four graphs."""
    fake = _build.FAKE_COMM_TAG
    if not os.path.exists(_build.variant_path(fake)):
        pytest.fail("ksched_amd/libksmcmf_fakecomm.so is not built (__graft_entry__.build())")
    cells = make_cells(CELLS[:4])
    b = native.Batch(devices=[0, 0], variant=fake, warm_start=1)
    b.reserve(SPARE)
    b.load([c.graph() for c in cells])
    try:
        res = b.solve()
        assert [r.raw["cells"] for r in res] == [2, 2]
        pu, _, _ = check_cells(b, cells)
        b.apply_deltas(step_all(b, cells, pu))
        res = b.solve()
        assert all(r.raw["solver"] == 1 and r.raw["cells_run"] == 2 for r in res)
        check_cells(b, cells)
        for g, cell in enumerate(cells):
            same_graph(GraphOf(b, g), cell.graph())
    finally:
        b.close()
