"""GPU: ks_commit_schedule — the pin of every placed task, the unscheduled
aggregators' capacities and the resource arcs' capacities, generated and applied
on the device-resident graph — against the rule restated on the host
(tests/commit_ref.py) and against the host path it replaces (churn.Cell's own
records through ks_apply_deltas)."""
import ctypes as C

import numpy as np
import pytest

from commit_ref import arc_table, commit_reference
from graphs import graph_from_lists, same_graph
from ksched_amd import churn, gen, native
from oracle import ko

pytestmark = pytest.mark.gpu

PLACE = native.KS_DELTA_PLACE


def dev_table(ctx) -> dict:
    """{(src, dst): (low, cap, cost, type)} of the device-resident graph."""
    _, a = ctx.graph()
    return {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
            for s, d, lo, c, co, ty in zip(a["src"], a["dst"], a["low"], a["cap"], a["cost"], a["type"])}


def live(table: dict) -> dict:
    return {k: a for k, a in table.items() if a[1] > 0}


def raises_code(code, fn, *a, **kw):
    with pytest.raises(native.KsError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def test_known_answer_config1():
    """ksched's own topology, 10 machines × 1000 slots, 100 pods: the checks hold for
    every optimal placement."""
    g = gen.trivial(10, 1000, 100)
    SINK, COORD, U, EC = 1, 2, 23, 24
    machines = [3 + 2 * k for k in range(10)]
    with native.Context(0) as ctx:
        ctx.load_graph(g)
        r = ctx.solve()
        assert (r.cost, r.flow) == (200, 100)
        mp = ctx.task_mapping()
        deltas, st = ctx.commit_schedule(continuation=3)
        assert deltas.shape[0] == 100 and set(deltas["type"].tolist()) == {PLACE}
        assert dict(zip(deltas["task"].tolist(), deltas["pu"].tolist())) == mp
        assert deltas["task"].tolist() == sorted(deltas["task"].tolist())
        assert (st["placed"], st["arcs_removed"], st["running_added"], st["running_converted"]) == (100, 200, 100, 0)
        assert st["unsched_updates"] == 1
        assert st["records"] == 300 + st["unsched_updates"] + st["cap_updates"]
        assert ctx.store_stats()["superseded"] == 0
        t = dev_table(ctx)
        running = [a for a in t.values() if a[3] == 1]
        assert len(running) == 100 and set(running) == {(1, 1, 3, 1)}
        assert (U, SINK) not in t
        assert sum(1000 - t[(EC, m)][1] for m in machines) == 100
        assert all(t[(COORD, m)][1] == t[(EC, m)][1] for m in machines)
        assert live(t) == commit_reference(g, mp, 3, True)
        r = ctx.solve()
        assert (r.cost, r.flow) == (300, 100)
        assert ctx.scheduling_deltas().shape[0] == 0


def run_differential(cell, rounds, **opts):
    T = cell.T0
    with native.Context(0, **opts) as a, native.Context(0, **opts) as b:
        for c in (a, b):
            c.load_graph(cell.graph())
        pins = 0
        for rnd in range(rounds):
            ra, rb = a.solve(), b.solve()
            st, cost, flow, _ = ko.cost_scaling(cell.graph())
            assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow), rnd
            mp = b.task_mapping()                      # both driven from B's placements
            before = cell.graph()
            waiting = set(cell.task_ids(cell.WAIT).tolist())
            host = cell.step(mp, 0, 0, age_cost=0, seed=100 + rnd)
            a.apply_deltas(host)
            deltas, stats = b.commit_schedule()
            placed = {t: p for t, p in mp.items() if t in waiting}
            assert dict(zip(deltas["task"].tolist(), deltas["pu"].tolist())) == placed, rnd
            pins += len(placed)
            model = cell.graph()
            same_graph(b, model)
            same_graph(a, model)
            want = live(arc_table(model))
            got = dev_table(b)
            assert {k: v[3] for k, v in got.items()} == {k: v[3] for k, v in want.items()}, rnd
            assert got == want == commit_reference(before, placed, 0, True), rnd
            assert stats["records"] == host.shape[0], rnd
            assert stats["placed"] == len(placed) == stats["running_added"]
            assert b.store_stats()["superseded"] == 0
            churn_stream = cell.step({}, T // 20, T // 20, seed=200 + rnd)
            a.apply_deltas(churn_stream)
            b.apply_deltas(churn_stream)
            same_graph(b, cell.graph())
        ra, rb = a.solve(), b.solve()
        st, cost, flow, _ = ko.cost_scaling(cell.graph())
        assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow)
        assert pins > 0
        return rb


def test_differential_against_host_path_cell_solver():
    r = run_differential(churn.Cell(200, 20, 4, 5, 3), 3)
    assert r.raw["solver"] == 1


def test_differential_against_host_path_engine():
    r = run_differential(churn.Cell(1000, 100, 5, 10, 7), 3, cell_nodes=-1)
    assert r.raw["solver"] == 0


def test_differential_against_host_path_engine_warm_start():
    r = run_differential(churn.Cell(1000, 100, 5, 10, 7), 3, cell_nodes=-1, warm_start=1)
    assert r.raw["solver"] == 0 and r.raw["warm_started"] == 1


def test_config2_size_one_round():
    """PU and aggregator segments run out of slack at this size: in-place inserts
    and the CSR rebuild both occur (the count is not asserted)."""
    cell = churn.Cell(10_000, 1_000, 25, 100, 12)
    with native.Context(0) as ctx:
        ctx.load_graph(cell.graph())
        ctx.solve()
        mp = ctx.task_mapping()
        deltas, stats = ctx.commit_schedule()
        host = cell.step(mp, 0, 0, age_cost=0)
        assert stats["placed"] == deltas.shape[0] == len(mp)
        assert stats["records"] == host.shape[0]
        model = cell.graph()
        same_graph(ctx, model)
        assert dev_table(ctx) == live(arc_table(model))
        r = ctx.solve()
        st, cost, flow, _ = ko.cost_scaling(model)
        assert st == 0 and (r.cost, r.flow) == (cost, flow)


def long_segment_graph():
    """3 tasks × 130 one-slot machine/PU pairs plus U: every task's segment spans
    more than two 64-position chunks."""
    SINK, U, M0, P0, T0, N = 1, 2, 3, 133, 263, 130
    nodes = [(SINK, -3, 3), (U, 0, 0)]
    arcs = [(U, SINK, 0, 3, 0)]
    for k in range(N):
        nodes += [(M0 + k, 0, 4), (P0 + k, 0, 2)]
        arcs += [(M0 + k, P0 + k, 0, 1, 0), (P0 + k, SINK, 0, 1, 0)]
    for i in range(3):
        nodes.append((T0 + i, 1, 1))
        arcs.append((T0 + i, U, 0, 1, 500))
        arcs += [(T0 + i, M0 + k, 0, 1, 1 + (7 * k + 13 * i) % 50) for k in range(N)]
    return graph_from_lists(nodes, arcs)


def hub_graph():
    """300 tasks → one machine → one PU of 300 slots (and U)."""
    SINK, U, MACH, PU, T0, N = 1, 2, 3, 4, 5, 300
    nodes = [(SINK, -N, 3), (U, 0, 0), (MACH, 0, 4), (PU, 0, 2)]
    arcs = [(U, SINK, 0, N, 0), (MACH, PU, 0, N, 0), (PU, SINK, 0, N, 0)]
    for i in range(N):
        nodes.append((T0 + i, 1, 1))
        arcs += [(T0 + i, MACH, 0, 1, 1), (T0 + i, U, 0, 1, 9)]
    return graph_from_lists(nodes, arcs)


@pytest.mark.parametrize("cell_nodes", [0, -1], ids=["cell", "engine"])
def test_long_segments(cell_nodes):
    g = long_segment_graph()
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        assert len(mp) == 3
        deltas, st = ctx.commit_schedule(continuation=2)
        assert (st["placed"], st["arcs_removed"], st["running_added"]) == (3, 3 * 131, 3)
        t = dev_table(ctx)
        for task, pu in mp.items():
            assert [(k, v) for k, v in t.items() if k[0] == task] == [((task, pu), (1, 1, 2, 1))]
        assert (2, 1) not in t                      # U → sink reached 0
        assert live(t) == commit_reference(g, mp, 2, True)
        r = ctx.solve()
        assert (r.cost, r.flow) == (6, 3)


@pytest.mark.parametrize("cell_nodes", [0, -1], ids=["cell", "engine"])
def test_hub_pu(cell_nodes):
    g = hub_graph()
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        ctx.load_graph(g)
        r = ctx.solve()
        assert (r.cost, r.flow) == (300, 300)
        mp = ctx.task_mapping()
        assert set(mp.values()) == {4} and len(mp) == 300
        deltas, st = ctx.commit_schedule(continuation=7)
        assert (st["placed"], st["running_added"], st["arcs_removed"]) == (300, 300, 600)
        assert (st["unsched_updates"], st["cap_updates"]) == (1, 1)
        t = dev_table(ctx)
        assert sum(1 for k, v in t.items() if k[1] == 4 and v == (1, 1, 7, 1)) == 300
        assert (3, 4) not in t                      # machine → PU reached 0
        assert live(t) == commit_reference(g, mp, 7, True)
        r = ctx.solve()
        assert (r.cost, r.flow) == (300 * 7, 300)


def test_refusals_change_nothing():
    cell = churn.Cell(200, 20, 4, 5, 3)
    g = cell.graph()
    with native.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        ctx.load_graph(g)
        raises_code(native.KS_E_INVALID, ctx.commit_schedule)           # before a solve
        ctx.solve()
        before = dev_table(ctx)
        d0 = ctx.scheduling_deltas(commit=False)
        n = d0.shape[0]
        assert n > 0

        def unchanged(deltas):
            same_graph(ctx, g)
            assert dev_table(ctx) == before
            assert (ctx.scheduling_deltas(commit=False) == deltas).all()

        cnt = C.c_size_t()
        assert L.ks_commit_schedule(h, 1, 0, None, 0, None, 0, C.byref(cnt), None) == native.KS_OK   # count only
        assert cnt.value == n
        unchanged(d0)
        out = np.zeros(n, native.SCHED_DELTA_DT)
        assert L.ks_commit_schedule(h, 1, 0, None, 0, out.ctypes.data, n - 1, C.byref(cnt),
                                    None) == native.KS_E_INVALID                                    # cap too small
        unchanged(d0)
        # a task bound elsewhere migrates: refused, bindings as they were
        t, p = int(d0["task"][0]), int(d0["pu"][0])
        other = cell.PU0 if p != cell.PU0 else cell.PU0 + 1
        ctx.set_bindings({t: other})
        d1 = ctx.scheduling_deltas(commit=False)
        assert native.KS_DELTA_MIGRATE in d1["type"].tolist()
        raises_code(native.KS_E_INVALID, ctx.commit_schedule)
        unchanged(d1)
        # a capacity below its lower bound cannot be produced here; an unknown flag is refused
        assert L.ks_commit_schedule(h, 2, 0, None, 0, out.ctypes.data, n, C.byref(cnt), None) == native.KS_E_INVALID
        unchanged(d1)
        ctx.set_bindings({t: 0})
        deltas, st = ctx.commit_schedule()
        assert (deltas == d0).all() and st["placed"] == n
        raises_code(native.KS_E_INVALID, ctx.commit_schedule)           # the solution is gone
        ctx.solve()
        assert ctx.scheduling_deltas(commit=False).shape[0] == 0        # the bindings were committed


def test_without_resource_caps():
    cell = churn.Cell(200, 20, 4, 5, 3)
    g = cell.graph()
    with native.Context(0) as ctx:
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        before = dev_table(ctx)
        deltas, st = ctx.commit_schedule(resource_caps=False)
        assert st["cap_updates"] == 0 and st["placed"] == len(mp) > 0
        assert st["records"] == st["arcs_removed"] + st["running_added"] + st["unsched_updates"]
        t = dev_table(ctx)
        res = [k for k in before if k[0] < cell.U0 and k[1] != cell.SINK]   # X → rack, rack → machine, machine → PU
        assert len(res) == cell.R + 2 * cell.M
        assert all(t[k] == before[k] for k in res)
        assert live(t) == commit_reference(g, mp, 0, False)
