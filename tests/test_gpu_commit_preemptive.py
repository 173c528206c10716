"""GPU: ks_commit_preemptive — every PLACE, PREEMPT and MIGRATE of a solve committed on
the device-resident graph (running arcs with low 0, running arcs deleted, preemption
costs, resource capacities without subtraction) — against the rule restated on the
host (tests/preempt_ref.py) and against the host path it replaces (churn.Cell's own
preemptive records through ks_apply_deltas)."""
import ctypes as C

import numpy as np
import pytest

from commit_ref import arc_table, commit_reference
from graphs import graph_from_lists, same_graph
from ksched_amd import churn, native
from oracle import ko, sched_ref
from preempt_ref import (CELL_CASES, MIGRATE, PLACE, PREEMPT, TOY_ARCS, TOY_CONTINUATION, TOY_NTYPE,
                         TOY_PREEMPTION, TOY_ROUNDS, TOY_SUPPLY, apply_edits, preempt_reference, table_graph,
                         toy_stats)
from test_gpu_commit import dev_table, hub_graph, live, long_segment_graph, raises_code

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("cell_nodes", [0, -1], ids=["cell", "engine"])


def triples(deltas) -> list:
    return list(zip(deltas["type"].tolist(), deltas["task"].tolist(), deltas["pu"].tolist()))


def arc_records(recs) -> np.ndarray:
    """(kind, type, src, dst, low, cap, cost) → DELTA_DT records."""
    out = np.zeros(len(recs), native.DELTA_DT)
    for x, (kind, ty, s, d, lo, cap, co) in zip(out, recs):
        x["kind"], x["type"], x["src"], x["dst"], x["low"], x["cap"], x["cost"] = kind, ty, s, d, lo, cap, co
    return out


def dev_graph(ctx, g):
    """The device-resident arcs on g's nodes, as a graph for the oracle and the rule."""
    return table_graph(g.ntype, g.supply, dev_table(ctx))


def check_commit(ctx, g, bindings, continuation, preemption, **kw):
    """One commit against the rule given the device's own deltas; → (deltas, stats, bindings)."""
    before = dev_graph(ctx, g)
    deltas, st = ctx.commit_preemptive(continuation=continuation, preemption=preemption, **kw)
    want, nb, wst = preempt_reference(before, triples(deltas), bindings, continuation, preemption,
                                      kw.get("resource_caps", True))
    assert dev_table(ctx) == want
    assert st == wst
    assert st["records"] == (st["running_added"] + st["running_converted"] + st["running_removed"] +
                             st["unsched_cost_updates"] + st["cap_updates"])
    assert ctx.store_stats()["superseded"] == 0
    return deltas, st, nb


@BOTH
def test_toy_network_three_kinds(cell_nodes):
    g0 = table_graph(TOY_NTYPE, TOY_SUPPLY, TOY_ARCS)
    arcs = dict(TOY_ARCS)
    bindings: dict = {}
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        ctx.load_graph(g0)
        for n, rnd in enumerate(TOY_ROUNDS):
            if rnd["edits"]:
                ctx.apply_deltas(arc_records(rnd["edits"]))
                apply_edits(arcs, rnd["edits"])
            r = ctx.solve()
            assert (r.cost, r.flow) == (rnd["cost"], 3), n
            # the bindings of the earlier commits are in place: only this round's moves show
            assert triples(ctx.scheduling_deltas(commit=False)) == rnd["deltas"], n
            if not rnd["deltas"]:
                continue
            g = table_graph(TOY_NTYPE, TOY_SUPPLY, arcs)
            deltas, st = ctx.commit_preemptive(continuation=TOY_CONTINUATION, preemption=TOY_PREEMPTION)
            assert triples(deltas) == rnd["deltas"], n
            assert st == toy_stats(rnd) and st["cap_updates"] == 0, n
            arcs, bindings, _ = preempt_reference(g, rnd["deltas"], bindings, TOY_CONTINUATION, TOY_PREEMPTION, True)
            assert dev_table(ctx) == arcs, n
            assert ctx.store_stats()["superseded"] == 0


def test_conversion_of_a_direct_arc():
    """Tasks whose preference arcs point straight at PUs: the arc itself becomes the
    running arc, nothing is added."""
    SINK, U, P0, T0 = 1, 2, 3, 6
    nodes = [(SINK, -2, 3), (U, 0, 0)] + [(P0 + k, 0, 2) for k in range(3)] + [(T0 + i, 1, 1) for i in range(2)]
    arcs = [(U, SINK, 0, 2, 0)] + [(P0 + k, SINK, 0, 1, 0) for k in range(3)]
    for i in range(2):
        arcs += [(T0 + i, U, 0, 1, 90)] + [(T0 + i, P0 + k, 0, 1, 10 + 5 * ((k + 2 * i) % 3)) for k in range(3)]
    g = graph_from_lists(nodes, arcs)
    with native.Context(0) as ctx:
        ctx.load_graph(g)
        r = ctx.solve()
        assert (r.cost, r.flow) == (20, 2)
        inserted = ctx.store_stats()["inserted"]
        deltas, st, _ = check_commit(ctx, g, {}, 4, 7)
        assert triples(deltas) == [(PLACE, T0, P0), (PLACE, T0 + 1, P0 + 1)]
        assert (st["placed"], st["running_converted"], st["running_added"], st["unsched_cost_updates"]) == (2, 2, 0, 2)
        assert ctx.store_stats()["inserted"] == inserted          # no ADD_ARC
        t = dev_table(ctx)
        assert t[(T0, P0)] == t[(T0 + 1, P0 + 1)] == (0, 1, 4, 1)
        assert t[(T0, P0 + 1)] == (0, 1, 15, 0) and t[(T0, U)] == (0, 1, 7, 0)
        r = ctx.solve()
        assert (r.cost, r.flow) == (8, 2)
        assert ctx.scheduling_deltas(commit=False).shape[0] == 0


@BOTH
def test_long_segments(cell_nodes):
    """Every task's segment spans more than two 64-position chunks: the running arc is
    added behind 131 arcs and found there again when the task leaves its PU. (Raising
    the running arcs' cost alone would send each task through its machine arc into the
    same PU, a move without a delta; the second stream therefore also prices two tasks
    out of their machine and frees the third one's U arc.)"""
    g = long_segment_graph()
    U, M0, P0, T0 = 2, 3, 133, 263
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        assert len(mp) == 3
        deltas, st, bindings = check_commit(ctx, g, {}, 2, 500)
        assert triples(deltas) == [(PLACE, t, p) for t, p in sorted(mp.items())]
        assert (st["running_added"], st["running_converted"], st["unsched_cost_updates"]) == (3, 0, 0)
        # the running arcs (and for two tasks the arc into that machine) become expensive:
        # those two move to another machine; the third, its U arc now free, is preempted
        recs = []
        for t, p in sorted(mp.items()):
            recs.append((3, 1, t, p, 0, 1, 1000))
            if t < T0 + 2:
                recs.append((3, 0, t, M0 + (p - P0), 0, 1, 1000))
        recs.append((3, 0, T0 + 2, U, 0, 1, 0))
        ctx.apply_deltas(arc_records(recs))
        r = ctx.solve()
        st0, cost, flow, _ = ko.cost_scaling(dev_graph(ctx, g))
        assert st0 == 0 and (r.cost, r.flow) == (cost, flow)
        deltas, st, bindings = check_commit(ctx, g, bindings, 2, 500)
        assert [(k, t) for k, t, _ in triples(deltas)] == [(PREEMPT, T0 + 2), (MIGRATE, T0), (MIGRATE, T0 + 1)]
        assert (st["running_removed"], st["running_added"]) == (3, 2)
        t = dev_table(ctx)
        assert all((task, pu) not in t for task, pu in mp.items())
        assert T0 + 2 not in bindings and len(bindings) == 2
        r = ctx.solve()
        st0, cost, flow, _ = ko.cost_scaling(dev_graph(ctx, g))
        assert st0 == 0 and (r.cost, r.flow) == (cost, flow)
        # the bindings were committed: the next deltas are the moves away from them (machines
        # of equal cost with a free PU remain, so an optimum may migrate a task again)
        assert triples(ctx.scheduling_deltas(commit=False)) == sched_ref.scheduling_deltas(
            bindings, ctx.task_mapping(), [T0, T0 + 1, T0 + 2])


@BOTH
def test_both_modes_through_one_context(cell_nodes):
    """The two commits share one kernel family and one scratch: a pinned commit after a
    preemptive one with a PREEMPT and two MIGRATEs (item kinds, PUs left, running arcs
    found) must see none of that call's items, and a preemptive commit after the pinned
    one none of its."""
    g = long_segment_graph()
    U, M0, P0, T0 = 2, 3, 133, 263
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        # the preemptive test_long_segments sequence
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        assert len(mp) == 3
        deltas, st, bindings = check_commit(ctx, g, {}, 2, 500)
        assert triples(deltas) == [(PLACE, t, p) for t, p in sorted(mp.items())]
        assert (st["running_added"], st["running_converted"], st["unsched_cost_updates"]) == (3, 0, 0)
        recs = []
        for t, p in sorted(mp.items()):
            recs.append((3, 1, t, p, 0, 1, 1000))
            if t < T0 + 2:
                recs.append((3, 0, t, M0 + (p - P0), 0, 1, 1000))
        recs.append((3, 0, T0 + 2, U, 0, 1, 0))
        ctx.apply_deltas(arc_records(recs))
        r = ctx.solve()
        st0, cost, flow, _ = ko.cost_scaling(dev_graph(ctx, g))
        assert st0 == 0 and (r.cost, r.flow) == (cost, flow)
        deltas, st, bindings = check_commit(ctx, g, bindings, 2, 500)
        assert [(k, t) for k, t, _ in triples(deltas)] == [(PREEMPT, T0 + 2), (MIGRATE, T0), (MIGRATE, T0 + 1)]
        assert (st["running_removed"], st["running_added"]) == (3, 2)
        # the pinned test_long_segments on the same context
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
        # and the preemptive mode after the pinned one: three PLACEs, nothing to leave
        ctx.load_graph(g)
        ctx.solve()
        mp = ctx.task_mapping()
        deltas, st, _ = check_commit(ctx, g, {}, 2, 500)
        assert triples(deltas) == [(PLACE, t, p) for t, p in sorted(mp.items())]
        assert (st["placed"], st["preempted"], st["migrated"]) == (3, 0, 0)
        assert (st["running_added"], st["running_removed"]) == (3, 0)


def test_a_migrate_is_one_scheduling_delta():
    """ks_scheduling_deltas with MIGRATEs between PLACEs: every kind counts once in the
    positions, so the count is the number of moves and no record is left empty."""
    cell = churn.Cell(200, 20, 4, 5, 3)
    with native.Context(0) as ctx:
        ctx.load_graph(cell.graph())
        ctx.solve()
        d0 = ctx.scheduling_deltas(commit=False)
        n = d0.shape[0]
        assert n > 4 and set(d0["type"].tolist()) == {PLACE}
        moved = {}
        for i in (0, 2):                                    # bound elsewhere: these two migrate
            t, p = int(d0["task"][i]), int(d0["pu"][i])
            moved[t] = cell.PU0 if p != cell.PU0 else cell.PU0 + 1
        ctx.set_bindings(moved)
        cnt = C.c_size_t()
        assert ctx._L.ks_scheduling_deltas(ctx._h, 0, None, 0, C.byref(cnt)) == native.KS_OK
        assert cnt.value == n
        d1 = ctx.scheduling_deltas(commit=False)
        assert d1.shape[0] == n and (d1["task"] != 0).all() and (d1["pu"] != 0).all()
        want = [(MIGRATE if t in moved else PLACE, t, p) for _, t, p in triples(d0)]
        assert triples(d1) == want == sched_ref.scheduling_deltas(moved, ctx.task_mapping(), d0["task"].tolist())
        assert triples(ctx.scheduling_deltas(commit=True)) == want
        assert ctx.scheduling_deltas(commit=False).shape[0] == 0   # the same solve against its own bindings


@BOTH
def test_many_preemptions_in_one_call(cell_nodes):
    g = hub_graph()
    SINK, MACH, PU = 1, 3, 4
    with native.Context(0, cell_nodes=cell_nodes) as ctx:
        ctx.load_graph(g)
        r = ctx.solve()
        assert (r.cost, r.flow) == (300, 300)
        deltas, st, bindings = check_commit(ctx, g, {}, 0, 9)
        assert (st["placed"], st["running_added"], st["unsched_cost_updates"], st["cap_updates"]) == (300, 300, 0, 0)
        ctx.apply_deltas(arc_records([(3, 0, PU, SINK, 0, 100, 0)]))
        r = ctx.solve()
        assert (r.cost, r.flow) == (1800, 300)
        deltas, st, bindings = check_commit(ctx, g, bindings, 0, 9)
        assert deltas.shape[0] == 200 and set(deltas["type"].tolist()) == {PREEMPT}
        assert set(deltas["pu"].tolist()) == {PU}
        assert (st["preempted"], st["running_removed"], st["cap_updates"], st["records"]) == (200, 200, 1, 201)
        t = dev_table(ctx)
        assert t[(MACH, PU)] == (0, 100, 0, 0)
        assert sum(1 for k, v in t.items() if k[1] == PU and v == (0, 1, 0, 1)) == 100 == len(bindings)
        r = ctx.solve()
        assert (r.cost, r.flow) == (1800, 300)
        assert ctx.scheduling_deltas(commit=False).shape[0] == 0


def run_differential(shape, rounds, **opts):
    """Twin contexts on the model's graph: A takes the model's own records through
    ks_apply_deltas, B commits on device; both are driven from B's mapping."""
    pc = CELL_CASES[shape]
    cell = churn.Cell(*shape, preemption=True, preemption_cost=pc)
    T = cell.T0
    total = dict.fromkeys(("placed", "preempted", "migrated"), 0)
    with native.Context(0, **opts) as a, native.Context(0, **opts) as b:
        for c in (a, b):
            c.load_graph(cell.graph())
        for rnd in range(rounds):
            ra, rb = a.solve(), b.solve()
            before = cell.graph()
            st, cost, flow, _ = ko.cost_scaling(before)
            assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow), rnd
            mp = b.task_mapping()
            run = cell.task_ids(cell.RUN)
            bindings = dict(zip(run.tolist(), cell.pu[run - cell.TASK0].tolist()))
            want_deltas = sched_ref.scheduling_deltas(bindings, mp, np.concatenate([run, cell.task_ids(cell.WAIT)]))
            host = cell.step(mp, 0, 0, age_cost=0, seed=100 + rnd)
            a.apply_deltas(host)
            deltas, stats = b.commit_preemptive(continuation=0, preemption=pc)
            assert triples(deltas) == want_deltas, rnd
            model = cell.graph()
            same_graph(b, model)
            same_graph(a, model)
            want = live(arc_table(model))
            got = dev_table(b)
            assert {k: v[3] for k, v in got.items()} == {k: v[3] for k, v in want.items()}, rnd
            ref, _, ref_stats = preempt_reference(before, want_deltas, bindings, 0, pc, True)
            assert got == want == ref, rnd
            assert stats == ref_stats and stats["records"] == host.shape[0], rnd
            assert b.store_stats()["superseded"] == 0
            for k in total:
                total[k] += stats[k]
            churn_stream = cell.step(None, T // 20, T // 20, seed=200 + rnd)
            a.apply_deltas(churn_stream)
            b.apply_deltas(churn_stream)
            same_graph(b, cell.graph())
        ra, rb = a.solve(), b.solve()
        st, cost, flow, _ = ko.cost_scaling(cell.graph())
        assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow)
        assert total["placed"] > 0 and total["preempted"] + total["migrated"] > 0, total
        return rb


def test_differential_against_host_path_cell_solver():
    r = run_differential((200, 20, 4, 5, 3), 3)
    assert r.raw["solver"] == 1


def test_differential_against_host_path_engine():
    r = run_differential((1000, 100, 5, 10, 7), 3, cell_nodes=-1)
    assert r.raw["solver"] == 0


def test_differential_against_host_path_engine_warm_start():
    r = run_differential((1000, 100, 5, 10, 7), 3, cell_nodes=-1, warm_start=1)
    assert r.raw["solver"] == 0 and r.raw["warm_started"] == 1


def test_refusals_change_nothing():
    shape = (200, 20, 4, 5, 3)
    cell = churn.Cell(*shape, preemption=True, preemption_cost=CELL_CASES[shape])
    g = cell.graph()
    with native.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        ctx.load_graph(g)
        raises_code(native.KS_E_INVALID, ctx.commit_preemptive)          # before a solve
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
        out = np.zeros(n, native.SCHED_DELTA_DT)
        call = lambda flags, cc, pc, o, cap: L.ks_commit_preemptive(h, flags, cc, pc, None, 0, o, cap, C.byref(cnt), None)
        assert call(1, 0, 0, None, 0) == native.KS_OK                    # count only
        assert cnt.value == n
        unchanged(d0)
        assert call(1, 0, 0, out.ctypes.data, n - 1) == native.KS_E_INVALID   # cap too small
        unchanged(d0)
        for flags in (2, 3 | 4):
            assert call(flags, 0, 0, out.ctypes.data, n) == native.KS_E_INVALID
            unchanged(d0)
        assert call(1, 1 << 41, 0, out.ctypes.data, n) == native.KS_E_RANGE
        assert call(1, 0, -(1 << 41), out.ctypes.data, n) == native.KS_E_RANGE
        unchanged(d0)
        raises_code(native.KS_E_INVALID, ctx.commit_preemptive, unsched_ids=[10 ** 6])   # no such aggregator
        unchanged(d0)
        # an unbound task bound elsewhere by hand migrates, but has no running arc to leave
        t, p = int(d0["task"][0]), int(d0["pu"][0])
        other = cell.PU0 if p != cell.PU0 else cell.PU0 + 1
        ctx.set_bindings({t: other})
        d1 = ctx.scheduling_deltas(commit=False)
        # (a MIGRATE is one delta: the placements after it keep their places)
        assert triples(d1) == [(MIGRATE, t, p)] + triples(d0)[1:]
        raises_code(native.KS_E_VERIFY, ctx.commit_preemptive)
        unchanged(d1)
        ctx.set_bindings({t: 0})
        deltas, st = ctx.commit_preemptive(preemption=CELL_CASES[shape])
        assert (deltas == d0).all() and st["placed"] == n
        raises_code(native.KS_E_INVALID, ctx.commit_preemptive)          # the solution is gone
        ctx.solve()
        # the bindings were committed: the next deltas are the moves away from them (running
        # tasks are not pinned here, so a tie may move one)
        bound = dict(zip(d0["task"].tolist(), d0["pu"].tolist()))
        tasks = np.nonzero(g.ntype == 1)[0] + 1
        assert triples(ctx.scheduling_deltas(commit=False)) == sched_ref.scheduling_deltas(bound, ctx.task_mapping(),
                                                                                           tasks)


def test_pinned_commit_still_refuses_a_preemption():
    arcs = dict(TOY_ARCS)
    with native.Context(0) as ctx:
        ctx.load_graph(table_graph(TOY_NTYPE, TOY_SUPPLY, arcs))
        ctx.solve()
        ctx.commit_preemptive(continuation=TOY_CONTINUATION, preemption=TOY_PREEMPTION)
        ctx.apply_deltas(arc_records(TOY_ROUNDS[1]["edits"]))
        ctx.solve()
        before = dev_table(ctx)
        d = ctx.scheduling_deltas(commit=False)
        assert PREEMPT in d["type"].tolist()
        raises_code(native.KS_E_INVALID, ctx.commit_schedule)
        assert dev_table(ctx) == before
        assert (ctx.scheduling_deltas(commit=False) == d).all()
        deltas, _ = ctx.commit_preemptive(continuation=TOY_CONTINUATION, preemption=TOY_PREEMPTION)
        assert triples(deltas) == TOY_ROUNDS[1]["deltas"]
