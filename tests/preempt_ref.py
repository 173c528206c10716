"""The rule of ks_commit_preemptive (include/ksmcmf.h) restated on the host: a graph,
the scheduling deltas and the bindings in; the arc table, the new bindings and the
call's statistics out. It follows what the reference does after applySchedulingDeltas
with Preemption == true — updateArcsForScheduledTask (flowmanager/graph_manager.go:
855-888) with updateRunningTaskToUnscheduledAggArc (:1164-1181), TaskEvicted
(:412-433), TaskMigrated (:407-410) and capacityFromResNodeToParent returning
NumSlotsBelow (:662-667). Test infrastructure: no product code uses it."""
from __future__ import annotations

import numpy as np

from commit_ref import INTERMEDIATE, MACHINE, OTHER, PU, SINK, TASK, arc_table, topology_sums
from ksched_amd import gen

PLACE, PREEMPT, MIGRATE = 0, 1, 2
STAT_KEYS = ("placed", "preempted", "migrated", "running_added", "running_converted", "running_removed",
             "unsched_cost_updates", "cap_updates", "records")


def table_graph(ntype, supply, arcs: dict) -> gen.Graph:
    """A gen.Graph of an arc table {(src, dst): (low, cap, cost, type)}, in key order."""
    keys = sorted(arcs)
    col = lambda i: np.asarray([arcs[k][i] for k in keys], np.int64)
    return gen.Graph(np.asarray(ntype, np.int32), np.asarray(supply, np.int64),
                     np.asarray([k[0] for k in keys], np.int64), np.asarray([k[1] for k in keys], np.int64),
                     col(0), col(1), col(2), col(3).astype(np.int32))


def preempt_reference(g, deltas, bindings: dict, continuation: int, preemption: int, resource_caps: bool,
                      unsched_ids=None):
    """deltas: (kind, task, pu) triples in the order of ks_scheduling_deltas (pu of a
    PREEMPT: the PU it leaves). → (arcs {(src, dst): (low, cap, cost, type)} without the
    arcs whose capacity is 0, the new bindings, the stats dict of ks_preempt_stats)."""
    ntype = [int(t) for t in g.ntype]
    arcs = arc_table(g)
    before = dict(arcs)
    bind = {int(t): int(p) for t, p in bindings.items() if p}
    sink = {i + 1 for i, t in enumerate(ntype) if t == SINK}
    if unsched_ids is None:
        aggs = {s for (s, d) in arcs if d in sink and ntype[s - 1] == OTHER}
    else:
        aggs = {int(a) for a in unsched_ids}
    out: dict[int, list[int]] = {}
    for s, d in arcs:
        out.setdefault(s, []).append(d)
    st = dict.fromkeys(STAT_KEYS, 0)
    for kind, t, p in deltas:
        kind, t, p = int(kind), int(t), int(p)
        if kind in (PREEMPT, MIGRATE):                    # TaskEvicted: the running arc goes, nothing else
            old = bind.pop(t)
            assert kind == MIGRATE or old == p
            assert (t, old) in arcs and arcs[(t, old)][3] == 1, "no running arc into the PU the task leaves"
            del arcs[(t, old)]
            st["running_removed"] += 1
        st[("placed", "preempted", "migrated")[kind]] += 1
        if kind == PREEMPT:
            continue
        if (t, p) in arcs:                                 # the preference arc becomes the running arc
            st["running_converted"] += 1
        else:
            st["running_added"] += 1
        arcs[(t, p)] = (0, 1, continuation, 1)
        bind[t] = p
        for d in out.get(t, ()):
            if d in aggs and (t, d) in arcs and d != p:
                lo, cap, co, ty = arcs[(t, d)]
                if co != preemption:                       # ChangeArcCost records a change only
                    arcs[(t, d)] = (lo, cap, preemption, ty)
                    st["unsched_cost_updates"] += 1
    if resource_caps:
        pu_slots = {s: c for (s, d), (lo, c, co, ty) in before.items() if d in sink and ntype[s - 1] == PU}
        slots, _ = topology_sums(ntype, before, pu_slots, {})
        for (u, v), (lo, cap, co, ty) in list(arcs.items()):
            tv = ntype[v - 1]
            if ntype[u - 1] == TASK or tv == SINK:
                continue
            if tv in (PU, MACHINE, INTERMEDIATE) or (tv == OTHER and slots.get(v, 0) > 0):
                new = slots.get(v, 0)
                assert new >= lo, "resource capacity below its lower bound"
                if new != cap:
                    arcs[(u, v)] = (lo, new, co, ty)
                    st["cap_updates"] += 1
    st["records"] = (st["running_added"] + st["running_converted"] + st["running_removed"] +
                     st["unsched_cost_updates"] + st["cap_updates"])
    return {k: a for k, a in arcs.items() if a[1] > 0}, bind, st


# ---- inputs shared by the CPU and the GPU suite -----------------------------------
# The toy network: three tasks, three one-slot machine/PU pairs (no task reaches M3 at
# first) and one unscheduled aggregator; its three optima are unique.
TOY_NTYPE = [3, 0, 4, 2, 4, 2, 4, 2, 1, 1, 1]          # SINK 1, U 2, M1 3, P1 4, M2 5, P2 6, M3 7, P3 8, T1..T3 9..11
TOY_SUPPLY = [-3, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
TOY_ARCS = {(2, 1): (0, 3, 0, 0),
            (3, 4): (0, 1, 0, 0), (5, 6): (0, 1, 0, 0), (7, 8): (0, 1, 0, 0),
            (4, 1): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (8, 1): (0, 1, 0, 0),
            (9, 3): (0, 1, 1, 0), (9, 5): (0, 1, 5, 0), (9, 2): (0, 1, 100, 0),
            (10, 3): (0, 1, 2, 0), (10, 5): (0, 1, 3, 0), (10, 2): (0, 1, 100, 0),
            (11, 3): (0, 1, 50, 0), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0)}
TOY_CONTINUATION, TOY_PREEMPTION = 0, 20
# per solve: (kind, type, src, dst, low, cap, cost) records applied before it, the optimal
# cost, the deltas (kind, task, pu), the records of the commit and its non-zero stats
TOY_ROUNDS = [
    dict(edits=[], cost=64, deltas=[(PLACE, 9, 4), (PLACE, 10, 6)], records=4,
         stats=dict(placed=2, running_added=2, unsched_cost_updates=2)),
    dict(edits=[(3, 0, 11, 2, 0, 1, 500), (3, 0, 11, 3, 0, 1, 1)], cost=21,
         deltas=[(PREEMPT, 9, 4), (PLACE, 11, 4)], records=3,
         stats=dict(preempted=1, placed=1, running_removed=1, running_added=1, unsched_cost_updates=1)),
    dict(edits=[(3, 1, 10, 6, 0, 1, 10), (2, 0, 10, 7, 0, 1, 0)], cost=5,
         deltas=[(PLACE, 9, 6), (MIGRATE, 10, 8)], records=3,
         stats=dict(placed=1, migrated=1, running_added=2, running_removed=1)),
    dict(edits=[], cost=0, deltas=[], records=0, stats={}),
]


def toy_stats(rnd: dict) -> dict:
    return {**dict.fromkeys(STAT_KEYS, 0), **rnd["stats"], "records": rnd["records"]}


def apply_edits(arcs: dict, edits) -> None:
    for kind, ty, s, d, lo, cap, co in edits:
        arcs[(s, d)] = (lo, cap, co, ty)


# Cell(preemption=True) inputs: shape → the preemption cost (continuation 0). Chosen so
# that over three rounds with 5 % churn the oracle's deltas hold every kind and that in a
# later round every optimum moves a running task (test_commit_preemptive_cpu.py asserts it).
CELL_CASES = {(200, 20, 4, 5, 3): 150, (1000, 100, 5, 10, 7): 150}
