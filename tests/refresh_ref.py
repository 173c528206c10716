"""The rule of ks_update_tasks (include/ksmcmf.h) restated on the host: the arc table in
arc-slot order (the order of ks_get_graph), the node types, the bindings, the task ids, one list
of (head, cost) per task, the aggregator ids or None, the sink cost and the flag in; the exact
ks_delta stream, the statistics and the arcs after out. It follows UpdateTimeDependentCosts =
AddOrUpdateJobNodes (flowmanager/graph_manager.go:211-213, :166-208) → updateTaskNode
(:1183-1192) with its arc writers (:1197-1285), each AddArc or ChangeArcCost
(graph_change_manager.go:171-182) and then removeInvalidECPrefArcs / removeInvalidPrefResArcs
(:732-790), except that a running arc is never deleted. The stream's order is the contract's:
the records on held arcs in arc-slot order, the new arcs in input order, the aggregator records
in ascending aggregator id. Every refusal raises, in the order the library finds them: the flag,
the sink cost, the offsets (the lists here: nothing to check), the ids in input order, the arcs
in input order (on one arc the head, the repeat, the cost), the tasks' aggregator counts in input
order, the sink count. Test infrastructure: no product code uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import OTHER, SINK, TASK
from remove_ref import DELTA_DT

KS_ADD_ARC, KS_UPDATE_ARC = 2, 3
KEEP_UNLISTED = 1
MAX_COST = 1 << 40
STAT_KEYS = ("tasks", "arcs_added", "cost_updates", "arcs_unchanged", "running_kept", "arcs_removed",
             "unsched_updates", "unsched_added", "records")


class OutOfRange(ValueError):
    """KS_E_RANGE: a cost beyond ±2^40 (args[0]: the task, None for the sink cost)."""


class InvalidRefresh(ValueError):
    """KS_E_INVALID (args[0]: the task id named, None when none is; args[1]: the head, if any)."""


class Refresh(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call, in arc-table order
    stream: np.ndarray  # the records in the contract's order (DELTA_DT)
    stats: dict         # ks_update_stats


def refresh_reference(ntype, table: dict, tasks, lists, bindings: dict, unsched_ids=None, sink_cost: int = 0,
                      flags: int = 0, alive=None) -> Refresh:
    """ntype: node types by id − 1 (alive: the live ids, default all). table: {(src, dst): (low,
    cap, cost, type)} in arc-slot order. lists[i]: task i's (head, cost) pairs. bindings: {task:
    pu} as the device keeps them (0 or absent: unbound)."""
    assert len(tasks) == len(lists)
    if flags & ~KEEP_UNLISTED:
        raise InvalidRefresh(None)
    if abs(int(sink_cost)) > MAX_COST:
        raise OutOfRange(None)
    ntype = [int(t) for t in ntype]
    n = len(ntype)
    live = set(range(1, n + 1)) if alive is None else set(alive)
    arcs = dict(table)
    if not tasks:
        return Refresh(arcs, np.zeros(0, DELTA_DT), dict.fromkeys(STAT_KEYS, 0))
    mine: list = []
    for t in tasks:
        t = int(t)
        if t < 1 or t > n or t not in live or ntype[t - 1] != TASK or t in mine:
            raise InvalidRefresh(t)
        mine.append(t)
    sinks = {i for i in live if ntype[i - 1] == SINK}
    if unsched_ids is None:
        aggs = {s for (s, d) in arcs if d in sinks and ntype[s - 1] == OTHER}
    else:
        aggs = {int(a) for a in unsched_ids}
    for t, lst in zip(mine, lists):
        heads = set()
        for d, c in lst:
            d, c = int(d), int(c)
            if d < 1 or d > n or d not in live or ntype[d - 1] == TASK:
                raise InvalidRefresh(t, d)
            if d in heads:                          # the diff needs a set
                raise InvalidRefresh(t, d)
            heads.add(d)
            if abs(c) > MAX_COST:
                raise OutOfRange(t)
    keep = bool(flags & KEEP_UNLISTED)
    listed = {(t, int(d)): int(c) for t, lst in zip(mine, lists) for d, c in lst}
    held = {t: [k for k in arcs if k[0] == t] for t in set(mine)}
    gain: dict = {}
    for t, lst in zip(mine, lists):
        ends = {int(d) for d, _ in lst if int(d) in aggs}
        ends |= {d for _, d in held[t] if d in aggs}         # an unlisted aggregator arc is kept
        if len(ends) > 1:                           # a task does not change its job
            raise InvalidRefresh(t)
        if not ends and unsched_ids is None and not bindings.get(t, 0):
            raise InvalidRefresh(t)                 # its aggregator may have lost the arc that marks it
        for d, _ in lst:
            if int(d) in aggs and (t, int(d)) not in arcs:
                gain[int(d)] = gain.get(int(d), 0) + 1
    if gain and len(sinks) != 1:
        raise InvalidRefresh(None)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["tasks"] = len(mine)
    rows = []
    own = set(mine)
    for (s, d), (lo, cap, co, ty) in arcs.items():  # the held arcs, in arc-slot order
        if s not in own:
            continue
        if (s, d) in listed:
            if ty == 1:                             # a running arc keeps its cost (:1250-1255)
                st["running_kept"] += 1
            elif listed[(s, d)] != co:              # ChangeArcCost
                rows.append((KS_UPDATE_ARC, ty, 0, s, d, lo, cap, listed[(s, d)], co, 0))
                st["cost_updates"] += 1
            else:
                st["arcs_unchanged"] += 1
        elif ty != 1 and d not in aggs and not keep:
            rows.append((KS_UPDATE_ARC, ty, 0, s, d, 0, 0, co, co, 0))
            st["arcs_removed"] += 1
    for t, lst in zip(mine, lists):                 # the new arcs, in input order
        for d, c in lst:
            if (t, int(d)) not in arcs:
                rows.append((KS_ADD_ARC, 0, 0, t, int(d), 0, 1, int(c), 0, 0))
                st["arcs_added"] += 1
    sink = next(iter(sinks)) if len(sinks) == 1 else 0
    for u in sorted(gain):
        if (u, sink) in arcs:                       # low, cost and type kept, the capacity raised
            lo, cap, co, ty = arcs[(u, sink)]
            rows.append((KS_UPDATE_ARC, ty, 0, u, sink, lo, cap + gain[u], co, co, 0))
            st["unsched_updates"] += 1
        else:                                       # the AddArc branch (:1300-1304)
            rows.append((KS_ADD_ARC, 0, 0, u, sink, 0, gain[u], int(sink_cost), 0, 0))
            st["unsched_added"] += 1
    st["records"] = len(rows)
    stream = np.zeros(len(rows), DELTA_DT)
    if rows:
        for name, col in zip(DELTA_DT.names, zip(*rows)):
            stream[name] = np.asarray(col, dtype=DELTA_DT[name])
    for kind, ty, _, s, d, lo, cap, co, _, _ in rows:
        if kind == KS_UPDATE_ARC and lo == 0 and cap == 0:
            del arcs[(s, d)]
        else:
            arcs[(s, d)] = (lo, cap, co, ty)
    return Refresh(arcs, stream, st)
