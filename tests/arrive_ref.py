"""The rule of ks_add_tasks (include/ksmcmf.h) restated on the host: a graph table, the new
task ids, one list of (head, cost) per task, the aggregator ids or None and the sink cost in;
the exact ks_delta stream, the statistics and the graph after out. It follows
AddOrUpdateJobNodes (flowmanager/graph_manager.go:166-208) → addTaskNode (:632-648),
updateUnscheduledAggNode(+1) (:194, :1291-1305) and updateTaskNode (:1183-1192) with its arc
writers (:1197-1285), each an AddArc(task, head, 0, 1, cost, ArcTypeOther). The stream's order
is the contract's: the ADD_NODE records in input order, the task arcs in input order, the
aggregator records in ascending aggregator id. Every refusal raises, in the order the library
finds them: the sink cost, the ids, the arcs in input order (a head before its cost), the
tasks' aggregator counts in input order, the sink count. Test infrastructure: no product code
uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import OTHER, SINK, TASK, arc_table
from remove_ref import DELTA_DT

KS_ADD_NODE, KS_ADD_ARC, KS_UPDATE_ARC = 0, 2, 3
MAX_ID = 1 << 30
MAX_COST = 1 << 40
STAT_KEYS = ("tasks", "arcs_added", "unsched_updates", "unsched_added", "records")


class OutOfRange(ValueError):
    """KS_E_RANGE: an id outside 1 … 2^30 − 1 or a cost beyond ±2^40 (args[0]: the id or the task)."""


class InvalidArrival(ValueError):
    """KS_E_INVALID (args[0]: the task id named, None when none is; args[1]: the head, if any)."""


class Arrival(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call
    ntype: list         # node types after the call, by id − 1
    supply: list        # supplies after the call as stated (the sink's follows at the solve)
    alive: set          # live ids after the call
    stream: np.ndarray  # the records in the contract's order (DELTA_DT)
    stats: dict         # ks_add_stats
    superseded: int     # arc records a later record of the same (src, dst) replaces


def offsets(lists) -> tuple:
    """The C-ABI's form of the lists: (arc_off, dst, cost)."""
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = [a for x in lists for a in x]
    return off, np.asarray([d for d, _ in flat], np.uint64), np.asarray([c for _, c in flat], np.int64)


def arrive_reference(g, tasks, lists, unsched_ids=None, sink_cost: int = 0, alive=None) -> Arrival:
    """g: a gen.Graph (alive: its live node ids, default all). lists[i]: task i's (head, cost) pairs."""
    assert len(tasks) == len(lists)
    if abs(int(sink_cost)) > MAX_COST:
        raise OutOfRange(None)
    ntype = [int(t) for t in g.ntype]
    supply = [int(s) for s in g.supply]
    n = len(ntype)
    live = set(range(1, n + 1)) if alive is None else set(alive)
    arcs = arc_table(g)
    if not tasks:
        return Arrival(arcs, ntype, supply, live, np.zeros(0, DELTA_DT), dict.fromkeys(STAT_KEYS, 0), 0)
    new: list = []
    for t in tasks:
        t = int(t)
        if t < 1 or t >= MAX_ID:
            raise OutOfRange(t)
        if t in live or t in new:                 # a live node, or listed twice: "already present"
            raise InvalidArrival(t)
        new.append(t)
    sinks = {i for i in live if ntype[i - 1] == SINK}
    if unsched_ids is None:
        aggs = {s for (s, d) in arcs if d in sinks and ntype[s - 1] == OTHER}
    else:
        aggs = {int(a) for a in unsched_ids}
    for t, lst in zip(new, lists):                # the heads as they were before the call
        for d, c in lst:
            d, c = int(d), int(c)
            if d < 1 or d > n or d not in live or ntype[d - 1] == TASK:
                raise InvalidArrival(t, d)
            if abs(c) > MAX_COST:
                raise OutOfRange(t)
    gain: dict = {}
    for t, lst in zip(new, lists):
        mine = [int(d) for d, _ in lst if int(d) in aggs]
        if len(mine) > 1:                         # two aggregators, or one twice: a task has one job
            raise InvalidArrival(t)
        if not mine and unsched_ids is None:      # its aggregator may have lost the arc that marks it
            raise InvalidArrival(t)
        for d in mine:
            gain[d] = gain.get(d, 0) + 1
    if gain and len(sinks) != 1:
        raise InvalidArrival(None)
    rows = [(KS_ADD_NODE, TASK, t, 0, 0, 0, 0, 0, 0, 1) for t in new]
    rows += [(KS_ADD_ARC, 0, 0, t, int(d), 0, 1, int(c), 0, 0) for t, lst in zip(new, lists) for d, c in lst]
    upd = add = 0
    sink = next(iter(sinks)) if len(sinks) == 1 else 0
    for u in sorted(gain):
        if (u, sink) in arcs:                     # low, cost and type kept, the capacity raised
            lo, cap, co, ty = arcs[(u, sink)]
            rows.append((KS_UPDATE_ARC, ty, 0, u, sink, lo, cap + gain[u], co, co, 0))
            upd += 1
        else:                                     # the AddArc branch (:1300-1304)
            rows.append((KS_ADD_ARC, 0, 0, u, sink, 0, gain[u], int(sink_cost), 0, 0))
            add += 1
    stream = np.zeros(len(rows), DELTA_DT)
    for name, col in zip(DELTA_DT.names, zip(*rows)):
        stream[name] = np.asarray(col, dtype=DELTA_DT[name])
    top = max(n, max(new))
    ntype += [0] * (top - n)
    supply += [0] * (top - n)
    for t in new:
        ntype[t - 1], supply[t - 1] = TASK, 1
    seen = 0
    for kind, ty, _, s, d, lo, cap, co, _, _ in rows[len(new):]:
        seen += (s, d) in arcs and s in new       # only a task's repeated head can supersede
        arcs[(s, d)] = (lo, cap, co, ty)
    narcs = sum(len(x) for x in lists)
    stats = dict(tasks=len(new), arcs_added=narcs, unsched_updates=upd, unsched_added=add, records=len(rows))
    return Arrival(arcs, ntype, supply, live | set(new), stream, stats, seen)
