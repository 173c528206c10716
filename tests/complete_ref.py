"""The rule of ks_complete_tasks (include/ksmcmf.h) restated on the host: a graph, the
finished task ids, the bindings and the flags in; the arc table, left, the bindings, the
equivalent ks_delta stream and the statistics out. It follows HandleTaskCompletion
(flowscheduler/scheduler.go:106-132) → TaskCompleted (flowmanager/graph_manager.go:389-405)
→ removeTaskNode (:803-813) with updateUnscheduledAggNode(−1) (:396, :1291-1305), and the
capacity rule of the two commits (capacityFromResNodeToParent, :662-667) over the sums of
ComputeTopologyStatistics (:480-511) on the graph without the completed tasks. The capacity
records stand here in (src, dst) order, the device's in arc-slot order: no (src, dst)
appears twice, so the order decides nothing. Test infrastructure: no product code uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import INTERMEDIATE, MACHINE, OTHER, PU, SINK, TASK, arc_table, topology_sums
from remove_ref import DELTA_DT, KS_REMOVE_NODE, KS_UPDATE_ARC, BelowLowerBound

KS_ADD_ARC = 2
STAT_KEYS = ("tasks", "bound", "arcs_removed", "unsched_updates", "cap_updates", "records")


class InvalidTask(ValueError):
    """KS_E_INVALID: an id that is 0, beyond the graph, dead or not a task (args[0]: the id)."""


class Completion(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call
    left: list          # per input id: the PU it was bound to, 0 = unbound
    removed: list       # the distinct ids, ascending
    bindings: dict      # {task: pu} after the call
    stream: np.ndarray  # the "r id" records, then the "x" capacity records (DELTA_DT)
    stats: dict         # ks_complete_stats


def complete_reference(g, tasks, bindings: dict, resource_caps: bool, preemptive: bool, unsched_ids=None,
                       alive=None) -> Completion:
    """g: a gen.Graph (alive: its live node ids, default all). bindings {task: pu}."""
    assert resource_caps or not preemptive
    ntype = [int(t) for t in g.ntype]
    n = len(ntype)
    arcs = arc_table(g)
    n_before = len(arcs)
    for t in tasks:
        t = int(t)
        if t < 1 or t > n or (alive is not None and t not in alive) or ntype[t - 1] != TASK:
            raise InvalidTask(t)
    bind = {int(t): int(p) for t, p in bindings.items() if p}
    left = [bind.get(int(t), 0) for t in tasks]
    removed = sorted({int(t) for t in tasks})
    gone = set(removed)
    bound = sum(1 for t in removed if t in bind)
    for t in removed:
        bind.pop(t, None)
    sink = {i + 1 for i, t in enumerate(ntype) if t == SINK and (alive is None or i + 1 in alive)}
    if unsched_ids is None:
        aggs = {s for (s, d) in arcs if d in sink and ntype[s - 1] == OTHER}
    else:
        aggs = {int(a) for a in unsched_ids}
    lost: dict[int, int] = {}
    if removed:
        for (s, d) in arcs:
            if s in gone and d in aggs:
                lost[d] = lost.get(d, 0) + 1      # updateUnscheduledAggNode(−1)
    arcs = {k: a for k, a in arcs.items() if k[0] not in gone and k[1] not in gone}
    urecs, crecs = [], []
    for (u, v), (lo, cap, co, ty) in sorted(arcs.items()):
        if v in sink and lost.get(u, 0):
            new = cap - lost[u]
            if new < lo:
                raise BelowLowerBound((u, v, new, lo))
            urecs.append((u, v, lo if new else 0, new, co, ty))
    if resource_caps:
        assert len(sink) == 1, "resource capacities need exactly one sink"
        pu_slots = {s: c for (s, d), (lo, c, co, ty) in arcs.items() if d in sink and ntype[s - 1] == PU}
        pu_running: dict[int, int] = {}
        for (s, d), (lo, c, co, ty) in arcs.items():
            if ty == 1:
                pu_running[d] = pu_running.get(d, 0) + 1
        live_types = [t if (alive is None or i + 1 in alive) and i + 1 not in gone else -1 for i, t in enumerate(ntype)]
        slots, running = topology_sums(live_types, arcs, pu_slots, {} if preemptive else pu_running)
        for (u, v), (lo, cap, co, ty) in sorted(arcs.items()):
            tv = ntype[v - 1]
            if ntype[u - 1] == TASK or tv == SINK:
                continue
            if tv in (PU, MACHINE, INTERMEDIATE) or (tv == OTHER and slots.get(v, 0) > 0):
                new = slots.get(v, 0) - (0 if preemptive else running.get(v, 0))
                if new < lo:
                    raise BelowLowerBound((u, v, new, lo))
                if new != cap:
                    crecs.append((u, v, lo if new else 0, new, co, ty))
    recs = sorted(urecs + crecs)
    for u, v, lo, new, co, ty in recs:
        if new:
            arcs[(u, v)] = (lo, new, co, ty)
        else:
            del arcs[(u, v)]                      # capacity 0 removes the arc
    stream = np.zeros(len(removed) + len(recs), DELTA_DT)
    for x, i in zip(stream, removed):
        x["kind"], x["id"] = KS_REMOVE_NODE, i
    for x, (u, v, lo, new, co, ty) in zip(stream[len(removed):], recs):
        x["kind"], x["type"], x["src"], x["dst"] = KS_UPDATE_ARC, ty, u, v
        x["low"], x["cap"], x["cost"], x["old_cost"] = lo, new, co, co
    stats = dict(tasks=len(removed), bound=bound, arcs_removed=n_before - len(arcs), unsched_updates=len(urecs),
                 cap_updates=len(crecs), records=len(removed) + len(recs))
    return Completion(arcs, left, removed, bind, stream, stats)


def parent_chains(ntype, arcs: dict, pus) -> list:
    """The pinned recipe's second step: the arcs of the PUs' parent chains, found in a table
    that still holds them (the caller's own topology), child first: [(src, dst), ...]."""
    into: dict[int, list[int]] = {}
    for (s, d) in arcs:
        if ntype[s - 1] != TASK and ntype[d - 1] in (PU, MACHINE, INTERMEDIATE, OTHER):
            into.setdefault(d, []).append(s)
    out, seen = [], set()
    front = sorted({int(p) for p in pus if p})
    while front:
        nxt = []
        for v in front:
            for u in into.get(v, ()):
                if (u, v) not in seen:
                    seen.add((u, v))
                    out.append((u, v))
                    nxt.append(u)
        front = sorted(set(nxt))
    return out


def chain_upserts(topology: dict, chain, cap: int = 1) -> np.ndarray:
    """ADD_ARC upserts (any positive capacity) of the chain's arcs, bounds and costs from the
    caller's topology table."""
    recs = np.zeros(len(chain), DELTA_DT)
    for x, (u, v) in zip(recs, chain):
        lo, _, co, ty = topology[(u, v)]
        x["kind"], x["type"], x["src"], x["dst"], x["low"], x["cap"], x["cost"] = KS_ADD_ARC, ty, u, v, lo, max(cap, lo), co
    return recs
