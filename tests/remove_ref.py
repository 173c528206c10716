"""The rule of ks_remove_resources (include/ksmcmf.h) restated on the host: a graph, the
roots and the bindings in; the arc table, the removed ids, the evictions, the bindings
and the equivalent ks_delta stream out. It follows DeregisterResource
(flowscheduler/scheduler.go:162-210): dfsEvictTasks (:533-566) → TaskEvicted
(flowmanager/graph_manager.go:412-433) for every task bound in the subtree,
RemoveResourceTopology (:362-387) with traverseAndRemoveTopology (:829-844) for its
nodes, and the capacity rule of the two commits (capacityFromResNodeToParent, :662-667)
over the sums of ComputeTopologyStatistics (:480-511) on the graph without the subtree.
Test infrastructure: no product code uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import INTERMEDIATE, MACHINE, OTHER, PU, SINK, TASK, arc_table, topology_sums

KS_REMOVE_NODE, KS_UPDATE_ARC = 1, 3
PREEMPT = 1
DELTA_DT = np.dtype({"names": ["kind", "type", "id", "src", "dst", "low", "cap", "cost", "old_cost", "excess"],
                     "formats": ["<i4", "<i4", "<u8", "<u8", "<u8", "<u8", "<u8", "<i8", "<i8", "<i8"],
                     "offsets": [0, 4, 8, 16, 24, 32, 40, 48, 56, 64], "itemsize": 72})
STAT_KEYS = ("roots", "nodes_removed", "pus_removed", "tasks_evicted", "arcs_removed", "cap_updates", "records")


class InvalidRoot(ValueError):
    """KS_E_INVALID: a root that is dead, beyond the graph, a task or a sink."""


class BelowLowerBound(ValueError):
    """KS_E_VERIFY: a capacity would fall below its arc's lower bound."""


class Removal(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call
    removed: list       # removed ids, ascending
    evicted: list       # (task, pu) in task order
    bindings: dict      # {task: pu} after the call
    stream: np.ndarray  # the "r id" records, then the "x" capacity records (DELTA_DT)
    stats: dict         # ks_remove_stats


def subtree(ntype, arcs, roots, alive=None) -> list:
    """traverseAndRemoveTopology: the roots and everything reached from them along arcs
    into PUs, machines and intermediate nodes."""
    n = len(ntype)
    for r in roots:
        r = int(r)
        if r < 1 or r > n or (alive is not None and r not in alive) or ntype[r - 1] in (TASK, SINK):
            raise InvalidRoot(r)
    out: dict[int, list[int]] = {}
    for s, d in arcs:
        out.setdefault(s, []).append(d)
    seen = {int(r) for r in roots}
    front = sorted(seen)
    while front:
        nxt = []
        for u in front:
            for v in out.get(u, ()):
                if v not in seen and ntype[v - 1] in (PU, MACHINE, INTERMEDIATE):
                    seen.add(v)
                    nxt.append(v)
        front = nxt
    return sorted(seen)


def remove_reference(g, roots, bindings: dict, resource_caps: bool, preemptive: bool, alive=None) -> Removal:
    """g: a gen.Graph (alive: its live node ids, default all). bindings {task: pu}."""
    assert resource_caps or not preemptive
    ntype = [int(t) for t in g.ntype]
    arcs = arc_table(g)
    n_before = len(arcs)
    removed = subtree(ntype, arcs, roots, alive)
    gone = set(removed)
    bind = {int(t): int(p) for t, p in bindings.items() if p}
    evicted = [(t, bind[t]) for t in sorted(bind) if bind[t] in gone]   # dfsEvictTasks
    for t, _ in evicted:
        del bind[t]
    arcs = {k: a for k, a in arcs.items() if k[0] not in gone and k[1] not in gone}
    recs = []
    if resource_caps:
        sink = {i + 1 for i, t in enumerate(ntype) if t == SINK and (alive is None or i + 1 in alive)}
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
                    recs.append((u, v, lo if new else 0, new, co, ty))
        for u, v, lo, new, co, ty in recs:
            if new:
                arcs[(u, v)] = (lo, new, co, ty)
            else:
                del arcs[(u, v)]            # capacity 0 removes the arc
    stream = np.zeros(len(removed) + len(recs), DELTA_DT)
    for x, i in zip(stream, removed):
        x["kind"], x["id"] = KS_REMOVE_NODE, i
    for x, (u, v, lo, new, co, ty) in zip(stream[len(removed):], recs):
        x["kind"], x["type"], x["src"], x["dst"] = KS_UPDATE_ARC, ty, u, v
        x["low"], x["cap"], x["cost"], x["old_cost"] = lo, new, co, co
    stats = dict(roots=len({int(r) for r in roots}), nodes_removed=len(removed),
                 pus_removed=sum(1 for i in removed if ntype[i - 1] == PU), tasks_evicted=len(evicted),
                 arcs_removed=n_before - len(arcs), cap_updates=len(recs), records=len(removed) + len(recs))
    return Removal(arcs, removed, evicted, bind, stream, stats)


# ---- the toy shared by the CPU and the GPU suite ----------------------------------
# 2 racks × 2 machines × 1 PU of 2 slots, 6 tasks of one job, four tasks running on three
# PUs (their running arcs: type 1, low 0).
# SINK 1, X 2, R1 3, R2 4, M1..M4 5..8 (M1, M2 in R1), P1..P4 9..12, U 13, T1..T6 14..19
TOY_NTYPE = [3, 0, 0, 0, 4, 4, 4, 4, 2, 2, 2, 2, 0, 1, 1, 1, 1, 1, 1]
TOY_SUPPLY = [-6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
TOY_ARCS = {(2, 3): (0, 4, 0, 0), (2, 4): (0, 4, 0, 0),
            (3, 5): (0, 2, 0, 0), (3, 6): (0, 2, 0, 0), (4, 7): (0, 2, 0, 0), (4, 8): (0, 2, 0, 0),
            (5, 9): (0, 2, 0, 0), (6, 10): (0, 2, 0, 0), (7, 11): (0, 2, 0, 0), (8, 12): (0, 2, 0, 0),
            (9, 1): (0, 2, 0, 0), (10, 1): (0, 2, 0, 0), (11, 1): (0, 2, 0, 0), (12, 1): (0, 2, 0, 0),
            (13, 1): (0, 6, 0, 0),
            **{(t, 13): (0, 1, 100 + t, 0) for t in range(14, 20)},
            **{(t, 2): (0, 1, 40 + t, 0) for t in range(14, 20)},
            (14, 5): (0, 1, 3, 0), (15, 3): (0, 1, 9, 0), (18, 5): (0, 1, 4, 0), (19, 8): (0, 1, 5, 0),
            (18, 6): (0, 1, 6, 0),
            (14, 9): (0, 1, 0, 1), (15, 9): (0, 1, 0, 1), (16, 10): (0, 1, 0, 1), (17, 11): (0, 1, 0, 1)}
TOY_BINDINGS = {14: 9, 15: 9, 16: 10, 17: 11}
TOY_M1, TOY_R1, TOY_U = 5, 3, 13
