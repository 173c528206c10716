"""The rule of ks_commit_schedule (include/ksmcmf.h) restated on the host: a graph
and the placements in, the arc table out. It follows what the reference does after
applySchedulingDeltas with Preemption == false — pinTaskToNode
(flowmanager/graph_manager.go:675-720), updateUnscheduledAggNode(-1) (:706,
:1291-1305) and capacityFromResNodeToParent (:662-667) over the sums of
ComputeTopologyStatistics (:480-511). Test infrastructure: no product code uses it."""
from __future__ import annotations

TASK, PU, SINK, MACHINE, INTERMEDIATE, OTHER = 1, 2, 3, 4, 5, 0
ACCUM = (PU, MACHINE, INTERMEDIATE, OTHER)


def arc_table(g) -> dict:
    """{(src, dst): (low, cap, cost, type)} of a gen.Graph, capacity-0 arcs included."""
    t = g.arc_types()
    return {(int(s), int(d)): (int(lo), int(c), int(co), int(ty))
            for s, d, lo, c, co, ty in zip(g.src, g.dst, g.low, g.cap, g.cost, t)}


def topology_sums(ntype, arcs, pu_slots, pu_running):
    """Level-synchronous BFS from the sink over in-arcs, as ks_topology_stats: a PU
    reached from the sink takes its own (slots, running); every accumulating node
    adds the sums of each expanded resource node it has an arc into."""
    into: dict[int, list[int]] = {}
    for s, d in arcs:
        into.setdefault(d, []).append(s)
    sinks = [i + 1 for i, t in enumerate(ntype) if t == SINK]
    slots: dict[int, int] = {}
    running: dict[int, int] = {}
    if len(sinks) != 1:
        return slots, running
    seen = {sinks[0]}
    front = [sinks[0]]
    while front:
        nxt = []
        for x in front:
            tx = ntype[x - 1]
            for u in into.get(x, ()):
                if u not in seen:
                    seen.add(u)
                    nxt.append(u)
                tu = ntype[u - 1]
                if tu not in ACCUM:
                    continue
                if tx == SINK:
                    if tu == PU:
                        slots[u] = pu_slots.get(u, 0)
                        running[u] = pu_running.get(u, 0)
                elif tx in ACCUM:
                    slots[u] = slots.get(u, 0) + slots.get(x, 0)
                    running[u] = running.get(u, 0) + running.get(x, 0)
        front = nxt
    return slots, running


def commit_reference(g, placed: dict, continuation: int, resource_caps: bool, unsched_ids=None) -> dict:
    """The arcs of g after pinning placed = {task: pu}: {(src, dst): (low, cap, cost,
    type)} without the arcs whose capacity is 0."""
    ntype = [int(t) for t in g.ntype]
    arcs = arc_table(g)
    before = dict(arcs)
    sink = {i + 1 for i, t in enumerate(ntype) if t == SINK}
    if unsched_ids is None:
        aggs = {s for (s, d) in arcs if d in sink and ntype[s - 1] == OTHER}
    else:
        aggs = {int(a) for a in unsched_ids}
    out: dict[int, list[int]] = {}
    for s, d in arcs:
        out.setdefault(s, []).append(d)
    left = {a: 0 for a in aggs}
    for t, p in placed.items():
        for d in out.get(t, ()):
            if d in aggs:
                left[d] += 1          # one task fewer waiting in this aggregator
            if d != p:
                del arcs[(t, d)]      # DeleteArc
        arcs[(t, p)] = (1, 1, continuation, 1)   # the running arc (new, or the preference arc converted)
    for a, k in left.items():
        for z in sink:
            if k and (a, z) in arcs:
                lo, cap, co, ty = arcs[(a, z)]
                assert cap - k >= lo, "aggregator capacity below its lower bound"
                arcs[(a, z)] = (lo, cap - k, co, ty)
    if resource_caps:
        pu_slots = {s: c for (s, d), (lo, c, co, ty) in arcs.items() if d in sink and ntype[s - 1] == PU}
        pu_running: dict[int, int] = {}
        for (s, d), (lo, c, co, ty) in arcs.items():
            if ty == 1:
                pu_running[d] = pu_running.get(d, 0) + 1
        # the sums run over the graph as it stood (the pins only touch arcs out of tasks)
        slots, running = topology_sums(ntype, before, pu_slots, pu_running)
        for (u, v), (lo, cap, co, ty) in list(arcs.items()):
            tv = ntype[v - 1]
            if ntype[u - 1] == TASK or tv == SINK:
                continue
            if tv in (PU, MACHINE, INTERMEDIATE) or (tv == OTHER and slots.get(v, 0) > 0):
                new = slots.get(v, 0) - running.get(v, 0)
                assert new >= lo, "resource capacity below its lower bound"
                arcs[(u, v)] = (lo, new, co, ty)
    return {k: a for k, a in arcs.items() if a[1] > 0}
