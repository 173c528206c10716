"""The rule of ks_add_resources (include/ksmcmf.h) restated on the host: a graph table, the
new resource nodes (id, type, slots, sink_cost) and the edges (parent, child, cost, kind) in;
the exact ks_delta stream, the statistics and the graph after out. It follows
AddResourceTopology (flowmanager/graph_manager.go:238-251) → addResourceTopologyDFS (:557-630)
with addResourceNode (:528-551), updateResToSinkArc (:1116-1129) and
capacityFromResNodeToParent (:662-667), and updateResourceStatsUpToRoot (:1041-1061) for the
arcs above the attach point. The stream's order is the contract's: the ADD_NODE records in
input order, the PU → sink arcs in input order of the PUs, one record per edge that gets one in
input order. Every refusal raises, in the order the library finds them: the nodes in input
order (the id, the type, the values), the summed slots, the sink count, the first offending
edge in input order (parent, child, parent == child, kind, a live node moved, cost, a repeated
pair, a second tree parent), the first PU whose walk does not end, the first edge whose raised
capacity leaves the range. Test infrastructure: no product code uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import INTERMEDIATE, MACHINE, OTHER, PU, SINK, TASK, arc_table
from remove_ref import DELTA_DT

KS_ADD_NODE, KS_ADD_ARC, KS_UPDATE_ARC = 0, 2, 3
TREE, EXTRA = 0, 1
MAX_DEPTH = 32
MAX_ID = 1 << 30
MAX_COST = 1 << 40
MAX_CAP = 1 << 53
STAT_KEYS = ("nodes", "pus", "slots", "sink_arcs", "arcs_added", "cap_updates", "arcs_skipped", "records")


class OutOfRange(ValueError):
    """KS_E_RANGE (args[0]: the node id or the (parent, child) named, None when none is)."""


class InvalidGrowth(ValueError):
    """KS_E_INVALID (args[0]: the node id or the (parent, child) named, None when none is;
    args[1]: what was wrong)."""


class Growth(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call
    ntype: list         # node types after the call, by id − 1
    supply: list        # supplies after the call
    alive: set          # live ids after the call
    stream: np.ndarray  # the records in the contract's order (DELTA_DT)
    stats: dict         # ks_grow_stats
    S: dict             # {node: the new slots beneath it} (only nodes with some)


def grow_reference(g, nodes, edges, alive=None) -> Growth:
    """g: a gen.Graph (alive: its live node ids, default all). nodes: (id, type, slots,
    sink_cost); edges: (parent, child, cost, kind)."""
    ntype = [int(t) for t in g.ntype]
    supply = [int(s) for s in g.supply]
    n0 = len(ntype)
    live = set(range(1, n0 + 1)) if alive is None else set(alive)
    arcs = arc_table(g)
    nodes = [tuple(int(v) for v in x) for x in nodes]
    edges = [tuple(int(v) for v in x) for x in edges]
    if not nodes and not edges:
        return Growth(arcs, ntype, supply, live, np.zeros(0, DELTA_DT), dict.fromkeys(STAT_KEYS, 0), {})
    new: dict = {}
    total = 0
    for i, ty, slots, co in nodes:
        if i < 1 or i >= MAX_ID:
            raise OutOfRange(i)
        if i in live or i in new:                     # a live node, or listed twice: "already present"
            raise InvalidGrowth(i, "present")
        if ty not in (PU, MACHINE, INTERMEDIATE, OTHER):
            raise InvalidGrowth(i, "type")
        if (slots == 0) if ty == PU else (slots != 0 or co != 0):
            raise InvalidGrowth(i, "values")
        if slots > MAX_CAP or abs(co) > MAX_COST:
            raise OutOfRange(i)
        total += slots
        if total > MAX_CAP:
            raise OutOfRange(i)
        new[i] = ty
    sinks = {i for i in live if ntype[i - 1] == SINK}
    if PU in new.values() and len(sinks) != 1:
        raise InvalidGrowth(None, "sink")

    def kind_of(i):                                   # the type as the call sees it, None: no node
        if i in new:
            return new[i]
        return ntype[i - 1] if 1 <= i <= n0 and i in live else None

    par: dict = {}
    pairs = set()
    for p, c, co, kind in edges:
        tp, tc = kind_of(p), kind_of(c)
        if tp is None or tp in (TASK, SINK, PU):
            raise InvalidGrowth((p, c), "parent")
        if tc is None or tc in (TASK, SINK):
            raise InvalidGrowth((p, c), "child")
        if p == c:
            raise InvalidGrowth((p, c), "loop")
        if kind not in (TREE, EXTRA):
            raise InvalidGrowth((p, c), "kind")
        if kind == TREE and p in new and c not in new:
            raise InvalidGrowth((p, c), "moves")
        if abs(co) > MAX_COST:
            raise OutOfRange((p, c))
        if (p, c) in pairs:
            raise InvalidGrowth((p, c), "pair")
        pairs.add((p, c))
        if kind == TREE:
            if c in par:
                raise InvalidGrowth((p, c), "second parent")
            par[c] = p
    S: dict = {}
    for i, ty, slots, _ in nodes:
        if ty != PU:
            continue
        v, steps = i, 0
        S[v] = S.get(v, 0) + slots
        while v in par:
            v, steps = par[v], steps + 1
            if steps > MAX_DEPTH:
                raise InvalidGrowth(i, "depth")
            S[v] = S.get(v, 0) + slots
    sink = next(iter(sinks)) if len(sinks) == 1 else 0
    rows = [(KS_ADD_NODE, ty, i, 0, 0, 0, 0, 0, 0, 0) for i, ty, _, _ in nodes]
    rows += [(KS_ADD_ARC, 0, 0, i, sink, 0, slots, co, 0, 0) for i, ty, slots, co in nodes if ty == PU]
    pus = len(rows) - len(nodes)
    add = upd = skipped = 0
    for p, c, co, _ in edges:
        s = S.get(c, 0)
        if s == 0:                                    # a capacity of 0 is an absent arc
            skipped += 1
        elif c not in new and (p, c) in arcs:         # low, cost and type kept, the capacity raised
            lo, cap, co0, ty = arcs[(p, c)]
            if cap + s > MAX_CAP:
                raise OutOfRange((p, c))
            rows.append((KS_UPDATE_ARC, ty, 0, p, c, lo, cap + s, co0, co0, 0))
            upd += 1
        else:
            rows.append((KS_ADD_ARC, 0, 0, p, c, 0, s, co, 0, 0))
            add += 1
    stream = np.zeros(len(rows), DELTA_DT)
    for name, col in zip(DELTA_DT.names, zip(*rows)):
        stream[name] = np.asarray(col, dtype=DELTA_DT[name])
    top = max([n0] + list(new))
    ntype += [0] * (top - n0)
    supply += [0] * (top - n0)
    for i, ty in new.items():
        ntype[i - 1], supply[i - 1] = ty, 0
    for kind, ty, _, s, d, lo, cap, co, _, _ in rows[len(nodes):]:
        arcs[(s, d)] = (lo, cap, co, ty)
    stats = dict(nodes=len(nodes), pus=pus, slots=total, sink_arcs=pus, arcs_added=add, cap_updates=upd,
                 arcs_skipped=skipped, records=len(rows))
    return Growth(arcs, ntype, supply, live | set(new), stream, stats, {v: s for v, s in S.items() if s})


def chain(parents: dict, node, costs=None) -> list:
    """The KS_RES_TREE edges from node up to the topology's root, child first (Go's
    nodeToParentNode walked as updateResourceStatsUpToRoot does): parents {child: parent}."""
    out = []
    while node in parents:
        p = parents[node]
        out.append((p, node, 0 if costs is None else costs.get((p, node), 0), TREE))
        node = p
    return out


def tree_parents(ntype, arcs: dict, extra=()) -> dict:
    """{child: parent} of a graph table: every arc between nodes that are no task and no sink,
    but those out of the nodes in `extra` (equivalence classes), is a ParentId edge."""
    out = {}
    for (s, d) in arcs:
        if ntype[s - 1] in (TASK, SINK) or ntype[d - 1] in (TASK, SINK) or s in extra:
            continue
        assert d not in out, "a resource has one parent"
        out[d] = s
    return out
