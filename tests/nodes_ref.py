"""The rule of ks_update_nodes (include/ksmcmf.h) restated on the host: the arc table in
arc-slot order (the order of ks_get_graph), the node types, the tails, one list of (head, cost,
cap) per tail and the flag in; the exact ks_delta stream, the statistics and the arcs after out.
It follows the class and resource part of AddOrUpdateJobNodes → updateFlowGraph
(flowmanager/graph_manager.go:1012-1033): updateEquivClassNode (:931-1010), AddArc(0, cap, cost)
or ChangeArc(low kept, cap, cost) per preferred arc and then removeInvalidECPrefArcs /
removeInvalidPrefResArcs (:732-790), and updateResourceNode → updateResOutgoingArcs (:1094-1111)
with updateResToSinkArc (:1116-1129), which delete nothing. The stream's order is the contract's:
the records on held arcs in arc-slot order, then the new arcs in input order. Every refusal
raises, in the order the library finds them: the flag, the tails in input order, the arcs' form
in input order (on one arc the head, the repeat, the cost, the capacity), then the arcs against
the store in input order (KS_CAP_KEEP on an arc it does not hold, a capacity below a lower
bound). Test infrastructure: no product code uses it."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from commit_ref import INTERMEDIATE, MACHINE, OTHER, PU, SINK, TASK
from remove_ref import DELTA_DT, BelowLowerBound

KS_ADD_ARC, KS_UPDATE_ARC = 2, 3
KEEP_UNLISTED = 1
CAP_KEEP = (1 << 64) - 1
MAX_COST = 1 << 40
MAX_CAP = 1 << 53
TAILS = (OTHER, MACHINE, INTERMEDIATE, PU)
STAT_KEYS = ("nodes", "arcs_added", "arcs_updated", "arcs_unchanged", "arcs_skipped", "arcs_zeroed", "arcs_removed",
             "records")


class OutOfRange(ValueError):
    """KS_E_RANGE: a cost beyond ±2^40 or a capacity beyond 2^53 (args: the tail, the head)."""


class InvalidNodes(ValueError):
    """KS_E_INVALID (args[0]: the tail named, None when none is; args[1]: the head, if any)."""


class NodeRefresh(NamedTuple):
    arcs: dict          # {(src, dst): (low, cap, cost, type)} after the call, in arc-table order
    stream: np.ndarray  # the records in the contract's order (DELTA_DT)
    stats: dict         # ks_node_stats


def nodes_reference(ntype, table: dict, nodes, lists, flags: int = 0, alive=None) -> NodeRefresh:
    """ntype: node types by id − 1 (alive: the live ids, default all). table: {(src, dst): (low,
    cap, cost, type)} in arc-slot order. lists[i]: tail i's (head, cost, cap) triples; cap may be
    CAP_KEEP. Raises InvalidNodes, OutOfRange or BelowLowerBound (args: the tail, the head)."""
    assert len(nodes) == len(lists)
    if flags & ~KEEP_UNLISTED:
        raise InvalidNodes(None)
    ntype = [int(t) for t in ntype]
    n = len(ntype)
    live = set(range(1, n + 1)) if alive is None else set(alive)
    arcs = dict(table)
    st = dict.fromkeys(STAT_KEYS, 0)
    if not nodes:
        return NodeRefresh(arcs, np.zeros(0, DELTA_DT), st)
    mine: list = []
    for u in nodes:
        u = int(u)
        if u < 1 or u > n or u not in live or ntype[u - 1] not in TAILS or u in mine:
            raise InvalidNodes(u)
        mine.append(u)
    for u, lst in zip(mine, lists):
        heads = set()
        tt = ntype[u - 1]
        for d, c, cap in lst:
            d, c, cap = int(d), int(c), int(cap)
            if d < 1 or d > n or d not in live or ntype[d - 1] == TASK or d == u:
                raise InvalidNodes(u, d)
            if ntype[d - 1] == SINK and tt not in (PU, OTHER):    # only a PU or a type-0 node reaches a sink
                raise InvalidNodes(u, d)
            if tt == PU and ntype[d - 1] != SINK:                 # a PU's only head is a sink
                raise InvalidNodes(u, d)
            if d in heads:                                        # the diff needs a set
                raise InvalidNodes(u, d)
            heads.add(d)
            if abs(c) > MAX_COST:
                raise OutOfRange(u, d)
            if cap != CAP_KEEP and cap > MAX_CAP:
                raise OutOfRange(u, d)
    listed = {}
    for u, lst in zip(mine, lists):                               # the store's answers, in input order
        for d, c, cap in lst:
            d, c, cap = int(d), int(c), int(cap)
            if (u, d) not in arcs:
                if cap == CAP_KEEP:
                    raise InvalidNodes(u, d)                      # there is nothing to keep
            else:
                lo, old, _, _ = arcs[(u, d)]
                cap = old if cap == CAP_KEEP else cap
                if cap < lo:
                    raise BelowLowerBound(u, d)
            listed[(u, d)] = (c, cap)
    keep = bool(flags & KEEP_UNLISTED)
    st["nodes"] = len(mine)
    rows = []
    own = set(mine)
    for (s, d), (lo, cap, co, ty) in arcs.items():                # the held arcs, in arc-slot order
        if s not in own:
            continue
        if (s, d) in listed:
            c, new = listed[(s, d)]
            if new == 0:                                          # (low is 0 here) a capacity of 0 is an absent arc
                rows.append((KS_UPDATE_ARC, ty, 0, s, d, 0, 0, co, co, 0))
                st["arcs_zeroed"] += 1
            elif (c, new) == (co, cap):                           # ChangeArc logs nothing
                st["arcs_unchanged"] += 1
            else:
                rows.append((KS_UPDATE_ARC, ty, 0, s, d, lo, new, c, co, 0))
                st["arcs_updated"] += 1
        elif ntype[s - 1] == OTHER and ntype[d - 1] != SINK and not keep:
            rows.append((KS_UPDATE_ARC, ty, 0, s, d, 0, 0, co, co, 0))   # no longer preferred (:732-790)
            st["arcs_removed"] += 1
    for (u, d), (c, cap) in listed.items():                       # the new arcs, in input order
        if (u, d) in arcs:
            continue
        if cap == 0:
            st["arcs_skipped"] += 1
        else:
            rows.append((KS_ADD_ARC, 0, 0, u, d, 0, cap, c, 0, 0))
            st["arcs_added"] += 1
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
    return NodeRefresh(arcs, stream, st)


def offsets3(lists) -> tuple:
    """The C-ABI's form of the lists: (arc_off, dst, cost, cap)."""
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = [x for lst in lists for x in lst]
    dst = np.asarray([int(x[0]) for x in flat], np.uint64)
    cost = np.asarray([int(x[1]) for x in flat], np.int64)
    cap = np.asarray([int(x[2]) for x in flat], np.uint64)
    return off, dst, cost, cap
