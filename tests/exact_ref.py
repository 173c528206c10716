"""An exact min-cost-flow reference in plain Python integers.

TEST INFRASTRUCTURE ONLY. The C oracle (oracle/ks_oracle.c) and the library both
compute in int64, so neither can referee a total beyond 2^63, and the oracle's SSP
refuses negative costs. This one uses Python's arbitrary-precision ``int`` for every
value (numpy arrays are only read, through ``tolist``) and accepts lower bounds,
supplies, negative costs and negative-cost cycles.

Method: every arc starts at ``cap`` if its cost is negative, else at ``low``. The
residual graph then has no arc of negative cost, so zero potentials are valid, and
the excesses this start leaves are removed by successive shortest paths (Dijkstra
on reduced costs) until none is left or no deficit can be reached. A flow without
a negative residual cycle that meets every supply is optimal.

Node ids may be sparse: only nodes that carry a supply or an arc are visited.
"""
from __future__ import annotations

import heapq


def _lists(g):
    """(supply, src, dst, low, cap, cost) of a gen.Graph as lists of Python ints."""
    return tuple([int(x) for x in a.tolist()] for a in (g.supply, g.src, g.dst, g.low, g.cap, g.cost))


def mcf(g):
    """→ (feasible, cost, flows): the exact optimum of g (gen.Graph, 1-based ids,
    supply[i − 1] the excess of node i), flows per arc of g in g's order. An
    infeasible g gives (False, None, None)."""
    supply, src, dst, low, cap, cost = _lists(g)
    m = len(src)
    if sum(supply) != 0:
        return False, None, None
    for i in range(m):
        if low[i] > cap[i] or low[i] < 0:
            return False, None, None
    # residual arcs 2i (forward) and 2i + 1 (backward) of arc i
    head = [0] * (2 * m)
    res = [0] * (2 * m)
    rcost = [0] * (2 * m)
    adj: dict[int, list[int]] = {}
    excess: dict[int, int] = {v + 1: s for v, s in enumerate(supply) if s}
    for i in range(m):
        f0 = cap[i] if cost[i] < 0 else low[i]
        head[2 * i], head[2 * i + 1] = dst[i], src[i]
        res[2 * i], res[2 * i + 1] = cap[i] - f0, f0 - low[i]
        rcost[2 * i], rcost[2 * i + 1] = cost[i], -cost[i]
        adj.setdefault(src[i], []).append(2 * i)
        adj.setdefault(dst[i], []).append(2 * i + 1)
        if f0:
            excess[src[i]] = excess.get(src[i], 0) - f0
            excess[dst[i]] = excess.get(dst[i], 0) + f0
    pot: dict[int, int] = {}
    while True:
        sources = [v for v, e in excess.items() if e > 0]
        if not sources:
            break
        # Dijkstra on reduced costs from every excess node to the nearest deficit
        dist = {v: 0 for v in sources}
        parent: dict[int, int] = {}
        heap = [(0, v) for v in sources]
        heapq.heapify(heap)
        done = set()
        target = None
        while heap:
            d, v = heapq.heappop(heap)
            if v in done:
                continue
            done.add(v)
            if excess.get(v, 0) < 0:
                target = v
                break
            pv = pot.get(v, 0)
            for a in adj.get(v, ()):
                if res[a] <= 0:
                    continue
                w = head[a]
                if w in done:
                    continue
                rc = rcost[a] + pv - pot.get(w, 0)
                assert rc >= 0, "reduced cost went negative: the reference itself is broken"
                nd = d + rc
                if nd < dist.get(w, nd + 1):
                    dist[w] = nd
                    parent[w] = a
                    heapq.heappush(heap, (nd, w))
        if target is None:
            return False, None, None
        dt = dist[target]
        for v in done:   # settled nodes have dist ≤ dt; the others keep their potential (+ 0 after the shift)
            pot[v] = pot.get(v, 0) + dist[v] - dt
        path = []
        v = target
        while v in parent:
            a = parent[v]
            path.append(a)
            v = head[a ^ 1]
        amount = min(excess[v], -excess[target], min(res[a] for a in path))
        for a in path:
            res[a] -= amount
            res[a ^ 1] += amount
        excess[v] -= amount
        excess[target] += amount
    if any(excess.values()):
        return False, None, None
    flows = [cap[i] - res[2 * i] for i in range(m)]
    return True, sum(f * c for f, c in zip(flows, cost)), flows


def flow_value(g, flows) -> int:
    """Net inflow into the demand nodes (supply < 0): the library's flow_value."""
    supply, src, dst, _, _, _ = _lists(g)
    fv = 0
    for s, d, f in zip(src, dst, flows):
        if supply[d - 1] < 0:
            fv += int(f)
        if supply[s - 1] < 0:
            fv -= int(f)
    return fv


def per_arc(g, flows) -> list[int]:
    """flows as one Python int per arc of g: either already that (a sequence of g.m
    numbers) or ks_flow records (fields src, dst, flow; arcs without flow absent)."""
    names = getattr(getattr(flows, "dtype", None), "names", None)
    if not names:
        out = [int(x) for x in (flows.tolist() if hasattr(flows, "tolist") else flows)]
        assert len(out) == g.m, "one flow per arc expected"
        return out
    idx = {}
    for i, key in enumerate(zip(g.src.tolist(), g.dst.tolist())):
        assert key not in idx, f"parallel arcs {key}: flow records cannot tell them apart"
        idx[key] = i
    out = [0] * g.m
    seen = set()
    for s, d, f in zip(flows["src"].tolist(), flows["dst"].tolist(), flows["flow"].tolist()):
        assert (s, d) in idx, f"flow on an arc {s}->{d} the graph does not have"
        assert (s, d) not in seen, f"two flow records for arc {s}->{d}"
        seen.add((s, d))
        out[idx[(s, d)]] = int(f)
    return out


def check_flows(g, flows) -> int:
    """Capacity (low ≤ f ≤ cap) and conservation (supply + inflow − outflow = 0 at
    every node) of flows, in Python ints; → Σ flow · cost. AssertionError otherwise."""
    supply, src, dst, low, cap, cost = _lists(g)
    f = per_arc(g, flows)
    bal = {v + 1: s for v, s in enumerate(supply) if s}
    for i in range(len(src)):
        assert low[i] <= f[i] <= cap[i], f"arc {src[i]}->{dst[i]}: flow {f[i]} outside [{low[i]}, {cap[i]}]"
        if f[i]:
            bal[src[i]] = bal.get(src[i], 0) - f[i]
            bal[dst[i]] = bal.get(dst[i], 0) + f[i]
    off = {v: b for v, b in bal.items() if b}
    assert not off, f"conservation violated at {sorted(off.items())[:5]}"
    return sum(x * c for x, c in zip(f, cost))
