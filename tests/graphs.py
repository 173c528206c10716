"""Test graph builders shared by the CPU and GPU suites."""
from __future__ import annotations

import numpy as np

from ksched_amd import gen


def graph_from_lists(nodes, arcs):
    """nodes: [(id, excess, dimacs_type)], arcs: [(src, dst, low, cap, cost)] (1-based ids)."""
    n = max(i for i, _, _ in nodes) if len(nodes) else 0
    ntype = np.zeros(n, np.int32)
    supply = np.zeros(n, np.int64)
    for i, e, t in nodes:
        ntype[i - 1] = t
        supply[i - 1] = e
    a = np.asarray(arcs, np.int64).reshape(-1, 5)
    return gen.Graph(ntype, supply, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(),
                     a[:, 4].copy())


def flow_mapping(g, flow) -> dict[int, int]:
    """task → last PU on its unit's path, following positive-flow arcs (the
    scheduling network is a DAG); the test-side twin of ks_get_task_mapping."""
    out = {}
    pos = np.nonzero(np.asarray(flow) > 0)[0]
    nxt: dict[int, list] = {}
    for i in pos.tolist():
        nxt.setdefault(int(g.src[i]), []).append([int(g.dst[i]), int(flow[i])])
    for t in (np.nonzero(g.ntype == 1)[0] + 1).tolist():
        v, last = t, None
        for _ in range(g.n + 1):
            if g.ntype[v - 1] == 2:
                last = v
            lst = nxt.get(v)
            while lst and lst[0][1] == 0:
                lst.pop(0)
            if not lst:
                break
            lst[0][1] -= 1
            v = lst[0][0]
        if last is not None:
            out[t] = last
    return out


def apply_deltas_to_arcs(nodes: dict, arcs: dict, deltas) -> None:
    """Test-side restatement of the graph-store semantics of ks_apply_deltas
    (include/ksmcmf.h): nodes {id: [excess, type]}, arcs {(s, d): (low, cap, cost)}."""
    for x in deltas:
        k = int(x["kind"])
        if k == 0:
            assert int(x["id"]) not in nodes
            nodes[int(x["id"])] = [int(x["excess"]), int(x["type"])]
        elif k == 1:
            i = int(x["id"])
            del nodes[i]
            for key in [a for a in arcs if i in a]:
                del arcs[key]
        elif k == 2:
            s, d = int(x["src"]), int(x["dst"])
            assert s in nodes and d in nodes
            arcs[(s, d)] = (int(x["low"]), int(x["cap"]), int(x["cost"]))
        elif k == 3:
            s, d = int(x["src"]), int(x["dst"])
            if int(x["low"]) == 0 and int(x["cap"]) == 0:
                arcs.pop((s, d), None)
            else:
                arcs[(s, d)] = (int(x["low"]), int(x["cap"]), int(x["cost"]))
        else:
            nodes[int(x["id"])][0] = int(x["excess"])


def dimacs_changes(deltas) -> str:
    """ks_delta records as the incremental DIMACS text of dimacs/*_change.go
    (GenerateChange), terminated by "c EOI" (dimacs/export.go:31-38)."""
    out = []
    for x in deltas:
        k = int(x["kind"])
        if k == 0:
            out.append(f"n {int(x['id'])} {int(x['excess'])} {int(x['type'])}")
        elif k == 1:
            out.append(f"r {int(x['id'])}")
        elif k == 2:
            out.append(f"a {int(x['src'])} {int(x['dst'])} {int(x['low'])} {int(x['cap'])} {int(x['cost'])} "
                       f"{int(x['type'])}")
        elif k == 3:
            out.append(f"x {int(x['src'])} {int(x['dst'])} {int(x['low'])} {int(x['cap'])} {int(x['cost'])} "
                       f"{int(x['type'])} {int(x['old_cost'])}")
        else:
            raise ValueError("SET_EXCESS has no DIMACS record")
    out.append("c EOI")
    return "\n".join(out) + "\n"


def graph_from_store(nodes: dict, arcs: dict):
    n = max(nodes) if nodes else 0
    ntype = np.zeros(n, np.int32)
    supply = np.zeros(n, np.int64)
    for i, (e, t) in nodes.items():
        ntype[i - 1] = t
        supply[i - 1] = e
    sink = np.nonzero(ntype == 3)[0]
    if sink.shape[0] == 1:                  # auto_sink: the sink absorbs every other supply
        supply[sink[0]] = 0
        supply[sink[0]] = -int(supply.sum())
    keys = sorted(arcs)
    a = np.asarray([(s, d, *arcs[(s, d)]) for s, d in keys], np.int64).reshape(-1, 5)
    return gen.Graph(ntype, supply, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(),
                     a[:, 4].copy())


def random_graphs(seed: int, count: int, max_n: int = 60, cost_lo: int = 0, cost_hi: int = 100):
    """General digraphs (cycles, antiparallel arcs, zero capacities, some lower
    bounds) with a few random balanced supply/demand pairs; may be infeasible."""
    rng = np.random.default_rng(seed)
    for trial in range(count):
        n = int(rng.integers(4, max_n))
        m = min(int(rng.integers(n, 6 * n)), n * (n - 1) // 2)
        pairs = set()
        arcs = []
        while len(arcs) < m:
            s, d = (int(x) for x in rng.integers(1, n + 1, 2))
            if s == d or (s, d) in pairs:
                continue
            pairs.add((s, d))
            lo = int(rng.integers(0, 2)) if rng.random() < 0.1 else 0
            cap = lo + int(rng.integers(0, 20))
            arcs.append((s, d, lo, cap, int(rng.integers(cost_lo, cost_hi))))
        supply = np.zeros(n, np.int64)
        for _ in range(int(rng.integers(1, 6))):
            a, b = (int(x) for x in rng.integers(0, n, 2))
            k = int(rng.integers(1, 10))
            supply[a] += k
            supply[b] -= k
        nodes = [(i + 1, int(supply[i]), 0) for i in range(n)]
        yield trial, graph_from_lists(nodes, arcs)


def parse_dimacs(text: str):
    """ksched's solver wire text (dimacs/export.go:11-76 for a full graph,
    dimacs/*_change.go GenerateChange for an incremental block) →
    (nodes [(id, excess, type)], arcs [(src, dst, low, cap, cost)], deltas DELTA_DT).
    A full export yields nodes/arcs, a change block yields delta records."""
    from ksched_amd import native
    nodes, arcs, recs = [], [], []
    for line in text.splitlines():
        f = line.split()
        if not f or f[0] in ("c", "p"):
            continue
        v = [int(x) for x in f[1:]]
        if f[0] == "n":
            nodes.append(tuple(v))
            recs.append(dict(kind=native.KS_ADD_NODE, id=v[0], excess=v[1], type=v[2]))
        elif f[0] == "a":
            arcs.append(tuple(v[:5]))
            recs.append(dict(kind=native.KS_ADD_ARC, src=v[0], dst=v[1], low=v[2], cap=v[3], cost=v[4],
                             type=v[5] if len(v) > 5 else 0))
        elif f[0] == "x":
            recs.append(dict(kind=native.KS_UPDATE_ARC, src=v[0], dst=v[1], low=v[2], cap=v[3], cost=v[4],
                             type=v[5], old_cost=v[6] if len(v) > 6 else 0))
        elif f[0] == "r":
            recs.append(dict(kind=native.KS_REMOVE_NODE, id=v[0]))
        else:
            raise ValueError(f"unknown DIMACS record {line!r}")
    d = np.zeros(len(recs), native.DELTA_DT)
    for i, x in enumerate(recs):
        for k, val in x.items():
            d[i][k] = val
    return nodes, arcs, d


def load_multi_schedule():
    """tests/golden/multi_schedule_iteration.json (gen_multi_schedule.py)."""
    import json
    import os
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_schedule_iteration.json")
    with open(p) as f:
        return json.load(f)["rounds"]


def same_graph(ctx, g):
    """The device-resident graph (ks_get_graph) equals g up to arcs of capacity 0
    (an "x … 0 0" record removes them from the store)."""
    nodes, arcs = ctx.graph()
    dev = sorted(zip(arcs["src"].tolist(), arcs["dst"].tolist(), arcs["low"].tolist(), arcs["cap"].tolist(),
                     arcs["cost"].tolist()))
    want = sorted(a for a in zip(g.src.tolist(), g.dst.tolist(), g.low.tolist(), g.cap.tolist(), g.cost.tolist())
                  if a[3] > 0)
    assert dev == want
    live = np.nonzero(g.ntype != 0)[0] + 1
    assert set(live.tolist()) <= set(nodes["id"].tolist())


def random_hub_graphs(seed: int, count: int, n_lo: int = 300, n_hi: int = 6000, cost_hi: int = 1000):
    """Medium general graphs for differential testing against the oracle: random
    arcs plus one to four hubs (a node joined to a quarter to all of the others,
    in both directions), a few large capacities, antiparallel
    and zero-capacity arcs, several sources and sinks. Hubs exercise the engine's
    hub chunks and inboxes and the cell solver's workgroup-wide items. Lower
    bounds of 1 sit on some arcs out of sources. Costs are
    non-negative, as in ksched's cost models (the reference's SSP assumes no
    negative cycle). Four in five graphs get expensive source → hub → sink arcs
    that make them feasible; the rest may be infeasible (then the solver must
    say so)."""
    rng = np.random.default_rng(seed)
    for trial in range(count):
        n = int(rng.integers(n_lo, n_hi))
        mb = int(rng.integers(2 * n, 6 * n))
        k = int(rng.integers(2, 40))
        ends = rng.choice(n, 2 * k, replace=False) + 1
        units = rng.integers(1, 200, k)
        hubs = rng.choice(n, int(rng.integers(1, 5)), replace=False) + 1
        src, dst = [], []
        if rng.random() < 0.8:   # feasibility arcs first: they win the de-duplication below
            src += [ends[:k], np.full(k, hubs[0])]
            dst += [np.full(k, hubs[0]), ends[k:]]
        nf = sum(x.shape[0] for x in src)
        src.append(rng.integers(1, n + 1, mb))
        dst.append(rng.integers(1, n + 1, mb))
        for h in hubs:
            deg = int(rng.integers(n // 4, n))
            other = rng.choice(n, deg, replace=False) + 1
            into = rng.random(deg) < 0.5
            src.append(np.where(into, other, h))
            dst.append(np.where(into, h, other))
        src = np.concatenate(src).astype(np.int64)
        dst = np.concatenate(dst).astype(np.int64)
        keep = src != dst
        src, dst = src[keep], dst[keep]
        _, first = np.unique(src * (n + 1) + dst, return_index=True)
        first.sort()
        src, dst = src[first], dst[first]
        m = src.shape[0]
        feas = first < nf   # (first is sorted: kept feasibility arcs come first)
        cap = rng.integers(0, 40, m)
        big = rng.random(m) < 0.03
        cap[big] = rng.integers(1000, 200000, int(big.sum()))
        # lower bounds only on arcs out of sources (as ksched's running arcs out of a
        # pinned task): anywhere else they mostly make a random graph infeasible
        low = np.zeros(m, np.int64)
        lb = np.isin(src, ends[:k]) & (cap > 0) & (rng.random(m) < 0.3)
        low[lb] = 1
        cost = rng.integers(0, cost_hi, m)
        cap[feas] = 200
        low[feas] = 0
        cost[feas] = 50 * cost_hi
        supply = np.zeros(n, np.int64)
        supply[ends[:k] - 1] += units
        supply[ends[k:] - 1] -= units
        ntype = np.zeros(n, np.int32)
        g = gen.Graph(ntype, supply, src, dst, low, cap.astype(np.int64), cost.astype(np.int64))
        g.hubs = [int(h) for h in hubs]   # (hubs[0] carries the feasibility arcs, when there are any)
        yield trial, g


# (seed, first stream applied after a first solve) of the adversarial random-stream cases
# (test_gpu_stress); test_store_ref_cpu checks on the oracle that they stay feasible
ADVERSARIAL_SEEDS = [(24, True), (31, True), (28, False)]


def random_stream(rng, nodes, arcs, nrec, hubs=(), adversarial=False):
    """A random ks_delta stream over the store state (nodes {id: [excess, type]},
    arcs {(s, d): (low, cap, cost)}), applied to that state as it is made: node
    removals (zero-supply nodes; their arcs go with them) and re-additions of the
    freed ids with new arcs, arc upserts, in-place edits, deletions (UPDATE 0/0),
    an arc deleted and re-created inside one stream (the store keeps the LAST
    record for a key), and a few units moved between two sources (SET_EXCESS
    pairs). The generator's expensive feasibility arcs are left alone, so most
    rounds stay feasible.

    adversarial: the stream also removes, a quarter of the way in, three pairs of
    adjacent zero-supply nodes (an arc with both endpoints removed) and, half way
    in, one hub of the generator (hubs[1:], never the feasibility hub hubs[0] nor an
    end of a feasibility arc; once those are gone, the eligible node of the highest
    degree): a node of hundreds of arcs removed among nodes of a few. Without the
    flag the stream is what it always was for a given rng."""
    from ksched_amd import native
    recs = []
    free_ids = []
    alive = sorted(nodes)
    keep = {x for (s, d), (_, _, c) in arcs.items() if c >= 50_000 for x in (s, d)}   # feasibility arcs' ends
    keep |= set(hubs[:1]) if adversarial else set()
    todo = [(nrec // 2, "hub"), (nrec // 4, "pairs")] if adversarial else []

    def emit(**x):
        r = np.zeros(1, native.DELTA_DT)
        for k, v in x.items():
            r[0][k] = v
        apply_deltas_to_arcs(nodes, arcs, r)
        recs.append(r[0])

    def removable(i):
        return i in nodes and nodes[i][0] == 0 and i not in keep

    def remove(i):
        emit(kind=native.KS_REMOVE_NODE, id=i)
        free_ids.append(i)

    keys = list(arcs)
    while len(recs) < nrec:
        if todo and len(recs) >= todo[-1][0]:
            if todo.pop()[1] == "pairs":
                for _ in range(3):
                    adj = [k for k in arcs if removable(k[0]) and removable(k[1]) and not set(k) & set(hubs)]
                    if adj:
                        for i in adj[int(rng.integers(0, len(adj)))]:
                            remove(i)
            else:
                deg = {}
                for k in arcs:
                    for i in k:
                        deg[i] = deg.get(i, 0) + 1
                # (a hub removed in an earlier round may be back under its id with three arcs)
                cand = [h for h in hubs[1:] if removable(h) and deg.get(h, 0) >= 64]
                if not cand:
                    cand = sorted((i for i in deg if removable(i)), key=lambda i: (-deg[i], i))[:1]
                if cand:
                    remove(cand[0])
            alive = sorted(nodes)
            continue
        op = rng.random()
        if op < 0.05:
            i = int(rng.choice(alive))
            if nodes.get(i, [1])[0] == 0 and i not in keep:
                emit(kind=native.KS_REMOVE_NODE, id=i)
                free_ids.append(i)
                alive = sorted(nodes)
        elif op < 0.10 and free_ids:
            i = free_ids.pop(0)   # FIFO id reuse (graph.go:169-182)
            emit(kind=native.KS_ADD_NODE, id=i, excess=0, type=0)
            alive = sorted(nodes)
            for j in rng.choice(alive, 3, replace=False).tolist():
                if j != i:
                    s, d = (i, j) if rng.random() < 0.5 else (j, i)
                    emit(kind=native.KS_ADD_ARC, src=s, dst=d, low=0, cap=int(rng.integers(1, 30)),
                         cost=int(rng.integers(0, 1000)))
        elif op < 0.40:
            s, d = (int(x) for x in rng.choice(alive, 2, replace=False))
            emit(kind=native.KS_ADD_ARC, src=s, dst=d, low=0, cap=int(rng.integers(0, 30)),
                 cost=int(rng.integers(0, 1000)))
        elif op < 0.90 and keys:
            s, d = keys[int(rng.integers(0, len(keys)))]
            if (s, d) not in arcs or arcs[(s, d)][2] >= 50_000:   # (the generator's feasibility arcs stay)
                continue
            low, cap, cost = arcs[(s, d)]
            r = rng.random()
            if r < 0.3:     # delete (UPDATE to 0/0), sometimes re-created later in this stream
                emit(kind=native.KS_UPDATE_ARC, src=s, dst=d, low=0, cap=0, cost=cost, old_cost=cost)
                if rng.random() < 0.3:
                    emit(kind=native.KS_ADD_ARC, src=s, dst=d, low=0, cap=int(rng.integers(1, 30)),
                         cost=int(rng.integers(0, 1000)))
            else:           # new capacity and cost in place (the flow is clamped)
                emit(kind=native.KS_UPDATE_ARC, src=s, dst=d, low=low, cap=max(low, int(rng.integers(0, 60))),
                     cost=int(rng.integers(0, 1000)), old_cost=cost)
        elif op < 0.92:    # a few units moved from one source to another
            src = [i for i in alive if nodes[i][0] > 3]
            if len(src) < 2:
                continue
            a, b = (int(x) for x in rng.choice(src, 2, replace=False))
            k = int(rng.integers(1, 4))
            emit(kind=native.KS_SET_EXCESS, id=a, excess=nodes[a][0] + k)
            emit(kind=native.KS_SET_EXCESS, id=b, excess=nodes[b][0] - k)
    return np.array(recs, native.DELTA_DT)


# ------------------------------------------------------------------ ranges ---
# The limits the library declares or guards (tests/test_exact_ref_cpu.py reads the
# same values out of the headers, so a change there cannot pass unnoticed):
CELL_MAX_CAP = (1 << 24) - 1      # ks_cell.h: capacity the cell solver's record holds
CELL_MAX_COST = (1 << 31) - 2     # ks_cell.h: |cost · mult| the cell solver's record holds
CPOS_MAX = 0x7FFFFFFE             # ks_pos.h: |cost · mult| or capacity a 16-byte position holds
ABI_MAX_COST = 1 << 40            # ks_host.cpp check_arc: |cost|
ABI_MAX_CAP = 1 << 53             # ks_host.cpp check_arc: capacity
LEN_CAP = 1 << 40                 # ks_engine_impl.h: arc lengths rc / ε are clamped here
FS_DMAX = 1 << 36                 # ks_engine_impl.h: the forward search's distance limit
SOLVE_RANGE = 4.0e18              # ks_engine.hip SolveRun::prepare: maxc · mult · 8 · mult above this is refused


def solve_range_maxc(mult: int) -> int:
    """The largest max |cost| that SolveRun::prepare accepts for a cost multiplier
    mult, by the same double arithmetic: maxc · mult · 8 · mult ≤ 4e18."""
    ok = lambda c: float(c) * float(mult) * 8.0 * float(mult) <= SOLVE_RANGE
    c = int(SOLVE_RANGE) // (8 * mult * mult)
    while not ok(c):
        c -= 1
    while ok(c + 1):
        c += 1
    return c


def scaled(g, cost_mul: int = 1, cap_mul: int = 1):
    """g with every cost multiplied by cost_mul, and every capacity, lower bound
    and supply by cap_mul. The exact optimum scales by cost_mul · cap_mul, the
    flow value by cap_mul."""
    mul = lambda a, k: np.asarray([int(x) * k for x in a.tolist()], np.int64)
    return gen.Graph(g.ntype, mul(g.supply, cap_mul), g.src, g.dst, mul(g.low, cap_mul), mul(g.cap, cap_mul),
                     mul(g.cost, cost_mul), g.atype)


def signed_candidates(seed: int, count: int, max_n: int = 60, cost_hi: int = 100):
    """random_graphs with costs in [−cost_hi, cost_hi): negative arcs and negative
    cycles occur. Every second graph has its lower bounds removed."""
    for trial, g in random_graphs(seed, count, max_n, -cost_hi, cost_hi):
        if trial % 2:
            g = gen.Graph(g.ntype, g.supply, g.src, g.dst, np.zeros_like(g.low), g.cap, g.cost)
        yield trial, g


_FAMILIES: dict = {}
FAMILY_FEASIBLE, FAMILY_INFEASIBLE = 24, 6


def select_family(candidates, feasible: int = FAMILY_FEASIBLE, infeasible: int = FAMILY_INFEASIBLE):
    """The first `feasible` feasible and the first `infeasible` infeasible candidates,
    as the exact reference alone judges them, in candidate order:
    [(trial, graph, (feasible, cost, flows))]. About half of random_graphs' output is
    infeasible (its lower bounds), so a test over the raw stream could pass while
    exercising mostly the infeasible path."""
    import exact_ref
    out, nf, ni = [], 0, 0
    for trial, g in candidates:
        ref = exact_ref.mcf(g)
        if ref[0] and nf < feasible:
            nf += 1
            out.append((trial, g, ref))
        elif not ref[0] and ni < infeasible:
            ni += 1
            out.append((trial, g, ref))
        if nf == feasible and ni == infeasible:
            return out
    raise AssertionError(f"only {nf} feasible and {ni} infeasible candidates")


def signed_graphs(seed: int = 4242, max_n: int = 60, cost_hi: int = 100):
    """The signed family of the GPU range tests: 24 feasible and 6 infeasible members
    of signed_candidates(seed), each with its exact optimum (computed once)."""
    key = ("signed", seed, max_n, cost_hi)
    if key not in _FAMILIES:
        _FAMILIES[key] = select_family(signed_candidates(seed, 400, max_n, cost_hi))
    return _FAMILIES[key]


def negative_cycle():
    """A 3-cycle of cost −5 and capacity 2, no supplies: the optimum sends 2 units
    round it (cost −10, flow value 0)."""
    return graph_from_lists([(1, 0, 0), (2, 0, 0), (3, 0, 0)],
                            [(1, 2, 0, 2, 3), (2, 3, 0, 2, -10), (3, 1, 0, 2, 2)])


def star(arms: int = 200, cap: int = CELL_MAX_CAP):
    """A centre with `arms` out-arcs of capacity cap and equal cost, so all of them
    are admissible at once, and the supply to fill every one: the admissible
    capacities of one node sum to arms · cap (200 · (2^24 − 1) > 2^31). Each arm
    reaches the sink by an arc of cost 1: the optimum is arms · cap."""
    centre, sink = 1, arms + 2
    nodes = [(centre, arms * cap, 0), (sink, -arms * cap, 0)] + [(2 + i, 0, 0) for i in range(arms)]
    arcs = [(centre, 2 + i, 0, cap, 0) for i in range(arms)] + [(2 + i, sink, 0, cap, 1) for i in range(arms)]
    return graph_from_lists(nodes, arcs)


SPARSE_TOP = 4000


def sparse_id_network(maxc: int = 16):
    """12 nodes whose highest id is 4,000: the cost multiplier (the node-slot count
    + 1) is large while the graph is tiny. Costs are k · maxc / 16, the largest
    exactly maxc on arcs the optimum must use (each source's only way to the far
    sink)."""
    ids = list(range(1, 12)) + [SPARSE_TOP]
    sup = {1: 4, 2: 3, 3: 5, 10: -6, SPARSE_TOP: -6}
    nodes = [(i, sup.get(i, 0), 0) for i in ids]
    c = lambda k: maxc * k // 16
    arcs = [(1, 4, 0, 3, c(2)), (1, 5, 0, 2, c(5)), (2, 4, 0, 2, c(1)), (2, 6, 0, 3, c(7)), (3, 5, 0, 4, c(3)),
            (3, 6, 0, 2, c(2)), (3, 7, 0, 2, c(9)), (4, 8, 0, 4, c(4)), (5, 8, 0, 3, c(1)), (5, 9, 0, 3, c(6)),
            (6, 9, 0, 4, c(2)), (7, 9, 0, 2, c(0)), (8, 10, 0, 5, c(3)), (9, 10, 0, 3, c(8)), (8, 11, 0, 3, c(2)),
            (9, 11, 0, 5, c(1)), (11, SPARSE_TOP, 0, 6, maxc), (10, 11, 0, 2, c(12)), (6, 5, 0, 2, c(1)),
            (9, 8, 0, 1, c(4)), (4, 1, 0, 1, c(3))]
    return graph_from_lists(nodes, arcs)


def long_chain(links: int = 7, link_cost: int = 1 << 37, cap: int = 3, supply: int = 5):
    """A chain of `links` arcs of cost link_cost beside one direct arc of cost
    ABI_MAX_COST. With links + 1 nodes the multiplier is links + 2, so in the ε = 1
    phase every arc's length link_cost · mult / ε is beyond LEN_CAP and FS_DMAX.
    The chain is cheaper (7 · 2^37 < 2^40) and takes `cap` units, the direct arc the rest."""
    n = links + 1
    nodes = [(1, supply, 0), (n, -supply, 0)] + [(i, 0, 0) for i in range(2, n)]
    arcs = [(i, i + 1, 0, cap, link_cost) for i in range(1, n)] + [(1, n, 0, supply, ABI_MAX_COST)]
    return graph_from_lists(nodes, arcs)
