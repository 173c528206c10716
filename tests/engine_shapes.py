"""The multi-kernel engine's layout rules, restated, and graphs that sit on them.

TEST INFRASTRUCTURE ONLY, shared by tests/test_engine_shapes_cpu.py (which asserts
every case's premise and solves it with three references) and
tests/test_gpu_engine_layout.py (which solves the same cases on the device with
cell_nodes = −1).

After ks_load_graph the residual CSR is tight (seg_capacity returns the degree
when there is no slack), so a node's class in the engine is exactly that of its
residual degree: its out-arcs plus its in-arcs.

What build() (ks_engine_build.hip:322-337) makes of the classes — and what nn is.
Internal ids take the classes in order, EACH PADDED TO WHOLE 64-NODE BLOCKS, the
hubs last:

    pad_c  = ceil(ncls[c] / 64) · 64            c = 0 … 5
    wbeg[] = running sum of pad_c / win_slots(c)
    hub_base = Σ pad_c,    nn = hub_base + nheavy

So after a plain load nn is NOT the node count: it is the padded count, a
multiple of 64 plus the number of hubs (ncap = nslots = the largest node id there,
ks_engine_build.hip:277-278, but s.nn = o + s.nheavy, :336). Every size switch of
plan() and of the finish reads that nn (ks_engine.hip:3214), so the size cases
below are chosen by layout(g).nn, not by g.n. For the same reason a class owns
pad_c / win_slots(c) windows, the last ones holding no real node (KS_WINDOW tests
base + lane < oend[c]): the count of class windows wbeg[CCLS] is always even.

The hubs keep the order of their node ids: build() selects cls_list[NGC] with
hipcub::DeviceSelect::If over a counting iterator (ks_engine_build.hip:305-317),
which is stable, and k_make_perm gives list[i] the id hub_base + i (:74-78). In a
ladder the sink is node 1 and U node 2, so they are hubs 0 and 1 when they are
hubs, and the hub PUs follow in id order.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import cell_shapes as cs
from cell_shapes import (PU_T, SINK_T, TASK_T, OTHER_T, UNSCHED_COST, Segments, dense, fill_pus, fill_tasks,  # noqa: F401
                         ladder, profile, pu_ids, rebuild_plan, seg_capacity, slot_capacity, sparse, task_ids)
from ksched_amd import gen

# ---------------------------------------------------------------- the rules ---
BLK = 256                 # ks_engine_impl.h:22
WAVE = 64                 # ks_engine_impl.h:23
WPB = BLK // WAVE         # ks_engine_impl.h:24: waves per workgroup
NGC = 6                   # ks_engine_impl.h:25: group classes (hubs are class NGC)
HEAVY_MIN = 4096          # ks_engine_impl.h:26: more positions → hub
CHUNK = 1024              # ks_engine_impl.h:27: positions per HItem
HSPLIT = 4                # ks_engine_impl.h:29: Bellman-Ford workgroups per HItem
WPW = 2                   # ks_engine_impl.h:32-35 (KS_WPW): windows per wave in sparse passes
HUB_LDS = 16              # ks_engine_impl.h:38: hubs whose Bellman-Ford minima are reduced in LDS
BX_CAP = 64               # ks_engine_impl.h:50: updates with at most this many excess nodes are bounded
CCLS = 5                  # ks_engine_impl.h:119: the chunked class
CITEM = 64                # ks_engine_build.hip:446-447: positions per CItem
LEAF_REGS = 5             # ks_engine.hip:1150-1153 (KS_LEAF_REGS): a leaf's arc records held in registers
LEAF_MAX = 8              # ks_engine.hip:1231: leaves are the nodes below obeg[2], classes 0 and 1
CYC_LDS_K, CYC_LDS_T = 14, 1024   # ks_engine.hip:2531-2532
CYC_LDS_MAX = CYC_LDS_K * CYC_LDS_T   # ks_engine.hip:2536: 14,336
CYC_LDS_WORDS = 3         # ks_engine.hip:2538: cyc_lds_bytes(n) = 3 · 4 · n, against the device's LDS per workgroup
LDS_GFX950 = 160 << 10    # ks_engine.hip:2933: 160 KiB on gfx950 (hipDeviceAttributeSharedMemPerBlockOptin)
SMALL_NN = 32768          # ks_engine.hip:3350, 3360, 3407: nn below it → fwd_k 32, α 32, final_div 20
FWD_K_SMALL, FWD_K = 32, 64   # ks_engine.hip:3350
CLASS_BOUNDS = (4, 8, 16, 32, 64, HEAVY_MIN)


def degree_class(d: int) -> int:
    """ks_engine_impl.h:116-118."""
    return 0 if d <= 4 else 1 if d <= 8 else 2 if d <= 16 else 3 if d <= 32 else 4 if d <= 64 else \
        5 if d <= HEAVY_MIN else NGC


def class_lanes(c: int) -> int:
    """ks_engine_impl.h:115."""
    return (4 << c) if c < 4 else 64


def win_batches(c: int) -> int:
    """ks_engine_impl.h:126."""
    return 2 if c < 4 else 1


def win_slots(c: int) -> int:
    """ks_engine_impl.h:128."""
    return win_batches(c) * (64 // class_lanes(c))


def batch_nodes(c: int) -> int:
    """Nodes one batch of a window holds (PER_ in KS_WINDOW, ks_engine.hip:393)."""
    return 64 // class_lanes(c)


def cyc_lds_limit(lds_bytes: int = LDS_GFX950) -> int:
    """The largest nn the one-workgroup cycle search takes (ks_engine.hip:3858):
    nn <= CYC_LDS_MAX and 12 · nn <= the LDS of one workgroup. 13,653 on gfx950."""
    return min(CYC_LDS_MAX, lds_bytes // (4 * CYC_LDS_WORDS))


@dataclass
class Hub:
    node: int        # 1-based node id
    deg: int
    chunks: int      # its HItems
    tail: int        # positions of the last one, 1 … CHUNK


@dataclass
class Layout:
    ncls: list                   # nodes per class, NGC + 1 entries (the last: hubs)
    pad: list                    # internal ids per class, whole 64-node blocks (NGC entries)
    windows: list                # windows per class (NGC entries; class 5: one per padded node)
    occupied: list               # windows that hold a real node, classes 0-4
    wbeg: list                   # NGC + 1 entries
    ncitems: int
    hubs: list                   # [Hub] in build()'s order (by node id)
    nhitems: int
    hub_base: int
    nn: int
    window_grid: int
    dense_grid: int
    sparse_grid: int
    sweep_grid: int
    sweep_cls_blocks: int
    cls: np.ndarray = field(repr=False, default=None)
    cap: np.ndarray = field(repr=False, default=None)

    @property
    def nheavy(self) -> int:
        return len(self.hubs)

    @property
    def class_windows(self) -> int:
        return self.wbeg[CCLS]

    @property
    def bf_items(self) -> int:
        """What the Bellman-Ford rounds deal to waves after the hub workgroups."""
        return self.wbeg[CCLS] + self.ncitems


def layout_of(cap) -> Layout:
    """build() on the segment capacities of the node slots (ks_engine_build.hip:292-470)."""
    cap = np.asarray(cap, np.int64)
    cls = np.searchsorted(CLASS_BOUNDS, cap, side="left")          # degree_class, vectorised
    ncls = np.bincount(cls, minlength=NGC + 1).tolist()
    pad = [(ncls[c] + 63) // 64 * 64 for c in range(NGC)]          # :329
    windows = [pad[c] // win_slots(c) for c in range(NGC)]         # :331
    wbeg = [0]
    for c in range(NGC):
        wbeg.append(wbeg[-1] + windows[c])
    occupied = [-(-ncls[c] // win_slots(c)) for c in range(CCLS)]
    hub_base = sum(pad)                                            # :335
    hubs = []
    for v in np.nonzero(cls == NGC)[0].tolist():                   # ascending slot: the select's order
        d = int(cap[v])
        k = -(-d // CHUNK)                                         # :422-423
        hubs.append(Hub(v + 1, d, k, d - (k - 1) * CHUNK))
    nhitems = sum(h.chunks for h in hubs)
    ncitems = int(sum(-(-int(d) // CITEM) for d in cap[cls == CCLS]))   # :445-447
    blocks = lambda items, per: max(1, -(-items // per))           # noqa: E731
    sweep_cls = blocks(wbeg[CCLS], WPW * WPB)                      # ks_engine_impl.h:521
    return Layout(
        ncls=ncls, pad=pad, windows=windows, occupied=occupied, wbeg=wbeg, ncitems=ncitems, hubs=hubs,
        nhitems=nhitems, hub_base=hub_base, nn=hub_base + len(hubs),
        window_grid=nhitems + blocks(wbeg[NGC], WPB),                          # ks_engine_impl.h:518
        dense_grid=nhitems * HSPLIT + blocks(wbeg[CCLS] + ncitems, WPB),       # :520
        sparse_grid=nhitems * HSPLIT + blocks(wbeg[CCLS] + ncitems, WPW * WPB),   # :526-528
        sweep_grid=nhitems + sweep_cls + ncls[CCLS],                           # :523-525
        sweep_cls_blocks=sweep_cls, cls=cls, cap=cap)


def layout(g) -> Layout:
    """The engine's layout of a graph just loaded: tight segments, capacity = degree."""
    return layout_of(profile(g).deg)


def layout_slack(seg: Segments) -> Layout:
    """The layout after a build with slack (deltas seen since the load): the segments of
    cell_shapes.Segments, plus the spare slots of ks_engine_build.hip:277 — max(64,
    nslots / 16) dead slots of 8 positions each (seg_capacity: not alive, degree 0)."""
    n = int(seg.cap.shape[0])
    spare = max(64, n // 16)
    return layout_of(np.concatenate([seg.cap, np.full(spare, seg_capacity(0, False, False, 1), np.int64)]))


def hub_index(g, node: int) -> int:
    """The index build() gives hub `node` (its minima are reduced in LDS below HUB_LDS)."""
    return [h.node for h in layout(g).hubs].index(int(node))


# --------------------------------------------------------------- the graphs ---
def with_pu_caps(g, caps: dict):
    """g with the capacity of PU → sink replaced for the PUs in caps {node id: cap}."""
    cap = g.cap.copy()
    into_sink = (g.ntype[g.src - 1] == PU_T) & (g.ntype[g.dst - 1] == SINK_T)
    for a in np.nonzero(into_sink)[0].tolist():
        if int(g.src[a]) in caps:
            cap[a] = caps[int(g.src[a])]
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, cap, g.cost)


def funnel(aggs, tasks: int, pus: int, seed: int = 1, pu_cap: int = 2, agg_cap: int = 1):
    """tasks → aggregators → PUs → sink, and every task → U → sink.

    aggs: [(i, o), …]: aggregator k has exactly i in-arcs (from i different tasks) and
    o out-arcs (to o different PUs): i + o residual positions, in both directions as
    the cluster aggregator has them. Ids: sink 1, U 2, the aggregators, the PUs, the
    tasks. A task's degree is 1 plus the aggregators that take it, a PU's 1 plus the
    aggregators that feed it. U → sink holds every task: feasible by construction."""
    A = len(aggs)
    if A < 1 or tasks < max(i for i, _ in aggs) or pus < max(o for _, o in aggs) or min(min(a) for a in aggs) < 1:
        raise ValueError("funnel: an aggregator needs i different tasks and o different PUs, both at least 1")
    rng = np.random.default_rng(seed)
    SINK, U, A0 = 1, 2, 3
    P0 = A0 + A
    T0 = P0 + pus
    ts, td, as_, ad = [], [], [], []
    toff = poff = 0
    for k, (i, o) in enumerate(aggs):        # consecutive runs, rotated so the aggregators overlap only partly
        ts.append(T0 + (toff + np.arange(i, dtype=np.int64)) % tasks)
        td.append(np.full(i, A0 + k, np.int64))
        as_.append(np.full(o, A0 + k, np.int64))
        ad.append(P0 + (poff + np.arange(o, dtype=np.int64)) % pus)
        toff = (toff + i // 2 + 1) % tasks
        poff = (poff + o // 2 + 1) % pus
    ts, td, as_, ad = (np.concatenate(x) for x in (ts, td, as_, ad))
    order = np.argsort(ts, kind="stable")
    ts, td = ts[order], td[order]
    tid = T0 + np.arange(tasks, dtype=np.int64)
    pid = P0 + np.arange(pus, dtype=np.int64)
    src = np.concatenate([ts, tid, as_, pid, [U]])
    dst = np.concatenate([td, np.full(tasks, U, np.int64), ad, np.full(pus, SINK, np.int64), [SINK]])
    cap = np.concatenate([np.ones(ts.shape[0] + tasks, np.int64), np.full(as_.shape[0], agg_cap, np.int64),
                          np.full(pus, pu_cap, np.int64), [tasks]])
    cost = np.concatenate([rng.integers(1, 101, ts.shape[0]), np.full(tasks, UNSCHED_COST, np.int64),
                           rng.integers(0, 21, as_.shape[0]), np.zeros(pus + 1, np.int64)])
    n = 2 + A + pus + tasks
    ntype = np.full(n, OTHER_T, np.int32)
    ntype[SINK - 1] = SINK_T
    ntype[P0 - 1:P0 - 1 + pus] = PU_T
    ntype[T0 - 1:] = TASK_T
    supply = np.zeros(n, np.int64)
    supply[T0 - 1:] = 1
    supply[SINK - 1] = -tasks
    return gen.Graph(ntype, supply, src, dst, np.zeros(src.shape[0], np.int64), cap, cost)


def agg_ids(g) -> np.ndarray:
    """The aggregators of a funnel: the untyped nodes after U."""
    return np.nonzero(g.ntype == OTHER_T)[0][1:] + 1


_RANGE = {0: (1, 4), 1: (5, 8), 2: (9, 16), 3: (17, 32), 4: (33, 64)}


def _spread(lo, hi, total):
    """Integers in [lo_k, hi_k] that sum to total (round robin from the lows), or None."""
    v = list(lo)
    rest = total - sum(v)
    if rest < 0 or total > sum(hi):
        return None
    while rest:
        moved = False
        for k in range(len(v)):
            if rest and v[k] < hi[k]:
                v[k] += 1
                rest -= 1
                moved = True
        if not moved:
            return None
    return v


def _splits(k: int):
    return sorted({0, k // 2, k})


def classed(counts, seed: int = 1):
    """A ladder with exactly counts[c] nodes in class c for c = 0 … 4 (the sink and U
    counted where their degrees put them; they may be chunked).

    Every class is split between PUs and tasks (none, half or all of its nodes as PUs; class 0
    may hold a few isolated nodes), the degrees within a class are spread so that both sides
    give the same number of preference arcs. The splits are tried in a fixed order, so the
    graph is a function of (counts, seed)."""
    want = [int(x) for x in counts]
    assert len(want) == CCLS
    for sc in range(NGC):
        for uc in range(NGC):
            m = list(want)
            for c in (sc, uc):              # the sink and U count where their degrees put them
                if c < CCLS:
                    m[c] -= 1
            if min(m) < 0:
                continue
            for pads in (0, 1, 2, 3):
                if pads > m[0]:
                    break
                for p4 in _splits(m[4]):
                    for p3 in _splits(m[3]):
                        for p2 in _splits(m[2]):
                            for p1 in _splits(m[1]):
                                for p0 in _splits(m[0] - pads):
                                    ps = (p0, p1, p2, p3, p4)
                                    pcls = [c for c in range(CCLS) for _ in range(ps[c])]
                                    tcls = [c for c in range(CCLS) for _ in range(m[c] - ps[c] - (pads if c == 0 else 0))]
                                    P, T = len(pcls), len(tcls)
                                    if P < 1 or T < 1 or degree_class(P + 1) != sc or degree_class(T + 1) != uc:
                                        continue
                                    plo = [max(_RANGE[c][0], 2) - 1 for c in pcls]
                                    phi = [min(_RANGE[c][1] - 1, T) for c in pcls]
                                    tlo = [_RANGE[c][0] - 1 for c in tcls]
                                    thi = [min(_RANGE[c][1] - 1, P) for c in tcls]
                                    if any(a > b for a, b in zip(plo + tlo, phi + thi)):
                                        continue
                                    total = max(sum(plo), sum(tlo))
                                    pin, tout = _spread(plo, phi, total), _spread(tlo, thi, total)
                                    if pin is None or tout is None:
                                        continue
                                    try:
                                        g = ladder([x + 1 for x in pin], [x + 1 for x in tout], pad=pads, seed=seed)
                                    except ValueError:
                                        continue
                                    if layout(g).ncls[:CCLS] == want:
                                        return g
    raise ValueError("classed: no ladder with %r nodes per class" % (want,))


# ---------------------------------------------------------------- the cases ---
@dataclass
class Case:
    """One engine case and the premise it claims (asserted on the CPU by
    tests/test_engine_shapes_cpu.py from layout(), before any device sees it)."""
    name: str
    build: object                 # () → gen.Graph
    kind: str                     # bound | window | leaf | chunk | hubchunk | hubcount | size | excess
    ncls: dict | None = None      # {class: nodes in it}, exact
    degrees: dict | None = None   # {residual degree: at least this many nodes of exactly that degree}
    hubs: list | None = None      # [(degree, chunks, tail)] of every hub, in build()'s order
    nheavy: int | None = None
    n: int | None = None          # g.n
    nn: int | None = None         # layout(g).nn
    check: object = None          # (g, layout) → None: further premises
    used: object = None           # (g) → node ids that must carry flow in the oracle's optimum


_BUILT: dict = {}


def built(case: Case):
    """The case's graph, built once per process."""
    if case.name not in _BUILT:
        _BUILT[case.name] = case.build()
    return _BUILT[case.name]


# bounds and strides: the lone cases of the cell file whose class bounds are the engine's too
# (4/5 … 64/65; the cell solver's 512/513 bound is no bound here, 4,096/4,097 is)
BOUND_NAMES = ["bound-pu-%d" % d for d in (4, 8, 16, 32, 64)] + ["bound-tasks-4-5-8-9", "bound-all"] + \
    list(cs.PARTIAL) + ["stride-hub-4096", "stride-hub-4097", "stride-hub-6145", "three-hubs"]


def _from_cell(name):
    c = cs.by_name(name)
    deg = dict(c.pus or {})
    for d, k in (c.tasks or {}).items():
        deg[d] = deg.get(d, 0) + k
    hubs = None
    if name == "stride-hub-4096":
        hubs = []                                     # 4,096 positions: still chunked, 64 CItems
    elif name == "stride-hub-4097":
        hubs = [(4097, 5, 1), (4097, 5, 1)]           # U, then the PU
    elif name == "stride-hub-6145":
        hubs = [(6201, 7, 57), (6145, 7, 1)]
    elif name == "three-hubs":
        hubs = []                                     # 513, 600, 701: hubs of the cell solver only
    return Case(name, lambda: cs.built(c), "bound", degrees=deg or None, hubs=hubs)


BOUNDS = [_from_cell(n) for n in BOUND_NAMES]

# ---- windows: for each class c, exactly 1, 64/G, 64/G + 1, WS − 1, WS, WS + 1 and 2·WS + 1 nodes
WINDOW_COUNTS = {c: sorted({1, batch_nodes(c), batch_nodes(c) + 1, win_slots(c) - 1, win_slots(c), win_slots(c) + 1,
                            2 * win_slots(c) + 1} - {0}) for c in range(CCLS)}
# which graph holds which count (found by trying classed() on the combinations, most new pairs
# first: a class-4 PU needs 32 tasks, so not every combination has a ladder)
WINDOW_GRAPHS = [
    (1, 15, 17, 9, 1),
    (16, 16, 4, 3, 3),
    (17, 17, 1, 4, 2),
    (31, 1, 5, 5, 1),
    (32, 8, 7, 1, 1),
    (33, 9, 8, 2, 1),
    (65, 33, 9, 1, 1),
]


def window_pairs():
    """{(class, count): case name}."""
    out = {}
    for cnt in WINDOW_GRAPHS:
        for c, k in enumerate(cnt):
            out.setdefault((c, k), "window-" + "-".join(map(str, cnt)))
    return out


def _window_case(cnt):
    return Case("window-" + "-".join(map(str, cnt)), lambda: classed(cnt, seed=500 + sum(cnt)), "window",
                ncls=dict(enumerate(cnt)))


def only_0_and_5():      # tasks and PUs of 3 positions; the sink and U of 601: classes 0 and 5 only
    return ladder([3] * 600, [3] * 600, seed=301)


def no_class_window():   # every degree at least 65: 70 tasks × 65 PUs complete, the sink of 65 positions
    return dense(65 * 70 + 65, pus=65, seed=17)


def windows_mod8(r: int):
    """wbeg[CCLS] ≡ r (mod 8), r even (see the module text): PUs of 3 and tasks of 2 positions
    only, 3·P class-0 nodes in 4, 1 and 3 blocks of two windows each. With 21 PUs the sink
    (22 positions, class 3: 16 windows) and U (43, class 4: 64 windows) add multiples of 8;
    with 64 and 85 both are chunked."""
    P = {0: 85, 2: 21, 6: 64}[r]
    return ladder([3] * P, [2] * (2 * P), seed=600 + r)


def items_mod(r: int, m: int):
    """wbeg[CCLS] + ncitems ≡ r (mod m) with m = 4 or 8: PUs on both sides of four bounds, 700
    tasks, and one chunked PU whose CItems (one more per 64 positions) give the residue."""
    base = [5, 9, 17, 33] * 3
    for d in range(65, 65 + 64 * 9, 64):
        pus = base + [d]
        g = ladder(pus, fill_tasks(pus, per=4, tasks=700), seed=700 + d)
        if layout(g).bf_items % m == r:
            return g
    raise ValueError("items_mod: no chunked PU gives the residue")


WINDOWS = [_window_case(cnt) for cnt in WINDOW_GRAPHS] + [
    Case("window-classes-0-and-5-only", only_0_and_5, "window", ncls={0: 1200, 1: 0, 2: 0, 3: 0, 4: 0, 5: 2, 6: 0}),
    Case("window-none-every-degree-65-up", no_class_window, "window", ncls={0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 6: 0},
         check=lambda g, L: _same((L.class_windows, L.sweep_cls_blocks, int(profile(g).deg.min())), (0, 1, 65))),
] + [Case("window-total-mod8-%d" % r, (lambda r=r: windows_mod8(r)), "window",
          check=(lambda g, L, r=r: _same(L.class_windows % (WPW * WPB), r))) for r in (0, 2, 6)] + [
    Case("window-items-mod4-1", lambda: items_mod(1, 4), "window",
         check=lambda g, L: _same(L.bf_items % WPB, 1)),
    Case("window-items-mod8-1", lambda: items_mod(1, 8), "window",
         check=lambda g, L: _same(L.bf_items % (WPW * WPB), 1)),
    Case("window-items-mod8-7", lambda: items_mod(7, 8), "window",
         check=lambda g, L: _same(L.bf_items % (WPW * WPB), 7)),
]


def _same(have, want):
    assert have == want, (have, want)


# ---- leaves: tasks and PUs of exactly 5, 6 and 8 positions; the cheap arcs of every PU are its last
def leaves():
    """Tasks of 5, 6 and 8 positions and PUs of 5, 6 and 8. A PU's segment holds its in-arcs
    in arc order (by task id) and its arc into the sink last, so positions 6-8 of an
    8-position PU are its 6th and 7th in-arc and the arc into the sink: the costs make
    the in-arcs from a PU's LAST tasks cheap (1-3) and the others dear (60-100), so the
    optimum places tasks through the positions expand_leaf reads one by one."""
    tk = [5] * 12 + [6] * 12 + [8] * 12
    pus = fill_pus(tk, [5] * 8 + [6] * 8 + [8] * 8, per=7, pus=24)
    g = ladder(pus, tk, seed=801)
    cost = g.cost.copy()
    for v in pu_ids(g).tolist():
        ins = np.nonzero(g.dst == v)[0]                 # arc order = position order
        cost[ins] = 60 + (cost[ins] % 41)
        cost[ins[LEAF_REGS:]] = 1 + (cost[ins[LEAF_REGS:]] % 3)
    return gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, g.cap, cost)


def late_in_arcs(g) -> np.ndarray:
    """Arcs of g that are the 6th or a later position of a leaf PU's segment (in-arcs only)."""
    p = profile(g)
    out = []
    for v in pu_ids(g).tolist():
        if p.deg[v - 1] <= LEAF_MAX:
            own = np.nonzero((g.src == v) | (g.dst == v))[0]
            out += [a for a in own[LEAF_REGS:].tolist() if g.dst[a] == v]
    return np.asarray(out, np.int64)


LEAVES = [Case("leaf-5-6-8-positions", leaves, "leaf", degrees={5: 20, 6: 20, 8: 20})]


# ---- the chunked class: 65, 128, 129 and 4,096 positions
def chunked_pus():
    pus = [65, 128, 129, 4096] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=4000), seed=901)     # 4,095 tasks at least: U has 4,096 too


def chunked_aggs():
    return funnel([(33, 32), (64, 64), (65, 64), (2048, 2048)], tasks=2100, pus=2060, seed=902)


CHUNKED = [
    Case("chunk-pus-65-128-129-4096", chunked_pus, "chunk", degrees={65: 1, 128: 1, 129: 1, 4096: 2}, nheavy=0),
    Case("chunk-aggregators-65-128-129-4096", chunked_aggs, "chunk", degrees={65: 1, 128: 1, 129: 1, 4096: 1},
         nheavy=0, check=lambda g, L: _same(profile(g).deg[agg_ids(g) - 1].tolist(), [65, 128, 129, 4096])),
]

# ---- hub chunks: tails of 1, 256, 257, 1,024, 1 and 1 positions
HUB_DEGREES = {4097: (5, 1), 4352: (5, 256), 4353: (5, 257), 5120: (5, 1024), 5121: (6, 1), 8193: (9, 1)}


def hub_pu(d: int):      # a PU and U of d positions each (d − 1 tasks)
    pus = [d] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=d - 1), seed=1000 + d)


def hub_agg():           # an aggregator of 5,121 positions: 2,561 in-arcs, 2,560 out-arcs
    return funnel([(2561, 2560)], tasks=4352, pus=2600, seed=1001)


HUBCHUNKS = [Case("hubchunk-%d-tail-%d" % (d, t), (lambda d=d: hub_pu(d)), "hubchunk", hubs=[(d, k, t), (d, k, t)])
             for d, (k, t) in HUB_DEGREES.items()] + [
    Case("hubchunk-aggregator-5121-both-directions", hub_agg, "hubchunk",
         hubs=[(4353, 5, 257), (5121, 6, 1)],        # U (4,352 tasks + 1), then the aggregator
         check=lambda g, L: _same((int((g.dst == 3).sum()), int((g.src == 3).sum())), (2561, 2560)))]


# ---- hub count: 0, 1, 16, 17 and 21 hubs
def many_hubs(k: int, fillers: int, reverse: bool = False):
    """k hub PUs of 4,097 positions, `fillers` PUs of 3, 6,000 tasks; U (6,001) is a hub, the
    sink one when k + fillers + 1 > 4,096. Every hub PU takes 50 tasks and every filler one,
    fewer places than tasks: every hub PU is full and U carries the rest in the optimum.
    reverse: the hub PUs take the LAST PU ids, so the hub order of build() is reversed
    among them against the arcs' costs."""
    pus = [3] * fillers + [4097] * k if reverse else [4097] * k + [3] * fillers
    g = ladder(pus, fill_tasks(pus, per=21, tasks=6000), seed=1100 + k)
    deg = profile(g).deg
    return with_pu_caps(g, {int(v): (50 if deg[v - 1] > HEAVY_MIN else 1) for v in pu_ids(g)})


def one_hub():           # U alone: 4,200 tasks, 2,000 PUs of 3 positions
    return ladder([3] * 2100, fill_tasks([3] * 2100, per=1, tasks=4200), seed=1101)


def hub_nodes(g):
    return [h.node for h in layout(g).hubs if g.ntype[h.node - 1] != SINK_T]


H4097 = (4097, 5, 1)
HUBCOUNT = [
    Case("hubcount-0", lambda: cs.built(cs.by_name("bound-all")), "hubcount", nheavy=0),
    Case("hubcount-1-U-alone", one_hub, "hubcount", hubs=[(4201, 5, 105)]),
    # 15 hub PUs and U; 3,900 fillers: the sink has 3,916 positions and stays chunked
    Case("hubcount-16-all-in-LDS", lambda: many_hubs(15, 3900), "hubcount", hubs=[(6001, 6, 881)] + [H4097] * 15,
         used=hub_nodes),
    # the sink (4,116) is hub 0, U hub 1, the PUs hubs 2-16: the last PU is the one at index 16
    Case("hubcount-17-one-past-LDS", lambda: many_hubs(15, 4100), "hubcount",
         hubs=[(4116, 5, 20), (6001, 6, 881)] + [H4097] * 15, used=hub_nodes),
    # sink, U, then 19 PUs: PUs 15-19 (ids 17-21) are hubs 16-20
    Case("hubcount-21-five-past-LDS", lambda: many_hubs(19, 4100), "hubcount",
         hubs=[(4120, 5, 24), (6001, 6, 881)] + [H4097] * 19, used=hub_nodes),
    # the same with the hub PUs after the fillers: other PUs (other costs) sit at indices 16-20
    Case("hubcount-21-hub-PUs-last", lambda: many_hubs(19, 4100, reverse=True), "hubcount",
         hubs=[(4120, 5, 24), (6001, 6, 881)] + [H4097] * 19, used=hub_nodes),
]


# ---- size switches: by nn = Σ padded classes + hubs, not by the node count
def quincy_nodes(n: int, seed: int):
    """gen.quincy in config-2 proportions (M = T/10 machines, 25 racks, 100 jobs) with the
    task count adjusted to n nodes: n = T + J + R + 2M + 2."""
    R, J = 25, 100
    for M in range((n - J - R - 2) // 12, (n - J - R - 2) // 12 - 40, -1):
        T = n - J - R - 2 - 2 * M
        if T >= 10 * M:
            return gen.quincy(T, M, R, J, seed)
    raise ValueError("quincy_nodes")


def quincy_nn(nn: int, seed: int):
    """The same family with layout(g).nn == nn: the node count is searched downwards from nn
    (the padding of six classes adds at most 378 ids)."""
    for n in range(nn, nn - 450, -1):
        g = quincy_nodes(n, seed)
        if layout(g).nn == nn:
            return g
    raise ValueError("quincy_nn: no node count gives nn = %d" % nn)


# the switches sit at nn <= 13,653 (the LDS of gfx950) and nn <= 14,336 (CYC_LDS_MAX); a config-2
# shaped graph has one hub (X), so nn = 64·k + 1: the nearest values on either side
CYC_SIDES = {"lds-13633": 13633, "lds-13697": 13697, "max-14273": 14273, "max-14337": 14337}
SIZE_SEEDS = (1, 2)
SIZES = [Case("size-quincy-n-%d-seed%d" % (n, s), (lambda n=n, s=s: quincy_nodes(n, s)), "size", n=n)
         for n in (14336, 14337) for s in SIZE_SEEDS] + [
    Case("size-quincy-nn-%s-seed%d" % (k, s), (lambda v=v, s=s: quincy_nn(v, s)), "size", nn=v, nheavy=1)
    for k, v in CYC_SIDES.items() for s in SIZE_SEEDS] + [
    Case("size-sparse-n-32767", lambda: sparse(32_767), "size", n=32767, nn=32770),
    Case("size-sparse-n-32768", lambda: sparse(32_768), "size", n=32768, nn=32770),
    # 32,704 class-0 nodes are 511 blocks: nn = 32,704 + 2 hubs, the largest below 32,768
    Case("size-sparse-nn-32706", lambda: sparse(32_706), "size", n=32706, nn=32706),
    Case("size-sparse-nn-32770", lambda: sparse(32_707), "size", n=32707, nn=32770),
]


# ---- few excess nodes: fwd_k (32 below 32,768 ids) and BX_CAP (64)
def few_tasks(t: int):
    tk = [3] * t
    return ladder(fill_pus(tk, per=4), tk, seed=1200 + t)


EXCESS = [Case("excess-%d-tasks" % t, (lambda t=t: few_tasks(t)), "excess", degrees={3: t}) for t in (32, 33, 64, 65)]

ALL = BOUNDS + WINDOWS + LEAVES + CHUNKED + HUBCHUNKS + HUBCOUNT + SIZES + EXCESS
OPTION_KINDS = ("bound", "chunk", "hubchunk", "hubcount")     # the cases that also run off the defaults
OPTIONS = {
    "pos32": {"compact_pos": -1},
    "hop-off": {"two_hop": -1},
    "hop1": {"two_hop": 1},
    "queue2": {"fault_inject": 512},      # the 2-entry continuation queue (no fault is injected)
}


def by_name(name: str) -> Case:
    return next(c for c in ALL if c.name == name)


# ------------------------------------------------------------- class moves ---
@dataclass
class Move:
    """A node v that changes class while the graph lives. Every step is one ks_apply_deltas
    stream of new arcs t → v (t: tasks without one, in id order) and one solve. The classes of
    v and the hub counts after the load and after every step's build are claimed here and
    derived on the CPU from cell_shapes.Segments (the shared seg_capacity / k_capacity rule)."""
    name: str
    build: object      # () → gen.Graph
    node: object       # (g) → v
    steps: tuple       # arcs added per step
    classes: tuple     # v's class after the load and after every step's solve
    nheavy: tuple      # hubs then
    rebuilt: tuple     # whether each step's solve rebuilds the CSR


def move_64():       # a PU of 64 positions, tight: class 4
    pus = [64] + [10] * 10
    return ladder(pus, fill_tasks(pus, per=3, tasks=200), seed=1301)


def move_4096():     # an aggregator of 2,048 + 2,048 positions; U (2,101) and the sink (2,061) chunked: no hub
    return funnel([(2048, 2048)], tasks=2100, pus=2060, seed=1302)


def move_5120():     # a hub PU of 5,120 positions (tail 1,024); 5,300 tasks, so some have no arc into it
    pus = [5120] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=5300), seed=1303)


def move_node(g, d):
    p = profile(g)
    return int(next(x + 1 for x in range(g.n) if p.deg[x] == d and g.ntype[x] in (PU_T, OTHER_T) and x > 1))


def move_tasks(g, v):
    """Tasks without an arc into v, in id order."""
    adj = set(g.src[g.dst == v].tolist())
    return [int(t) for t in task_ids(g) if int(t) not in adj]


MOVES = [
    # 64 tight → the 65th arc overflows: the rebuild with slack gives twice the segment, 128
    # (chunked, 2 CItems); 63 more arcs fill it in place; the 129th overflows again: 256
    Move("move-64-to-chunked", move_64, lambda g: move_node(g, 64), (1, 63, 1), (4, 5, 5, 5), (0, 0, 0, 0),
         (1, 0, 1)),
    # 4,096 tight (64 CItems) → the 4,097th arc: twice the segment, 8,192 positions: the graph's first
    # hub; the inbox, hub flags and claim slots appear on that rebuild; a second arc lands in place
    Move("move-4096-to-first-hub", move_4096, lambda g: move_node(g, 4096), (1, 1), (5, 6, 6), (0, 1, 1), (1, 0)),
    # a hub of 5,120 (5 full HItems) gains its 5,121st: 10,240 positions, 10 HItems of which half are inert
    Move("move-hub-5120-gains-one", move_5120, lambda g: move_node(g, 5120), (1, 1), (6, 6, 6), (2, 2, 2), (1, 0)),
]

MOVE_COST = 7        # cost of every arc a move adds: cheaper than most preferences, so the optimum takes it


def move_plan(mv: Move):
    """→ (g, v, [[task ids] per step])."""
    g = mv.build()
    v = mv.node(g)
    free = move_tasks(g, v)
    assert len(free) >= sum(mv.steps), "not enough tasks without an arc into the node"
    parts, at = [], 0
    for k in mv.steps:
        parts.append(free[at:at + k])
        at += k
    return g, v, parts


def size_side(nn: int, lds_bytes: int = LDS_GFX950) -> tuple:
    """(one-workgroup cycle search?, small-graph schedule?) for a graph of nn internal ids."""
    return nn <= cyc_lds_limit(lds_bytes), nn < SMALL_NN
