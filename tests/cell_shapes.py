"""The cell solver's layout rules, restated, and graphs that sit on them.

TEST INFRASTRUCTURE ONLY, shared by tests/test_cell_shapes_cpu.py (which asserts
every case's premise and solves it with three references) and
tests/test_gpu_cell_layout.py (which solves the same cases on the device).

After ks_load_graph the residual CSR is tight (seg_capacity returns the degree
when there is no slack), so a node's class in the cell solver is exactly that of
its residual degree: its out-arcs plus its in-arcs. A segment holds a node's
positions in arc order, so the graphs below list every node's arc into the sink
LAST: the one forward arc of a PU of 257 or 4,097 positions is then its 257th or
4,097th position, the first of the second round of a wave's or the workgroup's
walk.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ksched_amd import gen

# ---------------------------------------------------------------- the rules ---
CELL_NCLS = 7                 # ks_cell.h:27
CELL_THREADS = 1024           # ks_cell.h:28 (CT in ks_cell.hip:51)
CELL_MAX_POS = 1 << 18        # ks_cell.h:55: positions per cell the compact record addresses
UC = 4                        # ks_cell.hip:397: chunks a wave or the workgroup walks per round
WAVE_ROUND = 64 * UC          # ks_cell.hip:437: positions per round of sweep_wave
HUB_ROUND = CELL_THREADS * UC  # ks_cell.hip:496: positions per round of sweep_hub
BXC = 256                     # ks_cell.hip:57: updates with at most this many excess nodes are bounded
CLASS_BOUNDS = (4, 8, 16, 32, 64, 512)

SINK_T, PU_T, TASK_T, OTHER_T = 3, 2, 1, 0   # DIMACS node types (gen.py)
UNSCHED_COST = 1000


def cell_class(cap: int) -> int:
    """ks_cell.h:33-35."""
    return 0 if cap <= 4 else 1 if cap <= 8 else 2 if cap <= 16 else 3 if cap <= 32 else 4 if cap <= 64 else \
        5 if cap <= 512 else 6


def items_per_wave(c: int) -> int:
    """ks_cell.hip:931-933 (THR_CLASSES = 2, ks_cell.hip:930): leaf nodes per item."""
    if c < 2:
        return 64
    if c < 4:
        g = 4 << c
        return (64 // g) * (4 if g <= 16 else 2)
    return 1


def seg_capacity(deg: int, alive: bool, task: bool, slack: int) -> int:
    """ks_engine_build.hip:41-51."""
    if not slack:
        return deg
    if (not alive or task) and deg <= 8:
        return 8
    c = deg + (deg // 2 if deg // 2 > 4 else 4)
    if c <= 64:
        g = 4
        while g < c:
            g <<= 1
        return g
    return (c + 63) // 64 * 64


@dataclass
class Profile:
    deg: np.ndarray      # residual degree per node (out-arcs plus in-arcs)
    cls: np.ndarray      # cell_class of it
    counts: list         # nodes per class, CELL_NCLS entries
    positions: int       # the cell's residual positions (2·m after a load)


def profile(g) -> Profile:
    deg = np.bincount(g.src - 1, minlength=g.n) + np.bincount(g.dst - 1, minlength=g.n)
    cls = np.searchsorted(CLASS_BOUNDS, deg, side="left")   # the same bounds as cell_class
    return Profile(deg, cls, np.bincount(cls, minlength=CELL_NCLS).tolist(), 2 * g.m)


# --------------------------------------------------------------- the graphs ---
def ladder(pus, tasks, pad: int = 0, seed: int = 1):
    """A scheduling-shaped graph whose node degrees the caller dictates.

    pus: the residual degree of every PU (its in-arcs plus its one arc into the
    sink); tasks: the out-degree of every task (its preference arcs plus its one
    arc into the unscheduled aggregator U; tasks have no in-arcs). Ids: sink 1,
    U 2, the PUs, the tasks, then pad isolated nodes. U → sink holds every task,
    so the graph is feasible by construction. Raises ValueError when no simple
    bipartite graph has these degrees."""
    pus = [int(d) for d in pus]
    tasks = [int(d) for d in tasks]
    P, T = len(pus), len(tasks)
    if P < 1 or T < 1 or min(pus) < 1 or min(tasks) < 1:
        raise ValueError("ladder: at least one PU and one task, every degree >= 1")
    need = np.asarray(pus, np.int64) - 1        # in-arcs per PU
    want = np.asarray(tasks, np.int64) - 1      # preference arcs per task
    if need.sum() != want.sum():
        raise ValueError(f"ladder: the PUs take {int(need.sum())} preference arcs, the tasks give {int(want.sum())}")
    if want.max() > P or need.max() > T:
        raise ValueError("ladder: a degree beyond the other side's node count")
    rng = np.random.default_rng(seed)
    SINK, U, PU0 = 1, 2, 3
    T0 = PU0 + P
    # Gale–Ryser, greedily: the tasks with the most preferences first, each to the
    # PUs with the most in-arcs still open (ties broken by the seed)
    tie = rng.random(P)
    left = need.copy()
    src, dst = [], []
    for t in np.argsort(-want, kind="stable").tolist():
        k = int(want[t])
        if k == 0:
            continue
        key = -(left + tie)
        pick = np.argpartition(key, k - 1)[:k] if k < P else np.arange(P)
        if left[pick].min() <= 0:
            raise ValueError("ladder: these degrees have no simple bipartite graph")
        left[pick] -= 1
        src.append(np.full(k, T0 + t, np.int64))
        dst.append(PU0 + np.sort(pick).astype(np.int64))
    if left.any():
        raise ValueError("ladder: these degrees have no simple bipartite graph")
    order = np.argsort(np.concatenate(src), kind="stable") if src else np.zeros(0, np.int64)
    psrc = np.concatenate(src)[order] if src else np.zeros(0, np.int64)
    pdst = np.concatenate(dst)[order] if src else np.zeros(0, np.int64)
    npref = psrc.shape[0]
    tid = T0 + np.arange(T, dtype=np.int64)
    pid = PU0 + np.arange(P, dtype=np.int64)
    pu_cap = rng.integers(1, np.maximum(need, 1) + 1)          # 1..in-degree: PUs are contended
    a_src = np.concatenate([psrc, tid, pid, [U]])
    a_dst = np.concatenate([pdst, np.full(T, U, np.int64), np.full(P, SINK, np.int64), [SINK]])
    a_cap = np.concatenate([np.ones(npref + T, np.int64), pu_cap, [T]])
    a_cost = np.concatenate([rng.integers(1, 101, npref), np.full(T, UNSCHED_COST, np.int64),
                             np.zeros(P + 1, np.int64)])
    n = 2 + P + T + pad
    ntype = np.full(n, OTHER_T, np.int32)
    ntype[SINK - 1] = SINK_T
    ntype[PU0 - 1:PU0 - 1 + P] = PU_T
    ntype[T0 - 1:T0 - 1 + T] = TASK_T
    supply = np.zeros(n, np.int64)
    supply[T0 - 1:T0 - 1 + T] = 1
    supply[SINK - 1] = -T
    return gen.Graph(ntype, supply, a_src.astype(np.int64), a_dst.astype(np.int64), np.zeros(a_src.shape[0], np.int64),
                     a_cap.astype(np.int64), a_cost.astype(np.int64))


def pu_ids(g) -> np.ndarray:
    return np.nonzero(g.ntype == PU_T)[0] + 1


def task_ids(g) -> np.ndarray:
    return np.nonzero(g.ntype == TASK_T)[0] + 1


def fill_tasks(pus, fixed=(), per: int = 3, tasks: int = 0) -> list:
    """Task out-degrees for ladder(pus, ·): the fixed ones, then fillers that give the
    preference arcs the PUs still take, `per` each (the remainder spread one by one),
    at least as many tasks as the largest PU has in-arcs and at least `tasks`."""
    rest = sum(d - 1 for d in pus) - sum(t - 1 for t in fixed)
    if rest < 0:
        raise ValueError("fill_tasks: the fixed tasks give more preference arcs than the PUs take")
    f = max(-(-rest // per), max(pus) - 1 - len(fixed), tasks - len(fixed), 0)
    if f == 0:
        if rest:
            raise ValueError("fill_tasks: no room for the remaining preference arcs")
        return list(fixed)
    base, extra = divmod(rest, f)
    return list(fixed) + [base + 2] * extra + [base + 1] * (f - extra)


def fill_pus(tasks, fixed=(), per: int = 40, pus: int = 0) -> list:
    """PU degrees for ladder(·, tasks): the fixed ones, then fillers that take the
    preference arcs the tasks still give, `per` in-arcs each."""
    rest = sum(t - 1 for t in tasks) - sum(d - 1 for d in fixed)
    if rest < 0:
        raise ValueError("fill_pus: the fixed PUs take more preference arcs than the tasks give")
    f = max(-(-rest // per), max(tasks) - 1 - len(fixed), pus - len(fixed), 0)
    if f == 0:
        if rest:
            raise ValueError("fill_pus: no room for the remaining preference arcs")
        return list(fixed)
    base, extra = divmod(rest, f)
    return list(fixed) + [base + 2] * extra + [base + 1] * (f - extra)


def dense(arcs: int, pus: int = 256, seed: int = 7):
    """Few nodes and exactly `arcs` arcs: tasks with an arc to every one of `pus`
    PUs (the last task to the first few only), and every PU's arc into the sink.
    dense(131_072) is a 511 × 256 complete bipartite layer plus 256 arcs into the
    sink: 2^18 positions. Feasible: every task reaches a PU with spare room."""
    R = pus
    body = arcs - R
    if body < 1:
        raise ValueError("dense: fewer arcs than PUs")
    L = -(-body // R)
    rng = np.random.default_rng(seed)
    SINK, PU0 = 1, 2
    T0 = PU0 + R
    t = np.repeat(np.arange(L, dtype=np.int64), R)[:body]
    p = np.tile(np.arange(R, dtype=np.int64), L)[:body]
    cap = rng.integers(-(-L // R) + 1, -(-L // R) + 4, R)      # Σ cap > L: every task fits
    src = np.concatenate([T0 + t, PU0 + np.arange(R, dtype=np.int64)])
    dst = np.concatenate([PU0 + p, np.full(R, SINK, np.int64)])
    n = 1 + R + L
    ntype = np.full(n, TASK_T, np.int32)
    ntype[SINK - 1] = SINK_T
    ntype[PU0 - 1:PU0 - 1 + R] = PU_T
    supply = np.zeros(n, np.int64)
    supply[T0 - 1:] = 1
    supply[SINK - 1] = -L
    return gen.Graph(ntype, supply, src, dst, np.zeros(arcs, np.int64),
                     np.concatenate([np.ones(body, np.int64), cap]),
                     np.concatenate([rng.integers(1, 101, body), np.zeros(R, np.int64)]))


def sparse(nodes: int, seed: int = 11):
    """A ladder of exactly `nodes` nodes, every task with one preference and every PU
    with two in-arcs (the node-limit cases: few positions, many nodes)."""
    P = (nodes - 2) // 3
    T = 2 * P
    return ladder([3] * P, [2] * T, pad=nodes - 2 - P - T, seed=seed)


# ---------------------------------------------------------------- the cases ---
@dataclass
class Case:
    """One lone-graph case and the premise it claims (asserted on the CPU by
    tests/test_cell_shapes_cpu.py from profile(), before any device sees it)."""
    name: str
    build: object                 # () → gen.Graph
    counts: dict | None = None    # {class: nodes in it}, exact
    pus: dict | None = None       # {residual degree: PUs of exactly that degree}
    tasks: dict | None = None     # {out-degree: tasks of exactly that degree}
    hubs: list | None = None      # the class-6 nodes' degrees, sorted, exact
    degrees: tuple = ()           # degrees some node must have
    n: int | None = None
    positions: int | None = None
    solver: int = 1               # ks_result.solver the device must report (1: the cell solver)


_BUILT: dict = {}


def built(case: Case):
    """The case's graph, built once per process."""
    if case.name not in _BUILT:
        _BUILT[case.name] = case.build()
    return _BUILT[case.name]


BOUNDS_TASKS = [4] * 5 + [5] * 5 + [8] * 5 + [9] * 5


def bounds_pu(d: int):
    pus = [d] * 3 + [d + 1] * 3
    return ladder(pus, fill_tasks(pus), seed=100 + d)


def bounds_tasks():
    return ladder(fill_pus(BOUNDS_TASKS, per=11, pus=10), BOUNDS_TASKS, seed=99)


def bounds_all(pad: int = 0):
    pus = [x for d in CLASS_BOUNDS for x in (d, d, d + 1, d + 1)]
    return ladder(pus, fill_tasks(pus, [4, 5, 8, 9] * 3), pad=pad, seed=98)


BOUNDS_ALL_N = 2 + 24 + 834     # sink, U, 24 PUs, 12 + 822 tasks


def pad_to(mod32: int) -> int:
    """Isolated nodes that bring bounds_all to N ≡ mod32 (mod 32)."""
    return (mod32 - BOUNDS_ALL_N) % 32


def partial(pus, tasks, n0: int, seed: int):
    """ladder(pus, tasks) padded with isolated nodes up to n0 nodes of class 0."""
    g = ladder(pus, tasks, seed=seed)
    have = profile(g).counts[0]
    if have > n0:
        raise ValueError("partial: more class-0 nodes than asked for")
    return ladder(pus, tasks, pad=n0 - have, seed=seed)


def partial_1():    # classes 0–3 hold 1, 129, 1, 1 nodes (the sink is the class-3 node, a 16-position PU the class-2 one)
    tk = [5] * 120
    return partial(fill_pus(tk, [4] + [8] * 9 + [16], per=100, pus=20), tk, 1, 201)


def partial_2():    # 63, 1, 15, 3 (two PUs and the sink in class 3)
    pus = [5] + [9] * 15 + [17] * 2
    return partial(pus, fill_tasks(pus), 63, 202)


def partial_3():    # 64, 63, 16, 4 (three PUs and the sink in class 3)
    tk = [2] * 64 + [5] * 63
    return partial(fill_pus(tk, [32] * 3, per=1000, pus=19), tk, 64, 203)


def partial_4():    # 65, 64, 17, 5 (four PUs and the sink in class 3)
    tk = [2] * 65 + [5] * 64
    return partial(fill_pus(tk, [32] * 4, per=1000, pus=21), tk, 65, 204)


def partial_5():    # 129, 65, 33, 9
    tk = [3] * 129 + [5] * 65
    return partial(fill_pus(tk, [20] * 9, per=1000, pus=42), tk, 129, 205)


# where every (class, count) pair of the partial-item cases occurs
PARTIAL = {"partial-1": (1, 129, 1, 1), "partial-2": (63, 1, 15, 3), "partial-3": (64, 63, 16, 4),
           "partial-4": (65, 64, 17, 5), "partial-5": (129, 65, 33, 9)}


def partial_pairs():
    """{(class, count): case name} — every pair the issue of partial last items needs."""
    out = {}
    for name, cnt in PARTIAL.items():
        for c, k in enumerate(cnt):
            out.setdefault((c, k), name)
    return out


def only_0_and_6():
    return ladder([3] * 600, [3] * 600, seed=301)


def no_4_5():
    pus = [3] * 200 + [7] * 150 + [13] * 100 + [25] * 70
    return ladder(pus, fill_tasks(pus, [6] * 100 + [10] * 50 + [20] * 20), seed=302)


def no_6():
    pus = [4] * 50 + [8] * 30 + [16] * 20 + [32] * 10 + [64] * 6 + [300] * 2
    return ladder(pus, fill_tasks(pus, per=4, tasks=500), seed=303)


def wave_strides():    # PUs of 256, 257 and 512 positions; 511 tasks, so U has 512 too
    pus = [256, 257, 512]
    return ladder(pus, fill_tasks(pus, per=2), seed=304)


def hub_513():         # a PU and U of 513 positions: two class-6 nodes
    pus = [513, 20, 20]
    return ladder(pus, fill_tasks(pus, tasks=512), seed=305)


def hub_4096():        # a PU and U of 4,096 positions: one full round of CT·UC
    pus = [4096] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=4095), seed=306)


def hub_4097():        # a PU and U of 4,097 positions: the arc into the sink is the second round's first
    pus = [4097] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=4096), seed=307)


def hub_6145():        # a PU of 6,145 positions: half of its in-arcs lie in the workgroup's second round
    pus = [6145] + [10] * 40
    return ladder(pus, fill_tasks(pus, per=2, tasks=6200), seed=309)


def hub_three():       # two PUs and U above 512 positions
    pus = [513, 600] + [12] * 10
    return ladder(pus, fill_tasks(pus, tasks=700), seed=308)


def bounded(tasks: int):
    tk = [3] * tasks
    return ladder(fill_pus(tk, per=16), tk, seed=400 + tasks)


def _bounds_case(d):
    return Case("bound-pu-%d" % d, lambda: bounds_pu(d), pus={d: 3, d + 1: 3})


LONE = [_bounds_case(d) for d in CLASS_BOUNDS] + [
    Case("bound-tasks-4-5-8-9", bounds_tasks, tasks={4: 5, 5: 5, 8: 5, 9: 5}),
    Case("bound-all", bounds_all, pus={x: 2 for d in CLASS_BOUNDS for x in (d, d + 1)},
         tasks={5: 3, 8: 3, 9: 3}, n=BOUNDS_ALL_N),
] + [Case(name, globals()[name.replace("-", "_")], counts=dict(enumerate(cnt))) for name, cnt in PARTIAL.items()] + [
    Case("empty-only-0-and-6", only_0_and_6, counts={0: 1200, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 2}, hubs=[601, 601]),
    Case("empty-4-5", no_4_5, counts={4: 0, 5: 0, 6: 2}),
    Case("empty-6", no_6, counts={6: 0}),
    Case("stride-wave-256-257-512", wave_strides, pus={256: 1, 257: 1, 512: 1}, counts={5: 4, 6: 0},
         degrees=(256, 257, 512)),
    Case("stride-hub-513-two-hubs", hub_513, pus={513: 1}, hubs=[513, 513]),
    Case("stride-hub-4096", hub_4096, pus={4096: 1}, hubs=[4096, 4096]),
    Case("stride-hub-4097", hub_4097, pus={4097: 1}, hubs=[4097, 4097]),
    Case("stride-hub-6145", hub_6145, pus={6145: 1}, hubs=[6145, 6201]),
    Case("three-hubs", hub_three, hubs=[513, 600, 701]),
] + [Case("parity-n-mod32-%d" % r, (lambda r=r: bounds_all(pad_to(r))), n=BOUNDS_ALL_N + pad_to(r),
          pus={x: 2 for d in CLASS_BOUNDS for x in (d, d + 1)}) for r in (0, 1, 31)] + [
    Case("bounded-256-tasks", lambda: bounded(256), tasks={3: 256}),
    Case("bounded-257-tasks", lambda: bounded(257), tasks={3: 257}),
]

# the limits: positions (CELL_MAX_POS) and nodes (cell_max_nodes: the LDS of one workgroup)
LIMITS = [
    Case("positions-2^17", lambda: dense(65_536), positions=1 << 17, n=512),
    Case("positions-2^18", lambda: dense(131_072), positions=CELL_MAX_POS, n=768),
    Case("positions-2^18-plus-2", lambda: dense(131_073), positions=CELL_MAX_POS + 2, n=769, solver=0),
    Case("nodes-13000", lambda: sparse(13_000), n=13_000),
    Case("nodes-13300", lambda: sparse(13_300), n=13_300, solver=0),
]


def by_name(name: str) -> Case:
    return next(c for c in LONE + LIMITS if c.name == name)


# ------------------------------------------------------------ batch cells ---
# five cells of different class profiles: bound-pu-64 has classes 2 and 3 empty,
# three-hubs holds three class-6 nodes, and the largest (865 nodes, odd: the LDS
# carve of the whole launch is sized by it) is neither the first nor the last
BATCH_MIXED = ["partial-3", "bound-pu-64", "parity-n-mod32-1", "three-hubs", "empty-6"]
BATCH_UNION_SEEDS = (2, 3, 4)            # gen.quincy(10_000, 1_000, 25, 100, seed): config-2-sized cells
BATCH_INFEASIBLE = ["bound-pu-16", "partial-2", None, "bound-tasks-4-5-8-9", "bound-pu-32"]   # None: the infeasible one


def infeasible_cell():
    """partial-2 with every PU holding one task and U one: 19 places for 52 tasks.
    → (graph, (U, sink, the capacity of U → sink that makes it feasible again))."""
    g = partial_2()
    T = int(task_ids(g).shape[0])
    cap = g.cap.copy()
    cap[g.dst == 1] = 1
    h = gen.Graph(g.ntype, g.supply, g.src, g.dst, g.low, cap, g.cost)
    return h, (2, 1, T)


# ------------------------------------------- segments across a rebuild ---
def slot_capacity(deg: int, alive: bool, task: bool, hint: int, grow: bool) -> int:
    """ks_engine_build.hip:59-66 (k_capacity with slack): seg_capacity, never less than
    the slot had (hint), twice that when an insert overflowed it since the last build."""
    c = seg_capacity(deg, alive, task, 1)
    if grow:
        c = max(c, 2 * max(hint, 4))
    elif hint <= 4 * c:
        c = max(c, hint)
    else:
        c = max(c, hint // 2)
    return (c + 63) // 64 * 64 if c > 64 else c


class Segments:
    """Degrees and segment capacities of a loaded graph's nodes as arcs are added:
    tight after the load (seg_capacity without slack), rebuilt with slack by the first
    solve after an insert met a full segment (ks_store.hip:367-374 flags both ends)."""

    def __init__(self, g):
        self.deg = profile(g).deg.astype(np.int64)
        self.cap = np.asarray([seg_capacity(int(d), True, False, 0) for d in self.deg], np.int64)
        self.task = g.ntype == TASK_T
        self.grow: set = set()
        self.rebuilds = 0
        self.dirty = True          # the load itself: the first solve builds

    def add_arc(self, s: int, d: int):
        for v in (s - 1, d - 1):
            if self.deg[v] + 1 > self.cap[v]:
                self.grow.add(v)
        self.deg[s - 1] += 1
        self.deg[d - 1] += 1

    def solve(self) -> int:
        """→ ks_store_stats.rebuilds after the next solve."""
        if self.grow:
            self.cap = np.asarray([slot_capacity(int(self.deg[v]), True, bool(self.task[v]), int(self.cap[v]),
                                                 v in self.grow) for v in range(self.deg.shape[0])], np.int64)
            self.grow.clear()
            self.rebuilds += 1
        elif self.dirty:
            self.rebuilds += 1
        self.dirty = False
        return self.rebuilds


def rebuild_plan(g):
    """→ (v, tasks): the first PU of exactly 8 positions and, in id order, the tasks
    of out-degree 4 without an arc into it (each gives one new arc t → v)."""
    p = profile(g)
    v = int(next(x for x in pu_ids(g) if p.deg[x - 1] == 8))
    adj = set(g.src[g.dst == v].tolist())
    return v, [int(t) for t in task_ids(g) if p.deg[t - 1] == 4 and int(t) not in adj]
