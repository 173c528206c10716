"""GPU: whole scheduling rounds on one device context against the caller-and-
model of tests/round_ref.py, which never reads the device's graph: the ten-call round, commit →
ks_remove_resources → ks_complete_tasks → ks_add_resources → the capacity refresh → ks_add_tasks →
ks_update_tasks → ks_update_nodes → ks_update_unsched_costs → solve (and the mapping read after
it), for ten rounds of seeded churn with the header's recipes issued from the caller's own
knowledge. The cases with classes carry a cost model that moves: ks_update_nodes lists every
class's and every resource's arcs each round, over arcs the other calls have deleted, re-created
and re-sized on the device alone. After every call the store (ks_get_graph), the bindings
(ks_get_bindings), the call's statistics and its outputs are COMPARED with the model's; after every
solve the cost, the flow, the flows and the mapping are checked against the oracle on the MODEL's
graph before the model takes the mapping. Nothing read from ctx.graph() goes into the model or into
a later call. The single-call suites' twin contexts and second oracles are not repeated here."""
import pytest

from ksched_amd import native
from nodes_ref import CAP_KEEP, offsets3
from round_ref import hub_case, run, small_case, wave_case
from store_ref import same_store
from test_gpu_remove_resources import Snapshot, triples

pytestmark = pytest.mark.gpu

BOTH_MODES = pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
PATHS = {"default": {}, "engine": dict(cell_nodes=-1), "warm": dict(cell_nodes=-1, warm_start=1)}
INVALID = native.KS_E_INVALID


def offsets(lists):
    off, dst, cost = [0], [], []
    for lst in lists:
        dst += [d for d, _ in lst]
        cost += [c for _, c in lst]
        off.append(len(dst))
    return off, dst, cost


class Device:
    """The backend of round_ref.run on a native.Context. Every method compares; none feeds the model."""

    def __init__(self, ctx, warm=False, solver=None, refusals=(), nodes_refusal=None):
        self.ctx, self.warm, self.solver, self.refusals = ctx, warm, solver, set(refusals)
        self.nodes_refusal = nodes_refusal    # the round with one refused ks_update_nodes after the commit
        self.nodes_rebuilds: list = []        # per ks_update_nodes with a record: did rebuilds rise between its end and the next solve's?
        self._nodes_mark = None
        self.solves = self.warm_solves = self.refused = 0
        self.rebuilds_at_solve = None
        self.grow_rebuilds: list = []         # per ks_add_resources step: did ks_store_stats.rebuilds rise by the next call's end?
        self._grow_mark = None

    # -------------------------------------------------------------- the solve ---
    def solve(self, model):
        ctx = self.ctx
        builds = ctx.store_stats()["rebuilds"]
        r = ctx.solve()
        assert r.raw["recoveries"] == 0, "the optimality certificate needed a repair"
        if self.solver is not None:
            assert r.raw["solver"] == self.solver
        if self.warm and self.solves and builds == self.rebuilds_at_solve and not r.raw["rebuilt"]:
            assert r.raw["warm_started"] == 1, "no rebuild intervened: the solve starts from the previous solution"
            self.warm_solves += 1
        self.solves += 1
        self.rebuilds_at_solve = ctx.store_stats()["rebuilds"]
        if self._nodes_mark is not None:                          # only an insert of the call that overflowed a segment can have
            self.nodes_rebuilds.append(self.rebuilds_at_solve > self._nodes_mark)   # asked for a build: nothing after it adds an arc
            self._nodes_mark = None
        f = ctx.flows()
        flows = dict(zip(zip(f["src"].tolist(), f["dst"].tolist()), f["flow"].tolist()))
        return r.cost, r.flow, flows, ctx.task_mapping()

    def idle(self, model, mapping):
        """k == 0 and calls that generate no record keep the solution: the mapping is still served."""
        ctx, aggs = self.ctx, model.aggs
        s0 = ctx.store_stats()
        assert ctx.add_tasks([], [0], [], [], unsched_ids=aggs)["records"] == 0
        assert ctx.update_tasks([], [0], [], [], unsched_ids=aggs)["records"] == 0
        assert ctx.complete_tasks([], resource_caps=False, unsched_ids=aggs)[1]["records"] == 0
        chain_only = [(p, c, 0, 0) for c, p in sorted(model.parent.items())][:3]
        st = ctx.add_resources([], chain_only)
        assert st["records"] == 0 and st["arcs_skipped"] == len(chain_only)
        assert ctx.update_nodes([], [0], [], [], [])["records"] == 0
        assert ctx.task_mapping() == mapping and ctx.store_stats() == s0
        self.compare(model)

    # ------------------------------------------------------------ the refusals ---
    def between(self, model, rnd):
        """One refused call in the middle of a run: a dead root, a task listed twice, an arriving
        task with a dead head. The store and the bindings stay as the model has them; the calls and
        the solve that follow are compared as in every round."""
        if rnd == self.nodes_refusal:
            self.refused_nodes(model)
        if rnd not in self.refusals:
            return
        ctx, aggs = self.ctx, model.aggs
        dead = model.free[0] if model.free else model.top + 3
        s0 = ctx.store_stats()
        with pytest.raises(native.KsError) as e:
            which = sorted(self.refusals).index(rnd)
            if which == 0:
                ctx.remove_resources([model.of_type(4)[0], dead], resource_caps=True, preemptive=model.preemptive)
            elif which == 1:
                t = model.live_tasks()
                ctx.update_tasks([t[0], t[1], t[0]], [0, 1, 1, 2], [model.wildcard, model.wildcard], [5, 5], unsched_ids=aggs)
            else:
                ctx.add_tasks([model.top + 1, model.top + 2], [0, 1, 2], [aggs[0], dead], [7, 7], unsched_ids=aggs)
        assert e.value.code == INVALID, e.value
        assert ctx.store_stats() == s0
        self.refused += 1
        self.compare(model)

    def refused_nodes(self, model):
        """Pinned: KS_CAP_KEEP on a class → machine arc the commit has just deleted (the machine is
        full; the model knows it from its own table). Preemptive: a list that names a dead head."""
        ctx, s0 = self.ctx, self.ctx.store_stats()
        if model.preemptive:
            c, x = model.classes[0], model.free[0] if model.free else model.top + 3
            lst = [(x, 1, 1)]
        else:
            c, x = min(k for k in model.commit_dropped if k[1] in model.alive and k not in model.arcs)
            lst = [(d, 5, CAP_KEEP) for d in sorted({d for (s, d) in model.arcs if s == c} | {x})]
        with pytest.raises(native.KsError) as e:
            ctx.update_nodes([model.wildcard, c], *offsets3([[], lst]))
        assert e.value.code == INVALID and f"node {c}" in str(e.value), e.value
        assert (f"head {x} " if model.preemptive else f"KS_CAP_KEEP") in str(e.value) and str(x) in str(e.value), e.value
        assert ctx.store_stats() == s0
        self.refused += 1
        self.compare(model)

    # --------------------------------------------------------------- the calls ---
    def call(self, model, name, args, expect):
        ctx = self.ctx
        records, superseded = 1, 0
        builds = ctx.store_stats()["rebuilds"]
        if name == "commit":
            assert triples(ctx.scheduling_deltas(commit=False)) == args["deltas"]        # check (c)
            if model.preemptive:
                deltas, st = ctx.commit_preemptive(continuation=args["continuation"], preemption=args["preemption"],
                                                   resource_caps=True, unsched_ids=args["aggs"])
            else:
                deltas, st = ctx.commit_schedule(continuation=args["continuation"], resource_caps=True, unsched_ids=args["aggs"])
            assert triples(deltas) == expect["deltas"]
            assert st == expect["stats"], (st, expect["stats"])
            records = st["records"]
        elif name == "remove":
            removed, evicted, st = ctx.remove_resources(args["roots"], resource_caps=True, preemptive=model.preemptive)
            assert removed.tolist() == expect["removed"] and triples(evicted) == expect["evicted"]
            assert st == expect["stats"], (st, expect["stats"])
        elif name == "get_bindings":
            assert ctx.bindings(args["tasks"]).tolist() == expect["pu"]
            return
        elif name == "apply_deltas":
            ctx.apply_deltas(args["stream"])
        elif name == "complete":
            left, st = ctx.complete_tasks(args["tasks"], resource_caps=args["caps"], preemptive=False, unsched_ids=args["aggs"])
            assert left.tolist() == expect["left"]
            assert st == expect["stats"], (st, expect["stats"])
        elif name == "refresh_caps":
            left, st = ctx.complete_tasks([], resource_caps=True, preemptive=args["preemptive"], unsched_ids=args["aggs"])
            assert st == expect["stats"], (st, expect["stats"])
            records = st["records"]
        elif name == "grow":
            st = ctx.add_resources(args["nodes"], args["edges"])
            assert st == expect["stats"], (st, expect["stats"])
        elif name == "arrive":
            st = ctx.add_tasks(args["tasks"], *offsets(args["lists"]), unsched_ids=args["aggs"], unsched_sink_cost=0)
            assert st == expect["stats"], (st, expect["stats"])
            superseded = expect["superseded"]
        elif name == "refresh":
            st = ctx.update_tasks(args["tasks"], *offsets(args["lists"]), unsched_ids=args["aggs"], unsched_sink_cost=0)
            assert st == expect["stats"], (st, expect["stats"])
            records = st["records"]
        elif name == "nodes":
            st = ctx.update_nodes(args["tails"], *offsets3(args["lists"]))
            assert st == expect["stats"], (st, expect["stats"])
            records = st["records"]
            if records:
                self._nodes_mark = ctx.store_stats()["rebuilds"]
        elif name == "age":
            changed = ctx.update_unsched_costs(args["cost"], mode=args["mode"], continuation=args["continuation"],
                                               unsched_ids=args["aggs"])
            assert changed == expect["changed"], (changed, expect["changed"])
            records = 0
        else:
            raise AssertionError(name)
        if records:                                               # ks_store_stats counts the last stream
            assert ctx.store_stats()["superseded"] == superseded, name
        if self._grow_mark is not None:                           # the call after ks_add_resources: a pending rebuild has run
            self.grow_rebuilds.append(ctx.store_stats()["rebuilds"] > self._grow_mark)
            self._grow_mark = None
        if name == "grow" and args["edges"]:
            self._grow_mark = builds
        self.compare(model)

    def compare(self, model):
        ctx = self.ctx
        same_store(ctx, model.store())
        assert Snapshot(ctx).table == model.arcs
        tasks = model.live_tasks()
        assert ctx.bindings(tasks).tolist() == [model.bindings.get(t, 0) for t in tasks]


def rounds_on_device(model, script, rounds, tmp_path, refusals=(), solver=None, nodes_refusal=None, **opts):
    with native.Context(0, **opts) as ctx:
        ctx.load_graph(model.graph())
        dev = Device(ctx, warm=opts.get("warm_start", 0) == 1, solver=solver, refusals=refusals, nodes_refusal=nodes_refusal)
        dev.compare(model)
        counts = run(model, script, dev, rounds, tmp_path)
        return counts, dev


def check_counters(n, preemptive, rounds=10):
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["pu_id_reused"] > 0
    assert n["aggregator_recreated"] > 0 and n["new_jobs"] >= 1 and n["superseded"] > 0
    if preemptive:
        assert n["running_kept"] > 0
        if rounds >= 10:
            assert n["migrations"] > 0 and n["preemptions"] > 0 and n["stale_caps_repaired"] > 0
    else:
        assert n["ancestor_recreated"] > 0 and n["recipe_upserts"] > 0


# ----------------------------------------------------------------------- cases ---
@BOTH_MODES
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_small_cluster(seed, path, preemptive, tmp_path):
    """2 racks × 3 machines × 1 PU × 2 slots, 3 jobs, 24 tasks, ten rounds. The default path's size
    selects the cell solver; cell_nodes = −1 the engine; with warm_start = 1 every solve that no
    rebuild preceded starts warm."""
    m, s, _ = small_case(preemptive, seed, 10)
    s.feasible = False                                            # the device's solve is the feasibility check here
    n, dev = rounds_on_device(m, s, 10, tmp_path, solver=1 if path == "default" else 0, **PATHS[path])
    check_counters(n, preemptive)
    assert dev.solves == 11
    if path == "warm":
        assert dev.warm_solves > 0


@BOTH_MODES
def test_refusals_in_the_middle_of_a_run(preemptive, tmp_path):
    """Rounds 3, 6 and 9 each make one refused call after the commit: the host's node table rolls
    back over real edits, and everything that follows is compared as in every other round."""
    m, s, _ = small_case(preemptive, 4, 10)
    s.feasible = False
    n, dev = rounds_on_device(m, s, 10, tmp_path, refusals=(3, 6, 9), cell_nodes=-1, warm_start=1)
    assert dev.refused == 3
    check_counters(n, preemptive)


@BOTH_MODES
@pytest.mark.parametrize("path", ["engine", "warm"])
def test_wave_and_class_boundaries(path, preemptive, tmp_path):
    """One job of 150 tasks (its aggregator's residual degree is in the chunked class, above 64),
    one round with 65 arrivals and 65 completions (one more than a wave), and a rack that gains
    machines until its segment overflows: ks_store_stats.rebuilds rises after some
    ks_add_resources and not after others."""
    m, s, rounds = wave_case(preemptive)
    s.feasible = False
    n, dev = rounds_on_device(m, s, rounds, tmp_path, **PATHS[path])
    check_counters(n, preemptive, rounds=6)
    assert any(dev.grow_rebuilds) and not all(dev.grow_rebuilds), dev.grow_rebuilds


@BOTH_MODES
def test_a_hub(preemptive, tmp_path):
    """One aggregator with more than HEAVY_MIN (4,096) arcs: 4,200 waiting tasks on a 60-slot
    cluster, four rounds on the engine; completions and arrivals go through the hub's arcs."""
    m, s, rounds = hub_case(preemptive)
    n, dev = rounds_on_device(m, s, rounds, tmp_path, cell_nodes=-1)
    assert dev.solves == 5 and n["bound_id_reused"] > 0 and n["evictions"] > 0
    assert sum(1 for (_, d) in m.arcs if d == s.hub) > 4096


# ------------------------------------------- the ten-call round: ks_update_nodes ---
CLASS_SEEDS = [17, 19]                                            # two of test_round_ref_cpu.py's


def check_class_counters(n, preemptive):
    """The counters of test_round_ref_cpu.check_class_counters, and those of the plain cases that
    no scripted unique optimum stands behind (this cost model has ties)."""
    assert n["class_arcs_added"] > 0 and n["class_arcs_removed"] > 0 and n["cap_overwritten"] > 0
    assert n["resource_recosted"] > 0 and n["resource_unchanged"] > 0
    assert n["slots_raised"] == 1 and n["slots_lowered"] == 1
    if not preemptive:                                            # (no capacity of 0 and no deleted class arc under the preemptive rule)
        assert n["class_arcs_zeroed"] > 0 and n["class_arc_recreated"] > 0 and n["chain_relisted"] > 0
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["pu_id_reused"] > 0
    assert n["aggregator_recreated"] > 0 and n["superseded"] > 0


@BOTH_MODES
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("seed", CLASS_SEEDS)
def test_small_cluster_with_classes(seed, path, preemptive, tmp_path):
    """The small cluster with 6 slots per PU, one class per job (five by the end) and a cost
    model that moves: every round ks_update_nodes re-lists each class's three machines (one left,
    one joined) with the cost model's capacities and every resource arc with KS_CAP_KEEP, after
    the commit, the removals, the completions with their recipe and the additions have rewritten
    those arcs; round 2 takes slots from a PU and round 6 gives one to a (pinned: full) PU."""
    m, s, _ = small_case(preemptive, seed, 10, classes=True)
    s.feasible = False
    n, dev = rounds_on_device(m, s, 10, tmp_path, solver=1 if path == "default" else 0, **PATHS[path])
    check_class_counters(n, preemptive)
    assert dev.solves == 11 and len(dev.nodes_rebuilds) == 10
    if path == "warm":
        assert dev.warm_solves > 0


@BOTH_MODES
@pytest.mark.parametrize("path", ["engine", "warm"])
def test_wide_class_and_growing_rack(path, preemptive, tmp_path):
    """wave_case with classes. The 150-task job's class holds more than 64 arcs (its tasks' and
    its machines'), so the walk for its unlisted arc goes over a chunked segment; the class of the
    job that round 4 brings prefers every machine of the growing rack from its first call on, some
    fifty additions (pinned: the dozen into machines with room) into a segment the store has just
    sized for the one or two tasks pointing at it: ks_store_stats.rebuilds rises after that
    ks_update_nodes and not after others."""
    m, s, rounds = wave_case(preemptive, classes=True)
    s.feasible = False
    n, dev = rounds_on_device(m, s, rounds, tmp_path, **PATHS[path])
    assert n["class_tail_over_64"] > 0 and n["class_arcs_added"] > 0 and n["resource_recosted"] > 0
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["superseded"] > 0
    print("rebuilds after ks_update_nodes:", dev.nodes_rebuilds, "after ks_add_resources:", dev.grow_rebuilds)
    assert dev.nodes_rebuilds[4] and not all(dev.nodes_rebuilds), dev.nodes_rebuilds
    assert any(dev.grow_rebuilds) and not all(dev.grow_rebuilds), dev.grow_rebuilds


@BOTH_MODES
def test_a_refused_update_nodes_in_the_middle_of_a_run(preemptive, tmp_path):
    """Round 3, after the commit: KS_CAP_KEEP on a class arc the pinned commit has just deleted, or
    (preemptive) a dead head. KS_E_INVALID, the store's counters and the graph stand, and the rest
    of the run is compared as usual."""
    m, s, _ = small_case(preemptive, CLASS_SEEDS[0], 10, classes=True)
    s.feasible = False
    n, dev = rounds_on_device(m, s, 10, tmp_path, nodes_refusal=3, cell_nodes=-1, warm_start=1)
    assert dev.refused == 1 and dev.solves == 11 and dev.warm_solves > 0
    check_class_counters(n, preemptive)
