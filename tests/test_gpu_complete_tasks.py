"""GPU: ks_complete_tasks — finished tasks leave the device-resident graph, their
aggregators lose a unit each, the resource arcs get their capacities — and ks_get_bindings,
against the rule restated on the host (tests/complete_ref.py), against the store's reference
(tests/store_ref.py) and against the host path it replaces (the same records through
ks_apply_deltas on a twin context). The harness is that of test_gpu_remove_resources.py:
every case runs before any solve, after a solve with a commit on the cell path and on the
engine path, and with warm_start = 1, under both capacity rules."""
import numpy as np
import pytest

from complete_ref import chain_upserts, complete_reference, parent_chains
from ksched_amd import native
from oracle import ko, sched_ref
from preempt_ref import table_graph
from remove_ref import TOY_ARCS, TOY_BINDINGS, TOY_NTYPE, TOY_SUPPLY, TOY_U, BelowLowerBound
from store_ref import check_counters, same_store
from test_gpu_remove_resources import BOTH_MODES, EVERY_STATE, STATES, TOY, Snapshot, Spec, prepare, triples

pytestmark = pytest.mark.gpu

CAPS = pytest.mark.parametrize("caps", [True, False], ids=["caps", "nocaps"])


# ---------------------------------------------------------------------- graphs ---
class Jobs(Spec):
    """SINK 1, X 2, R racks, R·mpr machines (machine k in rack k // mpr), one PU each, J
    unscheduled aggregators, then the tasks (job, desig, wide, agg_first). A task with a
    designated machine has arcs into its aggregator (100), X (50), the machine (1) and, in
    the running form, its running arc: with room there the optimum places it on that
    machine. A task without one waits: `wide` arcs into machines 0 … wide − 1 (500 each:
    never taken) and its aggregator arc, created after them or, agg_first, before."""

    def __init__(self, R, mpr, slots, J, tasks):
        M = R * mpr
        self.SINK, self.X, self.R0 = 1, 2, 3
        self.M0 = self.R0 + R
        self.P0 = self.M0 + M
        self.U0 = self.P0 + M
        self.T0 = self.U0 + J
        T = len(tasks)
        n = self.T0 + T - 1
        ntype, supply = [0] * n, [0] * n
        ntype[0], supply[0] = 3, -T
        for k in range(M):
            ntype[self.M0 + k - 1], ntype[self.P0 + k - 1] = 4, 2
        for i in range(T):
            ntype[self.T0 + i - 1], supply[self.T0 + i - 1] = 1, 1
        per_job = [sum(1 for t in tasks if t[0] == j) for j in range(J)]
        arcs = [((self.U0 + j, self.SINK), (0, per_job[j], 0, 0)) for j in range(J)]
        self.topology = {}
        for r in range(R):
            self.topology[(self.X, self.R0 + r)] = (0, mpr * slots, 0, 0)
            for j in range(mpr):
                k = r * mpr + j
                self.topology[(self.R0 + r, self.M0 + k)] = (0, slots, 0, 0)
                self.topology[(self.M0 + k, self.P0 + k)] = (0, slots, 0, 0)
        arcs += list(self.topology.items())
        arcs += [((self.P0 + k, self.SINK), (0, slots, 0, 0)) for k in range(M)]
        bindings = {}
        for i, (job, desig, wide, agg_first) in enumerate(tasks):
            t = self.T0 + i
            agg = ((t, self.U0 + job), (0, 1, 100, 0))
            if desig is not None:
                arcs += [agg, ((t, self.X), (0, 1, 50, 0)), ((t, self.M0 + desig), (0, 1, 1, 0)),
                         ((t, self.P0 + desig), (0, 1, 0, 1))]
                bindings[t] = self.P0 + desig
            else:
                prefs = [((t, self.M0 + k), (0, 1, 500, 0)) for k in range(wide)]
                arcs += [agg] + prefs if agg_first else prefs + [agg]
        assert all(list(bindings.values()).count(p) <= slots for p in set(bindings.values()))
        super().__init__(ntype, supply, arcs, bindings)

    def task(self, i):
        return self.T0 + i


# --------------------------------------------------------------------- harness ---
def balanced(snap):
    """The snapshot as a full graph; the sink's demand as auto_sink sets it at the solve."""
    supply = snap.supply.copy()
    sink = int(np.nonzero(snap.ntype == 3)[0][0])
    supply[sink] = 0
    supply[sink] = -int(supply.sum())
    return table_graph(snap.ntype, supply, snap.table)


def live_tasks(snap) -> list:
    return [int(i) for i in sorted(snap.alive) if snap.ntype[i - 1] == 1]


def complete_and_check(ctx, tasks, bindings, preemptive, caps=True, unsched_ids=None):
    """One call against the rule, the store's reference and the host path; → (the rule's
    result, the device's (left, stats), the graph after)."""
    before = Snapshot(ctx)
    ref = complete_reference(before.graph(), tasks, bindings, caps, preemptive and caps, unsched_ids, alive=before.alive)
    sref = before.store()
    want = sref.apply(ref.stream)
    assert want["superseded"] == 0
    with native.Context(0) as twin:                               # the host path: the same records
        twin.load_arrays(before.nodes, before.arcs)
        twin.apply_deltas(ref.stream)
        same_store(twin, sref)
        twin_rows = Snapshot(twin).table
    left, stats = ctx.complete_tasks(tasks, resource_caps=caps, preemptive=preemptive and caps, unsched_ids=unsched_ids)
    assert left.tolist() == ref.left
    assert stats == ref.stats
    assert stats["records"] == stats["tasks"] + stats["unsched_updates"] + stats["cap_updates"]
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == before.alive - set(ref.removed)
    check_counters(ctx.store_stats(), want, exact=True)
    rest = live_tasks(after)
    assert dict(zip(rest, ctx.bindings(rest).tolist())) == {t: ref.bindings.get(t, 0) for t in rest}
    return ref, (left, stats), after


def resolve_and_check(ctx, ref, state):
    """The solve after the call: cost, flow, the flows and the scheduling deltas against the
    oracle and the rule's bindings."""
    r = ctx.solve()
    snap = Snapshot(ctx)
    g = balanced(snap)
    st, cost, flow, _ = ko.cost_scaling(g)
    assert st == 0 and (r.cost, r.flow) == (cost, flow)
    f = ctx.flows()
    got = dict(zip(zip(f["src"].tolist(), f["dst"].tolist()), f["flow"].tolist()))
    vec = np.asarray([got.pop((int(s), int(d)), 0) for s, d in zip(g.src, g.dst)], np.int64)
    assert not got
    vst, vcost, _ = ko.verify(g, vec)
    assert (vst, vcost) == (0, cost)
    d = triples(ctx.scheduling_deltas(commit=False))
    assert d == sched_ref.scheduling_deltas(ref.bindings, ctx.task_mapping(), live_tasks(snap))
    if state == "warm":
        assert r.raw["warm_started"] == 1
    return r


def run_case(spec, tasks, state, preemptive, caps=True, unsched_ids=None):
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, preemptive)
        ref, dev, after = complete_and_check(ctx, tasks, bindings, preemptive, caps, unsched_ids)
        resolve_and_check(ctx, ref, state)
        return ref, dev, after, bindings


# ----------------------------------------------------------------------- cases ---
@EVERY_STATE
@BOTH_MODES
@CAPS
def test_toy_running_and_waiting(state, preemptive, caps):
    ref, (left, stats), after, _ = run_case(TOY, [14, 18], state, preemptive, caps)
    assert stats["tasks"] == 2
    if state == "fresh":                                           # the literals of the CPU suite
        assert left.tolist() == [9, 0] and stats["bound"] == 1 and stats["arcs_removed"] == 8
        assert after.table[(13, 1)] == (0, 4, 0, 0) and stats["unsched_updates"] == 1
        if caps and not preemptive:
            assert after.table[(5, 9)] == after.table[(3, 5)] == (0, 1, 0, 0) and after.table[(2, 3)] == (0, 2, 0, 0)
        else:
            assert stats["cap_updates"] == 0


def chunked() -> Jobs:
    """Waiting tasks with 130 (three chunks), 63, 64 and 65 out-arcs whose aggregator arc was
    created last, one of 130 with it first, between running neighbours of two jobs."""
    tasks = [(0, 0, 0, False), (1, None, 129, False), (0, 1, 0, False), (1, None, 62, False), (1, None, 63, False),
             (0, None, 64, False), (1, 2, 0, False), (0, None, 129, True), (1, None, 1, False), (0, 3, 0, False)]
    return Jobs(2, 70, 2, 2, tasks)


@EVERY_STATE
@BOTH_MODES
def test_chunked_segments(state, preemptive):
    spec = chunked()
    done = [spec.task(i) for i in (1, 3, 4, 5, 7, 2, 8)]
    ref, (left, stats), after, bindings = run_case(spec, done, state, preemptive)
    assert stats["tasks"] == 7 and stats["bound"] == 1
    assert left.tolist() == [0, 0, 0, 0, 0, bindings[spec.task(2)], 0]
    # each job had 5 tasks; job 0 loses two waiting tasks and a running one, job 1 four waiting ones
    if state == "fresh" or preemptive:
        assert after.table[(spec.U0, 1)] == (0, 2, 0, 0) and after.table[(spec.U0 + 1, 1)] == (0, 1, 0, 0)
    else:   # the pinned commit took the running tasks' units: 2 − 2 and 4 − 4, both arcs go
        assert (spec.U0, 1) not in after.table and (spec.U0 + 1, 1) not in after.table


def crowded() -> Jobs:
    """70 tasks of job 0 (40 running, 30 waiting), then jobs 1, 2, 3 interleaved (30 tasks,
    every other one waiting): several waves meet on one aggregator's counter."""
    tasks = [(0, i % 20, 0, False) if i < 40 else (0, None, 2, False) for i in range(70)]
    tasks += [(1 + i % 3, 20 + i % 10 if i % 2 else None, 3, False) for i in range(30)]
    return Jobs(2, 15, 4, 4, tasks)


@EVERY_STATE
@BOTH_MODES
def test_one_job_ends_and_three_are_interleaved(state, preemptive):
    """Every task of job 0 completes: its aggregator → sink arc falls to 0 and is removed."""
    spec = crowded()
    done = [spec.task(i) for i in range(70)] + [spec.task(70 + i) for i in range(0, 20, 2)] + [spec.task(71)]
    ref, (left, stats), after, _ = run_case(spec, done, state, preemptive)
    assert stats["tasks"] == 81 and stats["bound"] == 41
    assert (spec.U0, 1) not in after.table
    assert stats["unsched_updates"] == 4
    assert all((spec.U0 + j, 1) in after.table for j in (1, 2, 3))


@EVERY_STATE
@BOTH_MODES
def test_three_hundred_completions(state, preemptive):
    """More ids than one workgroup holds, their order shuffled."""
    tasks = [(i % 3, i % 20 if i % 4 else None, 1 + i % 5, bool(i % 2)) for i in range(320)]
    spec = Jobs(2, 10, 17, 3, tasks)
    order = [(i * 77) % 320 for i in range(320)]
    done = [spec.task(i) for i in order if i % 16 != 5]
    assert len(done) == 300
    ref, (left, stats), after, _ = run_case(spec, done, state, preemptive)
    assert stats["tasks"] == 300 and stats["bound"] == sum(1 for i in order if i % 16 != 5 and i % 4)
    assert len([t for t in after.alive if after.ntype[t - 1] == 1]) == 20


@EVERY_STATE
@BOTH_MODES
def test_explicit_aggregators_against_the_null_rule(state, preemptive):
    spec = crowded()
    done = [spec.task(i) for i in range(35, 80)]
    every = [spec.U0 + j for j in range(4)]
    a, _, after_null, _ = run_case(spec, done, state, preemptive)
    b, _, after_ids, _ = run_case(spec, done, state, preemptive, unsched_ids=every)
    assert after_null.table == after_ids.table and a.stats == b.stats
    c, (_, stats), after_two, _ = run_case(spec, done, state, preemptive, unsched_ids=every[:2])
    assert after_two.table[(spec.U0 + 2, 1)][1] > after_null.table[(spec.U0 + 2, 1)][1]   # job 2 was not named
    assert stats["unsched_updates"] <= 2


@EVERY_STATE
@BOTH_MODES
def test_an_id_twice_and_its_reuse(state, preemptive):
    """A repeated id is removed once and both entries of left name its PU; the id can be
    added again, and the new task is unbound."""
    spec = chunked()
    t, w = spec.task(0), spec.task(8)
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, preemptive)
        ref, (left, stats), after = complete_and_check(ctx, [t, w, t, t], bindings, preemptive)
        assert stats["tasks"] == 2 and left.tolist() == [bindings[t], 0, bindings[t], bindings[t]] and bindings[t]
        rows = [(native.KS_ADD_NODE, t, 0, 0, 0, 0, 0, 1, 1), (native.KS_ADD_ARC, 0, t, spec.U0, 0, 1, 100, 0, 0),
                (native.KS_ADD_ARC, 0, t, spec.M0 + 5, 0, 1, 1, 0, 0),
                (native.KS_ADD_ARC, 0, spec.U0, 1, 0, after.table[(spec.U0, 1)][1] + 1, 0, 0, 0)]
        recs = np.zeros(len(rows), native.DELTA_DT)
        for x, (kind, nid, s, d, lo, cap, co, ty, ex) in zip(recs, rows):
            x["kind"], x["id"], x["src"], x["dst"], x["low"], x["cap"], x["cost"], x["type"], x["excess"] = \
                kind, nid, s, d, lo, cap, co, ty, ex
        ctx.apply_deltas(recs)
        assert ctx.bindings([t]).tolist() == [0]
        r = ctx.solve()
        snap = Snapshot(ctx)
        st, cost, flow, _ = ko.cost_scaling(balanced(snap))
        assert st == 0 and (r.cost, r.flow) == (cost, flow)
        assert ctx.task_mapping().get(t) == spec.P0 + 5
        with pytest.raises(native.KsError) as e:                    # w stays dead
            ctx.bindings([t, w])
        assert e.value.code == native.KS_E_INVALID


@EVERY_STATE
@BOTH_MODES
def test_no_task_is_a_plain_refresh(state, preemptive):
    """k == 0 with the flag: a resource capacity that ks_apply_deltas set wrong comes back;
    with every capacity right, and without the flag, nothing happens and the solution stands."""
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, TOY, state, preemptive)
        if state == "fresh" and not preemptive:                     # (the toy's running form carries the slots)
            ctx.complete_tasks([], resource_caps=True)
        good = Snapshot(ctx).table
        key = next(k for k in ((2, 4), (2, 3)) if k in good)
        lo, cap, co, ty = good[key]
        rec = np.zeros(1, native.DELTA_DT)
        rec[0]["kind"], rec[0]["src"], rec[0]["dst"], rec[0]["low"], rec[0]["cap"], rec[0]["cost"], rec[0]["type"] = \
            native.KS_UPDATE_ARC, key[0], key[1], lo, cap + 3, co, ty
        ctx.apply_deltas(rec)
        ref, (left, stats), after = complete_and_check(ctx, [], bindings, preemptive)
        assert left.shape[0] == 0
        assert stats == dict(tasks=0, bound=0, arcs_removed=0, unsched_updates=0, cap_updates=1, records=1)
        assert after.table == good
        resolve_and_check(ctx, ref, state)
        s0 = ctx.store_stats()
        d0 = ctx.scheduling_deltas(commit=False)
        for caps in (True, False):
            left, stats = ctx.complete_tasks([], resource_caps=caps, preemptive=preemptive and caps)
            assert left.shape[0] == 0 and not any(stats.values())
            assert ctx.store_stats() == s0 and Snapshot(ctx).table == good
            assert (ctx.scheduling_deltas(commit=False) == d0).all()   # the solution stands


def full_pu() -> Jobs:
    """Machine 0 (2 slots) runs two tasks: after a pinned commit neither M0 → P0 nor
    R0 → M0 is in the store. Machine 1 runs one."""
    return Jobs(2, 2, 2, 1, [(0, 0, 0, False), (0, 0, 0, False), (0, 1, 0, False), (0, None, 1, False)])


@pytest.mark.parametrize("state", ["cell", "engine", "warm"])
@pytest.mark.parametrize("recipe", [False, True], ids=["arcless", "recipe"])
def test_pinned_full_pu(state, recipe):
    spec = full_pu()
    t = spec.task(0)
    chain_keys = [(spec.M0, spec.P0), (spec.R0, spec.M0), (spec.X, spec.R0)]
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, False)
        held = Snapshot(ctx)
        assert chain_keys[0] not in held.table and chain_keys[1] not in held.table
        if recipe:
            pus = ctx.bindings([t]).tolist()                        # 1. the finishing tasks' PUs
            assert pus == [spec.P0]
            chain = parent_chains(spec.ntype, spec.topology, pus)
            assert sorted(chain) == sorted(chain_keys)
            ctx.apply_deltas(chain_upserts(spec.topology, chain, cap=7))   # 2. any positive capacity
        ref, _, after = complete_and_check(ctx, [t], bindings, False)     # 3. every one to its right value
        if recipe:
            # the rule on the full graph: the store's arcs plus the topology the host never lost
            full = dict(held.table)
            for k, a in spec.topology.items():
                full.setdefault(k, a)
            want = complete_reference(table_graph(held.ntype, held.supply, full), [t], bindings, True, False,
                                      alive=held.alive)
            for k in chain_keys:
                assert after.table[k] == want.arcs[k]
            assert after.table[chain_keys[0]] == after.table[chain_keys[1]] == (0, 1, 0, 0)
            assert after.table[chain_keys[2]] == (0, 2, 0, 0)
        else:
            assert chain_keys[0] not in after.table and chain_keys[1] not in after.table
        resolve_and_check(ctx, ref, state)


# -------------------------------------------------------------------- refusals ---
def test_refusals_change_nothing():
    g = TOY.graph(running=True)
    with native.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        ctx.load_graph(g)
        ctx.set_bindings(TOY_BINDINGS)
        left, _ = ctx.complete_tasks([19], resource_caps=False)     # a dead id for later
        assert left.tolist() == [0]
        ctx.solve()
        before = Snapshot(ctx)
        d0 = ctx.scheduling_deltas(commit=False)
        s0 = ctx.store_stats()
        b0 = ctx.bindings(live_tasks(before)).tolist()
        assert b0 == [9, 9, 10, 11, 0]

        def unchanged():
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive
            assert (now.nodes == before.nodes).all()
            assert ctx.store_stats() == s0
            assert ctx.bindings(live_tasks(now)).tolist() == b0
            assert (ctx.scheduling_deltas(commit=False) == d0).all()    # the bindings and the solution stand

        out = np.full(8, 77, np.uint64)

        def call(flags, tasks, null=False):
            ids = np.asarray(tasks, np.uint64)
            return L.ks_complete_tasks(h, flags, None if null else ids.ctypes.data, ids.shape[0], None, 0,
                                       out.ctypes.data, None)

        for bad in (19, 9, 0, 10 ** 6, 13, 1):                      # dead, a PU, 0, beyond, an aggregator, the sink
            for flags in (0, 1, 3):
                assert call(flags, [14, bad, 0]) == native.KS_E_INVALID
                assert f"task {bad} " in L.ks_last_error(h).decode()
                unchanged()
        for flags in (4, 2, 1 | 8):                                 # unknown bits, PREEMPTIVE alone
            assert call(flags, [14]) == native.KS_E_INVALID
            unchanged()
        assert call(1, [14], null=True) == native.KS_E_INVALID      # a null array with k > 0
        unchanged()
        assert out.tolist() == [77] * 8                             # left is written on success only
        pu = np.zeros(2, np.uint64)
        for bad in (19, 9, 0, 10 ** 6):
            ids = np.asarray([14, bad], np.uint64)
            assert L.ks_get_bindings(h, ids.ctypes.data, pu.ctypes.data, 2) == native.KS_E_INVALID
            assert str(bad) in L.ks_last_error(h).decode()
        unchanged()


def test_an_aggregator_capacity_below_its_lower_bound_is_refused():
    arcs = dict(TOY_ARCS)
    arcs[(TOY_U, 1)] = (1, 1, 0, 0)                                 # U → sink: low 1, cap 1
    spec = Spec(TOY_NTYPE, TOY_SUPPLY, list(arcs.items()), TOY_BINDINGS)
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(TOY_BINDINGS)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        with pytest.raises(BelowLowerBound):
            complete_reference(before.graph(), [18], TOY_BINDINGS, False, False)
        for caps, preemptive in ((False, False), (True, False), (True, True)):
            with pytest.raises(native.KsError) as e:
                ctx.complete_tasks([18], resource_caps=caps, preemptive=preemptive)
            assert e.value.code == native.KS_E_VERIFY
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive
            assert {k: v for k, v in ctx.store_stats().items() if k not in ("rebuilds", "residual_slots")} == \
                   {k: v for k, v in s0.items() if k not in ("rebuilds", "residual_slots")}
            assert ctx.bindings([14, 15, 18]).tolist() == [9, 9, 0]
        left, stats = ctx.complete_tasks([18], resource_caps=False, unsched_ids=[])   # no aggregator named: it goes
        assert left.tolist() == [0] and stats["unsched_updates"] == 0


def test_a_resource_capacity_below_its_lower_bound_is_refused():
    arcs = dict(TOY_ARCS)
    arcs[(2, 3)] = (3, 4, 0, 0)                                     # X → R1: low 3, slots − running below is 2
    spec = Spec(TOY_NTYPE, TOY_SUPPLY, list(arcs.items()), TOY_BINDINGS)
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(TOY_BINDINGS)
        before = Snapshot(ctx)
        with pytest.raises(native.KsError) as e:
            ctx.complete_tasks([14], resource_caps=True, preemptive=False)
        assert e.value.code == native.KS_E_VERIFY
        now = Snapshot(ctx)
        assert now.table == before.table and now.alive == before.alive
        complete_and_check(ctx, [14], TOY_BINDINGS, True)           # slots below: 4 ≥ 3


def test_two_sinks_refuse_the_capacities():
    ntype = list(TOY_NTYPE) + [3]
    supply = list(TOY_SUPPLY) + [0]
    spec = Spec(ntype, supply, list(TOY_ARCS.items()) + [((13, 20), (0, 3, 0, 0))], TOY_BINDINGS)
    with native.Context(0, auto_sink=0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(TOY_BINDINGS)
        before = Snapshot(ctx)
        for tasks in ([14, 18], []):
            with pytest.raises(native.KsError) as e:
                ctx.complete_tasks(tasks)
            assert e.value.code == native.KS_E_INVALID
            assert Snapshot(ctx).table == before.table and Snapshot(ctx).alive == before.alive
        ref, (left, stats), after = complete_and_check(ctx, [14, 18], TOY_BINDINGS, False, caps=False)
        assert left.tolist() == [9, 0] and stats["unsched_updates"] == 2    # both arcs into a sink lose the units
        assert after.table[(13, 1)] == (0, 4, 0, 0) and after.table[(13, 20)] == (0, 1, 0, 0)
