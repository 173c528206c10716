"""GPU: ks_update_tasks — live tasks' arcs are added, re-costed and dropped as their lists say,
and an evicted task's unit returns to its aggregator — against the rule restated on the host
(tests/refresh_ref.py), against the store's reference (tests/store_ref.py) and against the host
path it replaces (the same records through ks_apply_deltas on a twin context). The harness is
that of test_gpu_add_tasks.py: every case runs after a solve with a commit on the cell path and on
the engine path and with warm_start = 1, after a pinned and a preemptive commit where the mode
matters."""
import numpy as np
import pytest

from arrive_ref import offsets
from ksched_amd import native
from refresh_ref import KEEP_UNLISTED, refresh_reference
from store_ref import check_counters, same_store
from test_gpu_add_tasks import AFTER_A_COMMIT, aggregators, cluster, priced, resolve_and_check
from test_gpu_complete_tasks import Jobs, live_tasks
from test_gpu_remove_resources import BOTH_MODES, STATES, Snapshot, Spec, prepare

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------- harness ---
def held(snap, t, running=False) -> list:
    """The task's out-arcs as a list for the call: (head, cost), without the running arc."""
    return [(d, a[2]) for (s, d), a in snap.table.items() if s == t and (running or a[3] != 1)]


def bound(ctx) -> dict:
    tasks = live_tasks(Snapshot(ctx))
    return dict(zip(tasks, ctx.bindings(tasks).tolist()))


def update_and_check(ctx, tasks, lists, unsched_ids, sink_cost=0, keep=False, met_csr=False, solve=True):
    """One call against the rule, the store's reference and the host path, then the solve after
    it against the oracle; → (the rule's result, the device's stats, the graph after, the solve)."""
    before = Snapshot(ctx)
    bindings = bound(ctx)
    ref = refresh_reference(before.ntype, before.table, tasks, lists, bindings, unsched_ids, sink_cost,
                            KEEP_UNLISTED if keep else 0, alive=before.alive)
    sref = before.store()
    want = sref.apply(ref.stream)
    assert want["superseded"] == 0
    with native.Context(0) as twin:                               # the host path: the same records
        twin.load_arrays(before.nodes, before.arcs)
        if ref.stream.shape[0]:
            twin.apply_deltas(ref.stream)
        same_store(twin, sref)
        twin_rows = Snapshot(twin).table
    s0 = ctx.store_stats()
    off, dst, cost = offsets(lists)
    stats = ctx.update_tasks(tasks, off, dst, cost, unsched_ids=unsched_ids, unsched_sink_cost=sink_cost,
                             keep_unlisted=keep)
    assert stats == ref.stats
    assert stats["records"] == (stats["arcs_added"] + stats["cost_updates"] + stats["arcs_removed"] +
                                stats["unsched_updates"] + stats["unsched_added"])
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == before.alive and (after.nodes == before.nodes).all()
    assert bound(ctx) == bindings
    counters = ctx.store_stats()                                  # (before the solve: its auto-sink edit is a stream)
    if keep:
        assert counters["rebuilds"] == s0["rebuilds"]             # the flag needs no residual CSR
    if not stats["records"]:
        assert counters == s0
        return ref, stats, after, None
    assert counters["superseded"] == 0
    r = resolve_and_check(ctx) if solve else None
    # exact: the stream met a valid CSR and fit its slack (no build since)
    check_counters(counters, want, exact=solve and met_csr and ctx.store_stats()["rebuilds"] == counters["rebuilds"])
    return ref, stats, after, r


def evict(ctx, spec, indices, preemptive) -> list:
    """The machines of the spec's tasks leave the graph, and their PUs by name: under the pinned
    rule a full machine has lost its arc into its PU; → the evicted task ids."""
    pus = [spec.bindings[spec.task(i)] for i in indices]
    roots = [p - spec.P0 + spec.M0 for p in pus] + pus
    _, evicted, _ = ctx.remove_resources(roots, resource_caps=True, preemptive=preemptive)
    assert sorted(evicted["task"].tolist()) == [spec.task(i) for i in indices]
    return [spec.task(i) for i in indices]


def wishes(spec, job, length, first_machine=0) -> list:
    """A list: the aggregator (100), then length − 1 machines from the far end (500 + k: never taken)."""
    if length == 0:
        return []
    return [(spec.U0 + job, 100)] + [(spec.M0 + 139 - first_machine - k, 500 + k) for k in range(length - 1)]


# ----------------------------------------------------------------------- cases ---
@AFTER_A_COMMIT
@BOTH_MODES
def test_list_lengths(state, preemptive):
    """0, 1, 63, 64, 65 and 130 listed arcs mixed in one call: the arc → task bisection over
    offsets that repeat (the empty list) and that cross a wave and a workgroup. Waiting tasks
    hold arcs the lists keep, re-cost and drop; pinned, the running tasks list only new heads."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, preemptive)
        lengths = [65, 0, 1, 130, 63, 0, 64, 2]
        tasks = [spec.task(i) for i in range(8)]
        lists = []
        for i, L in enumerate(lengths):
            lst = wishes(spec, i % 3, L, first_machine=i)
            if L > 2 and i % 2 == 0:                               # a waiting task: one held arc re-costed, one kept
                lst = lst[:-2] + [(spec.M0, 123), (spec.M0 + 1, 500)]
            if not preemptive and i % 2 and lst:                   # a pinned task has no aggregator arc: it gains none
                lst = lst[1:]
            lists.append(lst)
        ref, stats, after, _ = update_and_check(ctx, tasks, lists, aggregators(spec), met_csr=True)
        assert stats["cost_updates"] >= 3 and stats["arcs_removed"] >= 2 and stats["arcs_added"] > 250
        assert stats["unsched_updates"] == stats["unsched_added"] == 0
        assert after.table[(tasks[3], spec.M0 + 139 - 3 - 128)][:2] == (0, 1)


def wide() -> Jobs:
    """Task 1 waits with 69 machine arcs and its aggregator arc: 70 held arcs, two 64-position chunks."""
    return Jobs(2, 70, 2, 2, [(0, 3, 0, False), (1, None, 69, False), (0, None, 2, False), (1, 9, 0, False)])


@AFTER_A_COMMIT
@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
def test_seventy_held_arcs_three_stay_listed(state, keep):
    spec = wide()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        t = spec.task(1)
        assert len(held(Snapshot(ctx), t)) == 70
        lst = [(spec.M0, 500), (spec.M0 + 34, 7), (spec.M0 + 68, 500)]
        ref, stats, after, _ = update_and_check(ctx, [t], [lst], aggregators(spec), keep=keep, met_csr=state == "warm")
        assert stats["arcs_removed"] == (0 if keep else 66) and stats["cost_updates"] == 1 and stats["arcs_unchanged"] == 2
        assert len(held(after, t)) == (70 if keep else 4)          # the three and the aggregator arc
        assert after.table[(t, spec.U0 + 1)] == (0, 1, 100, 0)


def one_job(k) -> Jobs:
    """k + 1 tasks of job 0, task i on machine i of one slot, the last one waiting; job 1 waits."""
    return Jobs(2, 70, 1, 2, [(0, i, 0, False) for i in range(k)] + [(0, None, 2, False), (1, None, 2, False)])


@AFTER_A_COMMIT
@pytest.mark.parametrize("k", [1, 64, 65])
def test_one_jobs_evicted_tasks_regain_their_unit(state, k):
    """k tasks of one job are evicted after a pinned commit and listed with their aggregator
    arc: the gains fill one wave exactly (64) and spill one lane into the next (65). The
    capacity rises by exactly k."""
    spec = one_job(k)
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        tasks = evict(ctx, spec, range(k), False)
        snap = Snapshot(ctx)
        assert all(not held(snap, t, running=True) for t in tasks) and snap.table[(spec.U0, 1)] == (0, 1, 0, 0)
        lists = [[(spec.U0, 100), (spec.X, 50)]] * k
        ref, stats, after, r = update_and_check(ctx, tasks, lists, aggregators(spec))
        assert after.table[(spec.U0, 1)] == (0, 1 + k, 0, 0)
        assert (stats["arcs_added"], stats["unsched_updates"], stats["records"]) == (2 * k, 1, 2 * k + 1)


@AFTER_A_COMMIT
def test_three_aggregators_interleaved_in_one_wave(state):
    """61 evicted tasks of three jobs in one call; jobs 0 and 1 still have a waiting task (their
    arcs into the sink are raised), job 2 was drained by the pin (its arc is re-created)."""
    jobs = [(i * 7) % 3 if i % 5 else 2 for i in range(61)]
    spec = Jobs(2, 70, 1, 3, [(j, i, 0, False) for i, j in enumerate(jobs)] + [(0, None, 2, False), (1, None, 2, False)])
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        tasks = evict(ctx, spec, range(61), False)
        assert (spec.U0 + 2, 1) not in Snapshot(ctx).table
        lists = [[(spec.X, 50), (spec.U0 + j, 100)] for j in jobs]
        ref, stats, after, _ = update_and_check(ctx, tasks, lists, aggregators(spec), sink_cost=13)
        assert [after.table[(spec.U0 + j, 1)] for j in range(3)] == [(0, 1 + jobs.count(0), 0, 0), (0, 1 + jobs.count(1), 0, 0),
                                                                    (0, jobs.count(2), 13, 0)]
        assert (stats["unsched_updates"], stats["unsched_added"]) == (2, 1) and min(jobs.count(j) for j in range(3)) > 5


@AFTER_A_COMMIT
@pytest.mark.parametrize("null_rule", [False, True], ids=["ids", "null"])
def test_a_present_aggregator_arc_keeps_its_bound_and_cost(state, null_rule):
    """Job 1's arc into the sink carries low 1 and cost 40; an evicted task listed into it raises its capacity."""
    spec = priced()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        (t,) = evict(ctx, spec, [3], False)
        lo, cap0, co, ty = Snapshot(ctx).table[(spec.U0 + 1, 1)]
        assert (lo, co) == (1, 40)
        ref, stats, after, _ = update_and_check(ctx, [t], [[(spec.U0 + 1, 100), (spec.X, 50)]],
                                                None if null_rule else aggregators(spec), sink_cost=77)
        assert after.table[(spec.U0 + 1, 1)] == (1, cap0 + 1, 40, 0)
        assert stats["unsched_updates"] == 1 and stats["unsched_added"] == 0


def raw_call(ctx, tasks, lists, ids, sink_cost=0, flags=0, off=None):
    L, h = ctx._L, ctx._h
    t = np.asarray(tasks, np.uint64)
    o, dst, cost = offsets(lists)
    if off is not None:
        o = np.asarray(off, np.uint64)
    arcs = np.zeros(max(dst.shape[0], 1), native.TASK_ARC_DT)
    arcs["dst"][:dst.shape[0]], arcs["cost"][:dst.shape[0]] = dst, cost
    a = None if ids is None else np.asarray(list(ids) or [0], np.uint64)
    st = native.KsUpdateStats()
    rc = L.ks_update_tasks(h, flags, t.ctypes.data, t.shape[0], o.ctypes.data, arcs.ctypes.data,
                           None if a is None else a.ctypes.data, 0 if ids is None else len(ids), sink_cost, st)
    return rc, L.ks_last_error(h).decode(), st.as_dict()


@AFTER_A_COMMIT
def test_an_aggregator_drained_by_a_pinned_commit_gets_its_arc_back(state):
    """Job 0's only task is placed: the pin takes the job's arc into the sink to 0. Evicted and
    listed with the ids, the task re-creates it with the sink cost; under NULL the drained
    aggregator is invisible and the call is refused."""
    spec = Jobs(2, 70, 2, 2, [(0, 5, 0, False), (1, None, 2, False), (1, 7, 0, False)])
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        (t,) = evict(ctx, spec, [0], False)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        assert (spec.U0, 1) not in before.table
        lst = [(spec.U0, 100), (spec.X, 50)]
        rc, msg, st = raw_call(ctx, [t], [lst], None, sink_cost=-3)
        assert rc == native.KS_E_INVALID and f"task {t}" in msg and "unsched_ids" in msg and not any(st.values())
        assert Snapshot(ctx).table == before.table and ctx.store_stats() == s0
        ref, stats, after, _ = update_and_check(ctx, [t], [lst], aggregators(spec), sink_cost=-3)
        assert after.table[(spec.U0, 1)] == (0, 1, -3, 0)
        assert (stats["unsched_updates"], stats["unsched_added"]) == (0, 1)


@AFTER_A_COMMIT
def test_tasks_evicted_after_a_preemptive_commit_are_refreshed(state):
    """They kept their arcs: the aggregator arc returns from the preemption cost to the
    unscheduled cost, no unit moves, and the next solve places them again."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        tasks = evict(ctx, spec, [1, 5], True)
        snap = Snapshot(ctx)
        caps = {j: snap.table[(spec.U0 + j, 1)] for j in range(3)}
        lists = [[(d, 100 if d >= spec.U0 else c) for d, c in held(snap, t)] for t in tasks]
        ref, stats, after, r = update_and_check(ctx, tasks, lists, aggregators(spec))
        assert stats["cost_updates"] == stats["records"] == 2 and stats["arcs_unchanged"] == 2
        assert {j: after.table[(spec.U0 + j, 1)] for j in range(3)} == caps
        mapping = ctx.task_mapping()
        assert all(mapping[t] for t in tasks)


@AFTER_A_COMMIT
def test_running_arcs_and_equal_lists_generate_nothing(state):
    """After a preemptive commit and a solve: one running task lists its running arc with another
    cost, one leaves it out, a waiting task lists what it holds. No record: the running arcs
    keep their cost and the solution and the mapping stay valid."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        ctx.solve()
        mapping = ctx.task_mapping()
        snap = Snapshot(ctx)
        a, b, w = spec.task(1), spec.task(3), spec.task(2)
        lists = [held(snap, a) + [(spec.bindings[a], 999)], held(snap, b), held(snap, w)]
        for keep in (False, True):
            ref, stats, after, _ = update_and_check(ctx, [a, b, w], lists, aggregators(spec), keep=keep)
            assert stats["records"] == 0 and stats["running_kept"] == 1 and stats["arcs_unchanged"] == 9
            assert after.table[(a, spec.bindings[a])] == after.table[(b, spec.bindings[b])] == (0, 1, 0, 1)
            assert ctx.task_mapping() == mapping                    # the mapping is still served
        stats = ctx.update_tasks([], [0], [], [], unsched_ids=None, unsched_sink_cost=5)
        assert not any(stats.values()) and ctx.task_mapping() == mapping


@AFTER_A_COMMIT
def test_an_aged_aggregator_cost_survives(state):
    """ks_update_unsched_costs(KS_COST_ADD) raised the waiting tasks' aggregator arcs on the
    device; a refresh that does not list them leaves the aged cost alone."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        assert ctx.update_unsched_costs(7, mode=native.KS_COST_ADD, unsched_ids=aggregators(spec)) > 0
        snap = Snapshot(ctx)
        tasks = [spec.task(0), spec.task(2)]
        assert all(snap.table[(t, spec.U0 + i % 3)][2] == 107 for t, i in zip(tasks, (0, 2)))
        lists = [[(spec.M0, 9)], [(spec.M0 + 1, 500), (spec.M0 + 7, 4)]]
        ref, stats, after, _ = update_and_check(ctx, tasks, lists, aggregators(spec), met_csr=state == "warm")
        assert all(after.table[(t, spec.U0 + i % 3)] == (0, 1, 107, 0) for t, i in zip(tasks, (0, 2)))
        assert (stats["cost_updates"], stats["arcs_removed"], stats["arcs_added"]) == (1, 2, 1)


def test_additions_overflow_a_machines_segment_then_land_in_place():
    spec = Jobs(2, 70, 2, 3, [(i % 3, None, 1, False) for i in range(210)])
    with native.Context(0, **STATES["warm"]) as ctx:
        prepare(ctx, spec, "warm", True)
        tasks = [spec.task(i) for i in range(200)]
        lists = [[(spec.M0 + 9, 500)]] * 200
        ref, stats, after, r = update_and_check(ctx, tasks, lists, aggregators(spec), keep=True, met_csr=True)
        assert stats["arcs_added"] == stats["records"] == 200
        assert r.raw["rebuilt"] == 1                                # a full segment: the CSR is rebuilt from the table
        more = [spec.task(200 + i) for i in range(10)]
        ref, stats, after, r = update_and_check(ctx, more, lists[:10], aggregators(spec), keep=True, met_csr=True)
        assert r.raw["rebuilt"] == 0 and stats["records"] == 10


# -------------------------------------------------------------------- refusals ---
@pytest.mark.parametrize("solved", [False, True], ids=["fresh", "solved"])
def test_refusals_change_nothing(solved):
    spec = cluster()
    U, X, M, INVALID, RANGE = spec.U0, spec.X, spec.M0, native.KS_E_INVALID, native.KS_E_RANGE
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(spec.bindings)
        dead = spec.task(0)
        ctx.complete_tasks([dead], resource_caps=False)             # a dead id, and job 0 …
        ctx.complete_tasks([spec.task(i) for i in (3, 6)], resource_caps=False)
        assert (U, 1) not in Snapshot(ctx).table                    # … drained: the NULL rule cannot see it
        if solved:
            ctx.solve()
            d0 = ctx.scheduling_deltas(commit=False)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        tasks0 = live_tasks(before)
        b0 = ctx.bindings(tasks0).tolist()
        n = int(before.nodes["id"].max())
        aggs = aggregators(spec)
        w, w2, run = spec.task(2), spec.task(4), spec.task(1)       # two waiting tasks (jobs 2 and 1), a running one (job 1)

        def refused(code, names, tasks, lists, ids=aggs, **kw):
            rc, msg, st = raw_call(ctx, tasks, lists, ids, **kw)
            assert rc == code, (rc, msg)
            for x in names:
                assert str(x) in msg, msg
            assert not any(st.values())
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive and (now.nodes == before.nodes).all()
            assert ctx.store_stats() == s0
            assert ctx.bindings(tasks0).tolist() == b0
            if solved:                                               # the valid solution stands
                assert (ctx.scheduling_deltas(commit=False) == d0).all()

        one = [(X, 1)]
        for flags in (0, native.KS_UPDATE_KEEP_UNLISTED):
            for bad in (dead, U + 1, n + 500, 10 ** 7, 0):                          # dead, no task, beyond the graph, 0
                refused(INVALID, [f"task {bad} "], [w, bad, 0], [one, one, one], flags=flags)
            refused(INVALID, [f"task {w} "], [w, w2, w, 0], [one, one, one, one], flags=flags)        # listed a second time
            for head in (dead, run, n + 500, 10 ** 7, 0):                           # dead, a task, beyond the graph, 0
                refused(INVALID, [f"task {w2}", f"head {head} "], [w, w2, run],     # the head before the cost
                        [one, [(X, 1), (head, (1 << 40) + 1)], [(0, 1)]], flags=flags)
            refused(INVALID, [f"task {w2}", f"head {M} ", "twice"], [w, w2], [one, [(M, 1), (X, 1), (M, 2)]], flags=flags)
            refused(INVALID, [f"task {w2}", f"head {M + 50} ", "twice"], [w, w2], [one, [(M + 50, 1), (X, 1), (M + 50, 2)]],
                    flags=flags)                                                    # a head the store does not hold
            refused(RANGE, [f"task {w2}"], [w, w2], [one, [(X, (1 << 40) + 1)]], flags=flags)
            refused(RANGE, [f"task {w}"], [w], [[(X, -(1 << 40) - 1)]], flags=flags)
            refused(INVALID, [f"task {w2}", "two"], [w, w2], [one, [(U + 2, 1), (M + 60, 3)]], ids=aggs + [M + 60],
                    flags=flags)                                                    # two aggregators, both listed
            refused(INVALID, [f"task {w2}", "two"], [w, w2], [one, [(U + 2, 1)]], flags=flags)        # one held, one listed
        refused(RANGE, ["sink cost"], [w], [one], sink_cost=(1 << 40) + 1)
        refused(RANGE, ["sink cost"], [w], [one], sink_cost=-(1 << 40) - 1)
        refused(INVALID, ["arc_off"], [w, w2], [one, one], off=[0, 2, 1])            # decreasing offsets
        refused(INVALID, ["arc_off[0]"], [w, w2], [one, one], off=[1, 1, 2])
        refused(INVALID, ["flag"], [w], [one], flags=2)
        refused(INVALID, ["flag"], [w], [one], flags=native.KS_UPDATE_KEEP_UNLISTED | 4)
        refused(INVALID, ["aggregator"], [w], [one], ids=aggs + [dead])              # an aggregator id that is dead
        # 2^40 itself is accepted, on an arc and on the sink
        rc, msg, st = raw_call(ctx, [w], [[(X, 1 << 40), (M, -(1 << 40))]], aggs, sink_cost=-(1 << 40),
                               flags=native.KS_UPDATE_KEEP_UNLISTED)
        assert rc == native.KS_OK, msg
        assert (st["arcs_added"], st["cost_updates"], st["records"]) == (1, 1, 2)
        assert Snapshot(ctx).table[(w, X)] == (0, 1, 1 << 40, 0)


def test_the_null_rule_and_bound_tasks():
    """Job 0 is drained by a pinned commit (its arc into the sink is gone). Under NULL its
    evicted, unbound task is refused when it lists no recognised aggregator; its bound sibling
    passes without an aggregator arc."""
    spec = Jobs(2, 70, 2, 2, [(0, 5, 0, False), (0, 6, 0, False), (1, None, 2, False)])
    with native.Context(0) as ctx:
        prepare(ctx, spec, "engine", False)
        (t,) = evict(ctx, spec, [0], False)
        sib = spec.task(1)
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        for lst in ([(spec.X, 50)], [(spec.U0, 100), (spec.X, 50)], []):
            rc, msg, st = raw_call(ctx, [sib, t], [[(spec.M0 + 6, 1)], lst], None)
            assert rc == native.KS_E_INVALID and f"task {t} " in msg and "unsched_ids" in msg, msg
            assert Snapshot(ctx).table == before.table and ctx.store_stats() == s0
        ref, stats, after, _ = update_and_check(ctx, [sib], [[(spec.M0 + 6, 1)]], None, solve=False)   # bound: passes
        assert stats["arcs_added"] == stats["records"] == 1
        ref, stats, after, _ = update_and_check(ctx, [t], [[(spec.U0, 100), (spec.X, 50)]], aggregators(spec))
        assert after.table[(spec.U0, 1)] == (0, 1, 0, 0)


def test_two_sinks_refuse_a_gaining_aggregator():
    spec = cluster()
    n0 = len(spec.ntype)
    two = Spec(list(spec.ntype) + [3], list(spec.supply) + [0], spec.arcs, spec.bindings)
    with native.Context(0, auto_sink=0) as ctx:
        ctx.load_graph(two.graph(running=True))
        t = spec.task(0)
        rec = np.zeros(1, native.DELTA_DT)                          # the task loses its aggregator arc
        rec[0]["kind"], rec[0]["src"], rec[0]["dst"] = native.KS_UPDATE_ARC, t, spec.U0
        ctx.apply_deltas(rec)
        before = Snapshot(ctx)
        assert n0 + 1 in before.alive and (t, spec.U0) not in before.table
        # a refresh to what the task holds: no record, and the walk builds the residual CSR the load left pending
        off, dst, cost = offsets([held(before, t)])
        r0 = ctx.store_stats()["rebuilds"]
        assert ctx.update_tasks([t], off, dst, cost, unsched_ids=aggregators(spec))["records"] == 0
        assert ctx.store_stats()["rebuilds"] == r0 + 1
        s0 = ctx.store_stats()
        for flags in (native.KS_UPDATE_KEEP_UNLISTED, 0):
            rc, msg, _ = raw_call(ctx, [t], [[(spec.U0, 100)]], aggregators(spec), flags=flags)
            assert rc == native.KS_E_INVALID and "one sink" in msg
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive and ctx.store_stats() == s0
        rc, msg, st = raw_call(ctx, [t], [[(spec.X, 50)]], aggregators(spec), flags=native.KS_UPDATE_KEEP_UNLISTED)
        assert rc == native.KS_OK and st["records"] == 1 and (t, spec.X) in Snapshot(ctx).table   # no unit moves: legal
