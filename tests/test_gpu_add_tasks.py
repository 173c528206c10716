"""GPU: ks_add_tasks — arriving tasks enter the device-resident graph with their arcs and
their aggregators gain a unit each — against the rule restated on the host
(tests/arrive_ref.py), against the store's reference (tests/store_ref.py) and against the
host path it replaces (the same records through ks_apply_deltas on a twin context). The
harness is that of test_gpu_complete_tasks.py: every case runs before any solve, after a
solve with a commit on the cell path and on the engine path, and with warm_start = 1."""
import numpy as np
import pytest

from arrive_ref import arrive_reference, offsets
from ksched_amd import churn, native
from oracle import ko
from store_ref import check_counters, same_store
from test_gpu_complete_tasks import Jobs, balanced, live_tasks
from test_gpu_remove_resources import EVERY_STATE, STATES, Snapshot, Spec, prepare

pytestmark = pytest.mark.gpu

AFTER_A_COMMIT = pytest.mark.parametrize("state", ["cell", "engine", "warm"])


# ---------------------------------------------------------------------- graphs ---
def cluster(J=3, waiting_only=()) -> Jobs:
    """140 machines of 2 slots, J jobs, 8 tasks: the odd ones designated to machine i, the
    even ones waiting. waiting_only: jobs whose tasks all wait."""
    tasks = [(i % J, i if i % 2 and i % J not in waiting_only else None, 2, False) for i in range(8)]
    return Jobs(2, 70, 2, J, tasks)


def arrival(spec, job, length, first_machine=0) -> list:
    """A task's arcs: its aggregator (100), then length − 1 machines (500 + k: never taken)."""
    if length == 0:
        return []
    return [(spec.U0 + job, 100)] + [(spec.M0 + first_machine + k, 500 + k) for k in range(length - 1)]


def aggregators(spec) -> list:
    return list(range(spec.U0, spec.T0))


def top(ctx) -> int:
    return int(Snapshot(ctx).nodes["id"].max())


# --------------------------------------------------------------------- harness ---
def add_and_check(ctx, tasks, lists, bindings, unsched_ids, sink_cost=0, met_csr=False, arcless=()):
    """One call against the rule, the store's reference and the host path, then the solve after
    it against the oracle; → (the rule's result, the device's stats, the graph after, the solve)."""
    before = Snapshot(ctx)
    ref = arrive_reference(before.graph(), tasks, lists, unsched_ids, sink_cost, alive=before.alive)
    sref = before.store()
    want = sref.apply(ref.stream)
    assert want["superseded"] == ref.superseded
    with native.Context(0) as twin:                               # the host path: the same records
        twin.load_arrays(before.nodes, before.arcs)
        twin.apply_deltas(ref.stream)
        same_store(twin, sref)
        twin_rows = Snapshot(twin).table
    old = live_tasks(before)
    builds = ctx.store_stats()["rebuilds"]
    off, dst, cost = offsets(lists)
    stats = ctx.add_tasks(tasks, off, dst, cost, unsched_ids=unsched_ids, unsched_sink_cost=sink_cost)
    assert stats == ref.stats
    assert stats["records"] == stats["tasks"] + stats["arcs_added"] + stats["unsched_updates"] + stats["unsched_added"]
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == ref.alive == before.alive | set(tasks)
    counters = ctx.store_stats()                                  # (before the solve: its auto-sink edit is a stream)
    rest = live_tasks(after)
    assert set(rest) == set(old) | set(tasks)
    assert dict(zip(rest, ctx.bindings(rest).tolist())) == {t: 0 if t in tasks else bindings.get(t, 0) for t in rest}
    if arcless:                                                   # a task without arcs cannot be routed: it leaves again
        ctx.complete_tasks(list(arcless), resource_caps=False, unsched_ids=[])
    r = resolve_and_check(ctx)
    # exact: the stream met a valid CSR and fit its slack (no build since, by the solve or the completion above)
    check_counters(counters, want, exact=met_csr and ctx.store_stats()["rebuilds"] == builds)
    return ref, stats, after, r


def resolve_and_check(ctx):
    """The solve after the call: cost and flow against the oracle, the flows through its verifier."""
    r = ctx.solve()
    g = balanced(Snapshot(ctx))
    st, cost, flow, _ = ko.cost_scaling(g)
    assert st == 0 and (r.cost, r.flow) == (cost, flow)
    f = ctx.flows()
    got = dict(zip(zip(f["src"].tolist(), f["dst"].tolist()), f["flow"].tolist()))
    vec = np.asarray([got.pop((int(s), int(d)), 0) for s, d in zip(g.src, g.dst)], np.int64)
    assert not got
    vst, vcost, _ = ko.verify(g, vec)
    assert (vst, vcost) == (0, cost)
    return r


# ----------------------------------------------------------------------- cases ---
@EVERY_STATE
def test_arc_list_lengths(state):
    """0, 1, 63, 64, 65 and 130 arcs mixed in one call: the arc → task bisection over offsets
    that repeat (the empty list) and that cross a wave and a workgroup."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        lengths = [65, 0, 1, 130, 63, 0, 64, 2]
        tasks = [n + 1 + i for i in range(len(lengths))]
        lists = [arrival(spec, i % 3, L, first_machine=i) for i, L in enumerate(lengths)]
        ref, stats, after, _ = add_and_check(ctx, tasks, lists, bindings, aggregators(spec), met_csr=state == "warm",
                                             arcless=[t for t, L in zip(tasks, lengths) if L == 0])
        assert stats["arcs_added"] == sum(lengths) and stats["unsched_updates"] == 3 and stats["unsched_added"] == 0
        assert after.table[(tasks[3], spec.M0 + 3 + 128)] == (0, 1, 628, 0)


@EVERY_STATE
@pytest.mark.parametrize("k", [1, 64, 65])
def test_one_job_fills_a_wave(state, k):
    """k tasks of one job with one arc each: their aggregator arcs fill one wave exactly (64)
    and spill one lane into the next (65). The aggregator gains exactly k."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        cap0 = Snapshot(ctx).table[(spec.U0 + 1, 1)][1]
        tasks = [n + 1 + i for i in range(k)]
        ref, stats, after, _ = add_and_check(ctx, tasks, [arrival(spec, 1, 1)] * k, bindings, aggregators(spec),
                                             met_csr=state == "warm")
        assert after.table[(spec.U0 + 1, 1)] == (0, cap0 + k, 0, 0)
        assert (stats["tasks"], stats["unsched_updates"], stats["records"]) == (k, 1, 2 * k + 1)


@EVERY_STATE
def test_three_aggregators_interleaved_in_one_wave(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        caps = [Snapshot(ctx).table[(spec.U0 + j, 1)][1] for j in range(3)]
        jobs = [(i * 7) % 3 if i % 5 else 2 for i in range(61)]
        tasks = [n + 1 + i for i in range(61)]
        ref, stats, after, _ = add_and_check(ctx, tasks, [arrival(spec, j, 1) for j in jobs], bindings,
                                             aggregators(spec), met_csr=state == "warm")
        assert [after.table[(spec.U0 + j, 1)][1] - caps[j] for j in range(3)] == [jobs.count(j) for j in range(3)]
        assert stats["unsched_updates"] == 3 and min(jobs.count(j) for j in range(3)) > 5


def priced() -> Jobs:
    """Job 1's arc into the sink carries a lower bound of 1 and a cost of 40."""
    spec = cluster(waiting_only=(1,))
    spec.arcs = [((s, d), (1, a[1], 40, 0) if (s, d) == (spec.U0 + 1, 1) else a) for (s, d), a in spec.arcs]
    return spec


@EVERY_STATE
@pytest.mark.parametrize("null_rule", [False, True], ids=["ids", "null"])
def test_a_present_aggregator_arc_keeps_its_bound_and_cost(state, null_rule):
    spec = priced()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        lo, cap0, co, ty = Snapshot(ctx).table[(spec.U0 + 1, 1)]
        assert (lo, co) == (1, 40)
        tasks = [n + 1, n + 2, n + 3]
        lists = [arrival(spec, 1, 3), arrival(spec, 0, 2), arrival(spec, 1, 1)]
        ref, stats, after, _ = add_and_check(ctx, tasks, lists, bindings, None if null_rule else aggregators(spec),
                                             sink_cost=77, met_csr=state == "warm")
        assert after.table[(spec.U0 + 1, 1)] == (1, cap0 + 2, 40, 0)     # one UPDATE_ARC: low and cost kept
        assert stats["unsched_updates"] == 2 and stats["unsched_added"] == 0


@EVERY_STATE
def test_an_aggregator_drained_by_completions_gets_its_arc_back(state):
    """Every task of job 1 completes: ks_complete_tasks takes its arc into the sink to 0 and the
    store drops it. Arrivals of job 1 re-create it with the sink cost."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        mine = [spec.task(i) for i in range(8) if i % 3 == 1]
        ctx.complete_tasks(mine, resource_caps=False, unsched_ids=aggregators(spec))
        assert (spec.U0 + 1, 1) not in Snapshot(ctx).table
        bindings = {t: p for t, p in bindings.items() if t not in mine}
        n = top(ctx)
        tasks = [n + 1, n + 2, n + 3]
        lists = [arrival(spec, 1, 2), arrival(spec, 2, 2), arrival(spec, 1, 4)]
        ref, stats, after, _ = add_and_check(ctx, tasks, lists, bindings, aggregators(spec), sink_cost=7)
        assert after.table[(spec.U0 + 1, 1)] == (0, 2, 7, 0)
        assert (stats["unsched_updates"], stats["unsched_added"]) == (1, 1)


@AFTER_A_COMMIT
def test_an_aggregator_drained_by_a_pinned_commit_gets_its_arc_back(state):
    """Job 0's only task is placed: the pinned commit takes the job's arc into the sink to 0."""
    spec = Jobs(2, 70, 2, 2, [(0, 5, 0, False), (1, None, 2, False), (1, 7, 0, False)])
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, False)
        assert (spec.U0, 1) not in Snapshot(ctx).table and (spec.U0 + 1, 1) in Snapshot(ctx).table
        n = top(ctx)
        lists = [arrival(spec, 0, 2, first_machine=20), arrival(spec, 0, 1), arrival(spec, 1, 1)]
        ref, stats, after, _ = add_and_check(ctx, [n + 1, n + 2, n + 3], lists, bindings, aggregators(spec), sink_cost=-3)
        assert after.table[(spec.U0, 1)] == (0, 2, -3, 0) and after.table[(spec.U0 + 1, 1)] == (0, 2, 0, 0)
        assert (stats["unsched_updates"], stats["unsched_added"]) == (1, 1)


@EVERY_STATE
def test_a_new_jobs_aggregator_has_no_arc_yet(state):
    """An aggregator node added by ks_apply_deltas, with no arc into the sink."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        u = top(ctx) + 1
        rec = np.zeros(1, native.DELTA_DT)
        rec[0]["kind"], rec[0]["id"], rec[0]["type"] = native.KS_ADD_NODE, u, 0
        ctx.apply_deltas(rec)
        lists = [[(u, 100), (spec.X, 50)], [(u, 90)], arrival(spec, 2, 2)]
        ref, stats, after, _ = add_and_check(ctx, [u + 1, u + 2, u + 3], lists, bindings, aggregators(spec) + [u], sink_cost=11)
        assert after.table[(u, 1)] == (0, 2, 11, 0)
        assert (stats["unsched_updates"], stats["unsched_added"]) == (1, 1)


@EVERY_STATE
def test_the_id_of_a_bound_task_is_reused(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        t = next(x for x in sorted(bindings) if bindings[x])
        left, _ = ctx.complete_tasks([t], resource_caps=False, unsched_ids=aggregators(spec))
        assert left.tolist() == [bindings[t]]
        old = {k for k in Snapshot(ctx).table if t in k}
        assert not old
        rest = {x: p for x, p in bindings.items() if x != t}
        ref, stats, after, _ = add_and_check(ctx, [t], [arrival(spec, 2, 3, first_machine=30)], rest, aggregators(spec),
                                             met_csr=True)
        assert {k for k in after.table if t in k} == {(t, spec.U0 + 2), (t, spec.M0 + 30), (t, spec.M0 + 31)}
        assert ctx.bindings([t]).tolist() == [0]


@EVERY_STATE
def test_fresh_ids_with_dead_slots_between_and_beyond_the_node_store(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        ref, stats, after, _ = add_and_check(ctx, [n + 70, n + 1], [arrival(spec, 0, 2), arrival(spec, 1, 66)], bindings,
                                             aggregators(spec))
        assert {n + 1, n + 70} <= after.alive and not (set(range(n + 2, n + 70)) & after.alive)
        r0 = ctx.store_stats()["rebuilds"]
        far = 5000                                                  # the node store holds 1,024 slots here
        assert far > 1024 + n
        ref, stats, after, r = add_and_check(ctx, [far], [arrival(spec, 2, 3)], bindings, aggregators(spec), met_csr=True)
        assert r.raw["rebuilt"] == 1 and ctx.store_stats()["rebuilds"] == r0 + 1
        assert far in after.alive and after.table[(far, spec.U0 + 2)] == (0, 1, 100, 0)


def test_two_hundred_arrivals_overflow_a_machines_segment_then_land_in_place():
    spec = cluster()
    with native.Context(0, **STATES["warm"]) as ctx:
        _, bindings = prepare(ctx, spec, "warm", True)
        n = top(ctx)
        tasks = [n + 1 + i for i in range(200)]
        lists = [[(spec.U0 + i % 3, 100), (spec.M0 + 9, 500)] for i in range(200)]
        ref, stats, after, r = add_and_check(ctx, tasks, lists, bindings, aggregators(spec), met_csr=True)
        assert r.raw["rebuilt"] == 1                                # a full segment: the CSR is rebuilt from the table
        more = [n + 201 + i for i in range(10)]
        ref, stats, after, r = add_and_check(ctx, more, lists[:10], bindings, aggregators(spec), met_csr=True)
        assert r.raw["rebuilt"] == 0
        assert ctx.store_stats()["rebuilds"] >= 2 and stats["records"] == 33


@EVERY_STATE
def test_a_repeated_machine_head_is_an_upsert(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        _, bindings = prepare(ctx, spec, state, True)
        n = top(ctx)
        lists = [[(spec.M0 + 4, 9), (spec.U0, 100), (spec.M0 + 4, 6)]]
        ref, stats, after, _ = add_and_check(ctx, [n + 1], lists, bindings, aggregators(spec), met_csr=state == "warm")
        assert ref.superseded == 1 and after.table[(n + 1, spec.M0 + 4)] == (0, 1, 6, 0)
        assert stats["arcs_added"] == 3 and stats["records"] == 5


# -------------------------------------------------------------------- refusals ---
def raw_call(ctx, tasks, lists, ids, sink_cost=0, flags=0, off=None):
    L, h = ctx._L, ctx._h
    t = np.asarray(tasks, np.uint64)
    o, dst, cost = offsets(lists)
    if off is not None:
        o = np.asarray(off, np.uint64)
    arcs = np.zeros(max(dst.shape[0], 1), native.TASK_ARC_DT)
    arcs["dst"][:dst.shape[0]], arcs["cost"][:dst.shape[0]] = dst, cost
    a = None if ids is None else np.asarray(list(ids) or [0], np.uint64)
    st = native.KsAddStats()
    rc = L.ks_add_tasks(h, flags, t.ctypes.data, t.shape[0], o.ctypes.data, arcs.ctypes.data,
                        None if a is None else a.ctypes.data, 0 if ids is None else len(ids), sink_cost, st)
    return rc, L.ks_last_error(h).decode(), st.as_dict()


@pytest.mark.parametrize("solved", [False, True], ids=["fresh", "solved"])
def test_refusals_change_nothing(solved):
    spec = cluster()
    U, X, INVALID, RANGE = spec.U0, spec.X, native.KS_E_INVALID, native.KS_E_RANGE
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
        n = top(ctx)
        aggs = aggregators(spec)

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

        one = [(U + 1, 100)]
        live = spec.task(1)
        refused(INVALID, [live], [n + 1, live, 0], [one, one, one])                 # a live id
        refused(INVALID, [U + 1], [n + 1, U + 1], [one, one])                       # a live node that is no task
        refused(INVALID, [n + 2], [n + 2, n + 1, n + 2], [one, one, one])           # an id listed twice
        refused(RANGE, ["node id 0 "], [n + 1, 0], [one, one])                      # id 0
        refused(RANGE, [1 << 30], [n + 1, 1 << 30], [one, one])                     # id 2^30
        for head in (dead, live, n + 500, 10 ** 7, n + 1, 0):                       # dead, a task, beyond the graph (in and
            refused(INVALID, [f"task {n + 2}", f"head {head} "],                    # past the node store), of this call, 0
                    [n + 1, n + 2, n + 3], [one, [(X, 1), (head, 5)], [(0, 1)]])
        refused(INVALID, [f"task {n + 2}"], [n + 1, n + 2], [one, [(U + 1, 1), (X, 2), (U + 1, 3)]])   # one aggregator twice
        refused(INVALID, [f"task {n + 2}"], [n + 1, n + 2], [one, [(U + 1, 1), (U + 2, 3)]])           # two aggregators
        refused(INVALID, [f"task {n + 2}", "unsched_ids"], [n + 1, n + 2], [one, [(U, 1), (X, 2)]], ids=None)   # drained, NULL
        refused(INVALID, [f"task {n + 1}", "unsched_ids"], [n + 1], [[]], ids=None)                    # no arc at all, NULL
        refused(RANGE, [f"task {n + 2}"], [n + 1, n + 2], [one, [(X, (1 << 40) + 1)]])
        refused(RANGE, [f"task {n + 1}"], [n + 1], [[(X, -(1 << 40) - 1)]])
        refused(RANGE, ["sink cost"], [n + 1], [one], sink_cost=(1 << 40) + 1)
        refused(RANGE, ["sink cost"], [n + 1], [one], sink_cost=-(1 << 40) - 1)
        refused(INVALID, ["arc_off"], [n + 1, n + 2], [one, one], off=[0, 2, 1])    # decreasing offsets
        refused(INVALID, ["arc_off[0]"], [n + 1, n + 2], [one, one], off=[1, 1, 2])
        refused(INVALID, ["flag"], [n + 1], [one], flags=1)
        refused(INVALID, ["aggregator"], [n + 1], [one], ids=aggs + [dead])          # an aggregator id that is dead
        # 2^40 itself is accepted, on an arc and on the sink
        rc, msg, st = raw_call(ctx, [n + 1], [[(U, 1 << 40), (X, -(1 << 40))]], aggs, sink_cost=-(1 << 40))
        assert rc == native.KS_OK, msg
        assert st == dict(tasks=1, arcs_added=2, unsched_updates=0, unsched_added=1, records=4)
        assert Snapshot(ctx).table[(U, 1)] == (0, 1, -(1 << 40), 0)


def test_two_sinks_refuse_a_gaining_aggregator():
    spec = cluster()
    n0 = len(spec.ntype)
    two = Spec(list(spec.ntype) + [3], list(spec.supply) + [0], spec.arcs, spec.bindings)
    with native.Context(0, auto_sink=0) as ctx:
        ctx.load_graph(two.graph(running=True))
        before = Snapshot(ctx)
        s0 = ctx.store_stats()
        rc, msg, _ = raw_call(ctx, [n0 + 2], [[(spec.U0, 100)]], aggregators(spec))
        assert rc == native.KS_E_INVALID and "one sink" in msg
        now = Snapshot(ctx)
        assert now.table == before.table and now.alive == before.alive and ctx.store_stats() == s0
        rc, msg, st = raw_call(ctx, [n0 + 2], [[(spec.X, 50)]], aggregators(spec))       # no unit moves: legal
        assert rc == native.KS_OK and st["records"] == 2 and (n0 + 2, spec.X) in Snapshot(ctx).table


@EVERY_STATE
def test_no_task_keeps_the_solution(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        ctx.solve()
        mapping = ctx.task_mapping()
        s0 = ctx.store_stats()
        table = Snapshot(ctx).table
        for ids in (None, aggregators(spec)):
            stats = ctx.add_tasks([], [0], [], [], unsched_ids=ids, unsched_sink_cost=5)
            assert not any(stats.values())
            assert ctx.task_mapping() == mapping                    # the mapping is still served
            assert ctx.store_stats() == s0 and Snapshot(ctx).table == table


# ------------------------------------------------------- a round without records ---
def test_a_round_without_arrival_records():
    """Four churn rounds of a small preemptive cell on twin contexts. A applies the model's
    own stream through ks_apply_deltas; B commits its solve, completes the stream's removed
    ids and adds the arrivals on the device: no arrival record crosses to B. After every
    round the two graphs are the same (src, dst) → row tables and both solves the oracle's."""
    cell = churn.Cell(36, 10, 2, 9, 3, preemption=True, preemption_cost=150)
    aggs = [cell.U0 + j for j in range(cell.J)]
    recreated = 0
    with native.Context(0) as a, native.Context(0) as b:
        g = cell.graph()
        a.load_graph(g)
        b.load_graph(g)
        for rnd in range(4):
            g = cell.graph()
            st, cost, flow, _ = ko.cost_scaling(g)
            ra, rb = a.solve(), b.solve()
            assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow), rnd
            # the model follows B's mapping (two optima may differ in who runs where)
            host = cell.step(b.task_mapping(), 12, 14, age_cost=0)
            a.apply_deltas(host)
            b.commit_preemptive(continuation=0, preemption=150, resource_caps=False, unsched_ids=aggs)
            done = host["id"][host["kind"] == churn.KS_REMOVE_NODE].astype(np.int64).tolist()
            b.complete_tasks(done, resource_caps=False, unsched_ids=aggs)
            ids = list(cell.last_arrived_ids)
            sl = np.asarray(ids) - cell.TASK0
            off = np.arange(len(ids) + 1) * 5
            stats = b.add_tasks(ids, off, cell.adst[sl].reshape(-1), cell.acost[sl].reshape(-1), unsched_ids=aggs)
            assert stats["tasks"] == 14 and stats["arcs_added"] == 70
            recreated += stats["unsched_added"]
            sa, sb = Snapshot(a), Snapshot(b)
            assert sa.table == sb.table and sa.alive == sb.alive, rnd
            assert (sa.nodes == sb.nodes).all()
        assert recreated > 0                                         # a job drained to zero and received arrivals
        g = cell.graph()
        st, cost, flow, _ = ko.cost_scaling(g)
        ra, rb = a.solve(), b.solve()
        assert st == 0 and (ra.cost, ra.flow) == (rb.cost, rb.flow) == (cost, flow)
