"""GPU: ks_update_nodes — class and resource arcs are added, re-costed, re-sized and dropped as
their tails' lists say — against the rule restated on the host (tests/nodes_ref.py), against the
store's reference (tests/store_ref.py) and against the host path it replaces (the same records
through ks_apply_deltas on a twin context). The harness is that of test_gpu_update_tasks.py: every
case runs before any solve, after a solve with a commit on the cell path and on the engine path,
and with warm_start = 1. The shapes follow the kernels' constants: 64 lanes, 64-position chunks,
256-thread workgroups."""
import importlib.util
import os
import re

import numpy as np
import pytest

from complete_ref import complete_reference
from ksched_amd import native
from nodes_ref import CAP_KEEP, KEEP_UNLISTED, nodes_reference, offsets3
from oracle import ko
from preempt_ref import preempt_reference, table_graph
from remove_ref import BelowLowerBound
from store_ref import check_counters, same_store
from test_gpu_add_tasks import aggregators, cluster, priced, resolve_and_check
from test_gpu_complete_tasks import Jobs, live_tasks
from test_gpu_remove_resources import EVERY_STATE, STATES, Snapshot, Spec, prepare, triples

pytestmark = pytest.mark.gpu

KEEP = pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


# --------------------------------------------------------------------- harness ---
def held(snap, u) -> list:
    """The tail's out-arcs as a list for the call: (head, cost, cap)."""
    return [(d, a[2], a[1]) for (s, d), a in snap.table.items() if s == u]


def bound(ctx) -> dict:
    tasks = live_tasks(Snapshot(ctx))
    return dict(zip(tasks, ctx.bindings(tasks).tolist()))


def nodes_and_check(ctx, nodes, lists, keep=False, met_csr=False, solve=True):
    """One call against the rule, the store's reference and the host path, then the solve after
    it against the oracle; → (the rule's result, the device's stats, the graph after, the solve)."""
    before = Snapshot(ctx)
    bindings = bound(ctx)
    ref = nodes_reference(before.ntype, before.table, nodes, lists, KEEP_UNLISTED if keep else 0, alive=before.alive)
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
    stats = ctx.update_nodes(nodes, *offsets3(lists), keep_unlisted=keep)
    assert stats == ref.stats
    assert stats["records"] == stats["arcs_added"] + stats["arcs_updated"] + stats["arcs_zeroed"] + stats["arcs_removed"]
    same_store(ctx, sref)
    after = Snapshot(ctx)
    assert after.table == ref.arcs == twin_rows
    assert after.alive == before.alive and (after.nodes == before.nodes).all()   # no node is added or removed
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


# ----------------------------------------------------------------------- cases ---
def wide_class() -> Jobs:
    """X holds 130 out-arcs (two racks and 128 machines, half of them ahead of everything else in
    the arc table and half behind it) and 70 running tasks point at it: its residual segment
    spans four 64-position chunks and mixes forward and reverse positions."""
    spec = Jobs(2, 70, 2, 2, [(i % 2, i, 0, False) for i in range(70)] + [(0, None, 2, False), (1, None, 2, False)])
    extra = [((spec.X, spec.M0 + k), (0, 2, 60 + k % 5, 0)) for k in range(128)]
    spec.arcs = extra[:64] + spec.arcs + extra[64:]
    return spec


@EVERY_STATE
@KEEP
def test_a_wide_class_three_arcs_stay_listed(state, keep):
    spec = wide_class()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        snap = Snapshot(ctx)
        assert len(held(snap, spec.X)) == 130 and sum(1 for (s, d) in snap.table if d == spec.X) == 70
        cap = snap.table[(spec.X, spec.M0 + 127)][1]
        lst = [(spec.R0, 0, CAP_KEEP), (spec.M0 + 40, 7, CAP_KEEP), (spec.M0 + 127, 62, cap + 1)]
        ref, stats, after, _ = nodes_and_check(ctx, [spec.X], [lst], keep=keep, met_csr=state == "warm")
        assert stats["arcs_removed"] == (0 if keep else 127)
        assert (stats["arcs_updated"], stats["arcs_unchanged"]) == (2, 1)
        assert len(held(after, spec.X)) == (130 if keep else 3)
        assert sum(1 for (s, d) in after.table if d == spec.X) == 70           # no reverse position was taken for an arc


@EVERY_STATE
def test_sixty_five_tails_of_mixed_types_in_one_call(state):
    """Classes (X and the racks), machines and PUs alternate inside one wave; the 65th tail opens
    the next. The machines' and PUs' unlisted arcs survive, the classes' do not."""
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        snap = Snapshot(ctx)
        tails, lists = [], []
        for k in range(31):
            m, p = spec.M0 + 2 * k, spec.P0 + 2 * k + 1
            tails += [m, p]
            lists += [[] if k % 2 else [(p - 1, 3 + k, CAP_KEEP)], [] if k % 3 else [(spec.SINK, 1, CAP_KEEP)]]
        racks = [held(snap, spec.R0 + r) for r in range(2)]
        tails = tails[:20] + [spec.R0] + tails[20:40] + [spec.X] + tails[40:] + [spec.R0 + 1]
        lists = (lists[:20] + [[(d, c + 1, cap) for d, c, cap in racks[0][:60]]] + lists[20:40] +
                 [[(spec.R0, 2, CAP_KEEP)]] + lists[40:] + [racks[1][5:]])
        assert len(tails) == 65
        ref, stats, after, _ = nodes_and_check(ctx, tails, lists, met_csr=state == "warm")
        assert stats["nodes"] == 65 and stats["arcs_removed"] == len(racks[0]) - 60 + 1 + 5
        assert stats["arcs_updated"] == 60 + 1 + 16 + 11 and stats["arcs_unchanged"] == len(racks[1]) - 5
        for k in range(31):                                         # every machine → PU and PU → sink arc is still there
            assert (spec.M0 + 2 * k, spec.P0 + 2 * k) in after.table and (spec.P0 + 2 * k + 1, spec.SINK) in after.table
        assert (spec.X, spec.R0 + 1) not in after.table


@EVERY_STATE
def test_one_list_hits_every_row_of_the_table(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        snap = Snapshot(ctx)
        R, M = spec.R0, spec.M0
        cap = {k: snap.table[(R, M + k)][1] for k in range(6)}
        assert all(snap.table[(R, M + k)][2] == 0 for k in range(6))
        lst = [(M + 70, 5, 2),                  # add: a machine of the other rack
               (M, 3, cap[0]),                  # cost only
               (M + 1, 0, cap[1] + 1),          # capacity only
               (M + 2, 4, cap[2] + 2),          # both
               (M + 3, 0, cap[3]),              # unchanged
               (M + 71, 5, 0),                  # skipped: absent and cap 0
               (M + 4, 9, 0),                   # zeroed
               (M + 5, 6, CAP_KEEP)]            # the capacity kept, the cost moves
        lst += [(d, c, CAP_KEEP) for d, c, _ in held(snap, R) if d >= M + 10]     # the rest stay; M + 6 … M + 9 are dropped
        ref, stats, after, _ = nodes_and_check(ctx, [R], [lst], met_csr=state == "warm")
        assert stats == dict(nodes=1, arcs_added=1, arcs_updated=4, arcs_unchanged=61, arcs_skipped=1, arcs_zeroed=1,
                             arcs_removed=4, records=10)
        assert after.table[(R, M + 70)] == (0, 2, 5, 0) and after.table[(R, M + 5)] == (0, cap[5], 6, 0)
        assert (R, M + 4) not in after.table and (R, M + 71) not in after.table


def interleaved() -> Jobs:
    """The two racks' arcs into their machines alternate in the arc table."""
    spec = cluster()
    rack = lambda r: [x for x in spec.arcs if x[0][0] == spec.R0 + r]
    a, b = rack(0), rack(1)
    rest = [x for x in spec.arcs if x[0][0] not in (spec.R0, spec.R0 + 1)]
    spec.arcs = rest[:10] + [x for pair in zip(a, b) for x in pair] + rest[10:]
    return spec


@EVERY_STATE
def test_two_classes_whose_records_interleave_in_arc_slot_order(state):
    spec = interleaved()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        snap = Snapshot(ctx)
        order = [k for k in snap.table if k[0] in (spec.R0, spec.R0 + 1)]
        assert [k[0] for k in order[:6]] == [spec.R0, spec.R0 + 1] * 3           # ks_get_graph lists arcs by slot
        lists = [[(d, c + 1 + d % 3, cap) for d, c, cap in held(snap, spec.R0 + r)[r::2]] + [(spec.M0 + 70 * (1 - r), 8, 1)]
                 for r in range(2)]
        ref, stats, after, _ = nodes_and_check(ctx, [spec.R0 + 1, spec.R0], lists[::-1], met_csr=state == "warm")
        srcs = ref.stream["src"][:stats["arcs_updated"] + stats["arcs_removed"]].tolist()
        assert srcs[:6] == [spec.R0, spec.R0 + 1] * 3                             # the stream alternates between the tails
        assert (stats["arcs_updated"], stats["arcs_removed"], stats["arcs_added"]) == (70, 70, 2)


@pytest.mark.parametrize("state", ["cell", "engine", "warm"])
def test_an_unlisted_arc_into_the_sink_stays(state):
    """After a pinned commit job 1's aggregator is drained (its arc into the sink is gone), jobs 0
    and 2 keep theirs. Every aggregator and two PUs listed with empty lists: no record. Then the
    aggregators again with X, whose list drops a rack."""
    spec = Jobs(2, 70, 2, 3, [(0, None, 2, False), (1, 1, 0, False), (2, None, 2, False), (1, 3, 0, False), (0, 5, 0, False)])
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        ctx.solve()                                                 # (a valid residual CSR: a call without a record builds none)
        snap = Snapshot(ctx)
        aggs = aggregators(spec)
        have = [u for u in aggs if (u, spec.SINK) in snap.table]
        assert have and len(have) < len(aggs)
        tails = aggs + [spec.P0 + 1, spec.P0 + 2]
        ref, stats, after, _ = nodes_and_check(ctx, tails, [[]] * len(tails))
        assert stats == dict(nodes=len(tails), arcs_added=0, arcs_updated=0, arcs_unchanged=0, arcs_skipped=0,
                             arcs_zeroed=0, arcs_removed=0, records=0)
        ref, stats, after, _ = nodes_and_check(ctx, tails + [spec.X], [[]] * len(tails) + [[(spec.R0, 1, CAP_KEEP)]])
        assert (stats["arcs_removed"], stats["arcs_updated"], stats["records"]) == (1, 1, 2)
        assert all((u, spec.SINK) in after.table for u in have) and (spec.P0 + 1, spec.SINK) in after.table


def test_a_capacity_lowered_below_the_flow_of_the_last_solve():
    """Two tasks run on machine 3's PU; after the warm solve its arc into the sink carries 2.
    The call takes that arc to 1: the warm re-solve moves one task away and equals the oracle."""
    spec = Jobs(2, 70, 2, 2, [(0, 3, 0, False), (1, 3, 0, False), (0, None, 2, False)])
    with native.Context(0, **STATES["warm"]) as ctx:
        prepare(ctx, spec, "warm", True)
        p = spec.P0 + 3
        f = ctx.flows()
        flow = dict(zip(zip(f["src"].tolist(), f["dst"].tolist()), f["flow"].tolist()))
        assert flow[(p, spec.SINK)] == 2
        ref, stats, after, r = nodes_and_check(ctx, [p], [[(spec.SINK, 0, 1)]], met_csr=True)
        assert after.table[(p, spec.SINK)] == (0, 1, 0, 0) and stats["records"] == 1
        assert r.raw["warm_started"] == 1


def test_additions_overflow_a_classs_segment_then_land_in_place():
    spec = cluster()
    with native.Context(0, **STATES["warm"]) as ctx:
        prepare(ctx, spec, "warm", True)
        snap = Snapshot(ctx)
        lst = held(snap, spec.X) + [(spec.M0 + k, 70, 2) for k in range(120)]
        b0 = ctx.store_stats()["rebuilds"]
        ref, stats, after, r = nodes_and_check(ctx, [spec.X], [lst], met_csr=True)
        assert stats["arcs_added"] == stats["records"] == 120
        assert r.raw["rebuilt"] == 1 and ctx.store_stats()["rebuilds"] == b0 + 1   # a full segment: rebuilt from the table
        more = held(after, spec.X) + [(spec.M0 + 120 + k, 70, 2) for k in range(5)]
        ref, stats, after, r = nodes_and_check(ctx, [spec.X], [more], met_csr=True)
        assert r.raw["rebuilt"] == 0 and stats["records"] == 5 and ctx.store_stats()["rebuilds"] == b0 + 1


@EVERY_STATE
def test_a_call_with_no_record_keeps_the_mapping(state):
    spec = cluster()
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, True)
        ctx.solve()
        mapping = ctx.task_mapping()
        snap = Snapshot(ctx)
        tails = [spec.X, spec.R0, spec.M0 + 1, spec.P0 + 1, spec.U0]
        lists = [held(snap, u) for u in tails]
        lists[1] = [(d, c, CAP_KEEP if i % 2 else cap) for i, (d, c, cap) in enumerate(lists[1])] + [(spec.M0 + 90, 4, 0)]
        for keep in (False, True):
            ref, stats, after, _ = nodes_and_check(ctx, tails, lists, keep=keep)
            assert stats["records"] == 0 and stats["arcs_skipped"] == 1 and stats["arcs_unchanged"] == 2 + 70 + 1 + 1 + 1
            assert ctx.task_mapping() == mapping                    # the mapping is still served
        stats = ctx.update_nodes([], [0], [], [], [])
        assert not any(stats.values()) and ctx.task_mapping() == mapping


# -------------------------------------------------------- UpdateResourceTopology ---
def chain_caps(spec, table) -> dict:
    m = spec.M0
    return {k: table.get(k, (0, 0))[1] for k in ((m, spec.P0), (spec.R0, m), (spec.X, spec.R0))}


@pytest.mark.parametrize("state", ["cell", "engine", "warm"])
@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
@pytest.mark.parametrize("slots", [3, 1])
def test_the_update_resource_topology_recipe(state, preemptive, slots):
    """Machine 0's PU goes from 2 slots to 3 and to 1 while one task runs on it: the PU → sink arc
    through the call, then the capacity refresh of ks_complete_tasks with no task. Every capacity
    on the chain above the PU is what ks_topology_stats implied before the change, moved by the
    slot difference: slots below the head (preemptive), minus the tasks running there (pinned)."""
    spec = Jobs(2, 2, 2, 1, [(0, 0, 0, False), (0, 1, 0, False), (0, 2, 0, False), (0, None, 1, False)])
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, preemptive)
        sl, rn = ctx.topology_stats(2)
        before = Snapshot(ctx)
        p = spec.P0
        ref, stats, after, _ = nodes_and_check(ctx, [p], [[(spec.SINK, 0, slots)]], solve=False)
        assert stats["arcs_updated"] == stats["records"] == 1 and after.table[(p, spec.SINK)][1] == slots
        want = complete_reference(after.graph(), [], bound(ctx), True, preemptive, alive=after.alive)
        left, cstats = ctx.complete_tasks([], resource_caps=True, preemptive=preemptive)
        assert left.shape[0] == 0 and cstats["cap_updates"] == 3
        done = Snapshot(ctx)
        assert done.table == want.arcs
        for (u, v), cap in chain_caps(spec, done.table).items():
            below = int(sl[v - 1]) + slots - 2
            assert cap == (below if preemptive else below - int(rn[v - 1])), (u, v)
        off = {k: a[1] for k, a in done.table.items() if k not in chain_caps(spec, done.table) and k != (p, spec.SINK)}
        assert off == {k: before.table[k][1] for k in off}           # nothing off the chain moved
        resolve_and_check(ctx)


@pytest.mark.parametrize("state", ["cell", "engine", "warm"])
def test_a_full_pu_gains_a_slot_under_the_pinned_rule(state):
    """Pinned, one slot per PU, tasks running on machines 0 and 1: rack 0 is full, and the commit's
    capacity rule has deleted M0 → P0, R0 → M0, M1 → P1, R0 → M1 and X → R0. P0 goes to 2 slots.
    PU → sink and the refresh alone (the recipe as the header first gave it) leave the new slot cut
    off: the refresh writes only arcs that exist. KS_CAP_KEEP on the chain is refused, there is
    nothing to keep. The completed recipe lists the chain arcs the rule had deleted with an explicit
    positive capacity in the same call (ADD_ARC), and the refresh then sets them: the new slot can
    be reached from X again."""
    spec = Jobs(2, 2, 1, 1, [(0, 0, 0, False), (0, 1, 0, False), (0, None, 1, False)])
    X, R, M, P, SINK = spec.X, spec.R0, spec.M0, spec.P0, spec.SINK
    chain = [(X, R), (R, M), (M, P)]
    with native.Context(0, **STATES[state]) as ctx:
        prepare(ctx, spec, state, False)
        before = Snapshot(ctx)
        assert bound(ctx) == {spec.task(0): P, spec.task(1): P + 1, spec.task(2): 0}
        assert not [k for k in chain + [(R, M + 1), (M + 1, P + 1)] if k in before.table]
        other = (R + 1, 0, CAP_KEEP)                                    # X is a type-0 tail: its arc into rack 1 stays listed
        rc, msg, _ = raw_call(ctx, [P, M, R, X], [[(SINK, 0, 2)], [(P, 0, CAP_KEEP)], [(M, 0, CAP_KEEP)], [(R, 0, CAP_KEEP), other]])
        assert rc == native.KS_E_INVALID and "KS_CAP_KEEP" in msg and f"node {M}" in msg and Snapshot(ctx).table == before.table
        ref, stats, after, _ = nodes_and_check(ctx, [P, M, R, X], [[(SINK, 0, 2)], [(P, 0, 1)], [(M, 0, 1)], [(R, 0, 1), other]],
                                               solve=False)
        assert (stats["arcs_updated"], stats["arcs_added"], stats["arcs_unchanged"], stats["records"]) == (1, 3, 1, 4)
        want = complete_reference(after.graph(), [], bound(ctx), True, False, alive=after.alive)
        _, cstats = ctx.complete_tasks([], resource_caps=True, preemptive=False)
        done = Snapshot(ctx)
        assert done.table == want.arcs and cstats["cap_updates"] == 0       # 2 slots − 1 running: the 1 it was listed with
        assert [done.table[k][1] for k in chain] == [1, 1, 1] and (R, M + 1) not in done.table
        resolve_and_check(ctx)


# -------------------------------------------------------------- load spreading ---
SPREAD_PREEMPTION = 150


def spreading():
    """SINK 1, A 2 and C 3 (classes: every task → A, A → C with capacity 2, C → each machine), 6
    machines 4..9 of 2 slots in 2 racks' worth of PUs 10..15, U 16, 24 tasks 17..40."""
    ntype = [3, 0, 0] + [4] * 6 + [2] * 6 + [0] + [1] * 24
    supply = [-24] + [0] * 15 + [1] * 24
    arcs = {(16, 1): (0, 24, 0, 0), (2, 3): (0, 2, 0, 0)}
    for k in range(6):
        arcs[(3, 4 + k)] = (0, 2, 0, 0)
        arcs[(4 + k, 10 + k)] = (0, 2, 0, 0)
        arcs[(10 + k, 1)] = (0, 2, 0, 0)
    for t in range(17, 41):
        arcs[(t, 16)] = (0, 1, 100, 0)
        arcs[(t, 2)] = (0, 1, 10, 0)
    return ntype, supply, arcs


@pytest.mark.parametrize("state", ["cell", "engine", "warm"])
def test_six_rounds_of_load_spreading(state):
    """Each round: solve → preemptive commit without the capacity rule → ks_update_nodes with
    class → machine cost = the machine's running count and capacity = its free slots, both
    from ks_get_bindings → solve. A → C lets two tasks through per round, so the cluster fills
    over six rounds and every round's costs differ. The model is kept on the host alone
    (preempt_ref, nodes_ref): ks_get_graph is read only to compare against it."""
    ntype, supply, table = spreading()
    tasks = list(range(17, 41))
    with native.Context(0, **STATES[state]) as ctx:
        ctx.load_graph(Spec(ntype, supply, list(table.items()), {}).graph(running=False))
        bindings: dict = {}
        placed = 0
        for rnd in range(6):
            r = ctx.solve()
            g = table_graph(ntype, supply, table)
            st, cost, flow, _ = ko.cost_scaling(g)
            assert st == 0 and (r.cost, r.flow) == (cost, flow), rnd
            deltas, _ = ctx.commit_preemptive(continuation=0, preemption=SPREAD_PREEMPTION, resource_caps=False,
                                              unsched_ids=[16])
            table, bindings, _ = preempt_reference(g, triples(deltas), bindings, 0, SPREAD_PREEMPTION, False, [16])
            pus = ctx.bindings(tasks).tolist()
            assert dict(zip(tasks, pus)) == {t: bindings.get(t, 0) for t in tasks}
            running = [pus.count(10 + k) for k in range(6)]
            placed += 2
            assert sum(running) == placed and max(running) <= 2
            lists = [[(3, 0, 2)], [(4 + k, running[k], 2 - running[k]) for k in range(6)]]
            ref = nodes_reference(ntype, table, [2, 3], lists)
            stats = ctx.update_nodes([2, 3], *offsets3(lists))
            assert stats == ref.stats and stats["records"] > 0, rnd
            table = ref.arcs
            assert Snapshot(ctx).table == table
            assert ctx.store_stats()["superseded"] == 0
        r = ctx.solve()
        st, cost, flow, _ = ko.cost_scaling(table_graph(ntype, supply, table))
        assert st == 0 and (r.cost, r.flow) == (cost, flow) and placed == 12
        assert not [k for k in table if k[0] == 3]                  # every machine is full: the class has no arc left


# -------------------------------------------------------------------- refusals ---
def raw_call(ctx, nodes, lists, flags=0, off=None):
    L, h = ctx._L, ctx._h
    t = np.asarray(nodes, np.uint64)
    o, dst, cost, cap = offsets3(lists)
    if off is not None:
        o = np.asarray(off, np.uint64)
    arcs = np.zeros(max(dst.shape[0], 1), native.NODE_ARC_DT)
    arcs["dst"][:dst.shape[0]], arcs["cost"][:dst.shape[0]], arcs["cap"][:dst.shape[0]] = dst, cost, cap
    st = native.KsNodeStats()
    rc = L.ks_update_nodes(h, flags, t.ctypes.data, t.shape[0], o.ctypes.data, arcs.ctypes.data, st)
    return rc, L.ks_last_error(h).decode(), st.as_dict()


@pytest.mark.parametrize("solved", [False, True], ids=["fresh", "solved"])
def test_refusals_change_nothing(solved):
    spec = priced()                                                 # job 1's arc into the sink has a lower bound of 1
    X, R, M, P, U, SINK = spec.X, spec.R0, spec.M0, spec.P0, spec.U0, spec.SINK
    INVALID, RANGE, VERIFY = native.KS_E_INVALID, native.KS_E_RANGE, native.KS_E_VERIFY
    BIG = (1 << 40) + 1
    with native.Context(0) as ctx:
        ctx.load_graph(spec.graph(running=True))
        ctx.set_bindings(spec.bindings)
        ctx.remove_resources([M + 139], resource_caps=False)        # two dead ids: the last machine and its PU
        dead = M + 139
        if solved:
            ctx.solve()
            d0 = ctx.scheduling_deltas(commit=False)
            m0 = ctx.task_mapping()
        before = Snapshot(ctx)
        assert dead not in before.alive and before.table[(U + 1, SINK)][0] == 1
        s0 = ctx.store_stats()
        n = int(before.nodes["id"].max())
        task = spec.task(0)

        def refused(code, names, nodes, lists, **kw):
            rc, msg, st = raw_call(ctx, nodes, lists, **kw)
            assert rc == code, (rc, msg)
            for x in names:
                assert str(x) in msg, msg
            assert not any(st.values())
            now = Snapshot(ctx)
            assert now.table == before.table and now.alive == before.alive and (now.nodes == before.nodes).all()
            assert ctx.store_stats() == s0
            if solved:                                               # the valid solution and the mapping stand
                assert (ctx.scheduling_deltas(commit=False) == d0).all() and ctx.task_mapping() == m0

        one = [(R, 0, CAP_KEEP)]
        with pytest.raises(BelowLowerBound):                        # the rule agrees on the one KS_E_VERIFY below
            nodes_reference(before.ntype, before.table, [U + 1], [[(SINK, 40, 0)]], alive=before.alive)
        for flags in (0, native.KS_NODES_KEEP_UNLISTED):
            for bad in (dead, task, SINK, n + 500, 10 ** 7, 0):     # dead, a task, a sink, beyond the graph, 0
                refused(INVALID, [f"node {bad} "], [X, bad, 0], [one, [], []], flags=flags)
            refused(INVALID, [f"node {X} "], [X, R, X, 0], [one, [], one, []], flags=flags)           # listed a second time
            for head in (dead, task, n + 500, 10 ** 7, 0, R):       # dead, a task, beyond the graph, 0, the tail itself
                refused(INVALID, [f"node {R}", f"head {head} "], [X, R, M],   # the head before the cost and the capacity
                        [one, [(M, 0, 2), (head, BIG, 1 << 60)], [(0, 0, 0)]], flags=flags)
            refused(INVALID, [f"node {P}", f"head {M} "], [X, P], [one, [(M, 0, 1)]], flags=flags)    # a PU's only head is a sink
            refused(INVALID, [f"node {M}", f"head {SINK} "], [X, M], [one, [(SINK, 0, 1)]], flags=flags)   # a machine → sink
            refused(INVALID, [f"node {R}", f"head {M} ", "twice"], [X, R], [one, [(M, 0, 2), (M + 1, 0, 2), (M, BIG, 2)]],
                    flags=flags)                                    # a held head twice, before its cost
            refused(INVALID, [f"node {R}", f"head {M + 80} ", "twice"], [X, R],
                    [one, [(M + 80, 0, 2), (M + 1, 0, 2), (M + 80, 0, 2)]], flags=flags)              # an absent head twice
            refused(RANGE, [f"node {R}", "cost", f"into {M}"], [X, R], [one, [(M, BIG, 1 << 60)]], flags=flags)   # cost, then capacity
            refused(RANGE, [f"node {R}", "cost"], [X, R], [one, [(M, -BIG, 2)]], flags=flags)
            refused(RANGE, [f"node {R}", "capacity", f"into {M + 1}"], [X, R], [one, [(M, 0, 2), (M + 1, 0, (1 << 53) + 1)]],
                    flags=flags)
            refused(RANGE, [f"node {X}", "capacity"], [X, R], [[(R, 0, CAP_KEEP - 1)], [(0, 0, 0)]], flags=flags)   # the first in input order
            # the arcs' form comes before the store's answers
            refused(RANGE, [f"node {R}", "cost"], [X, R], [[(M + 80, 0, CAP_KEEP)], [(M + 1, BIG, 2)]], flags=flags)
            refused(INVALID, [f"node {X}", "KS_CAP_KEEP", f"into {M + 80}"], [X, R], [[(M + 80, 0, CAP_KEEP)], [(M + 1, 0, 2)]],
                    flags=flags)                                    # nothing to keep
            refused(VERIFY, [f"node {U + 1}", "lower bound"], [X, U + 1], [one, [(SINK, 40, 0)]], flags=flags)
            refused(VERIFY, [f"node {U + 1}", "lower bound"], [U + 1, X], [[(SINK, 40, 0)], [(M + 80, 0, CAP_KEEP)]],
                    flags=flags)                                    # the first in input order of the two
            refused(INVALID, [f"node {X}", "KS_CAP_KEEP"], [X, U + 1], [[(M + 80, 0, CAP_KEEP)], [(SINK, 40, 0)]], flags=flags)
        refused(INVALID, ["arc_off"], [X, R], [one, one], off=[0, 2, 1])             # decreasing offsets
        refused(INVALID, ["arc_off[0]"], [X, R], [one, one], off=[1, 1, 2])
        refused(INVALID, ["flag"], [X], [one], flags=2)
        refused(INVALID, ["flag"], [X], [one], flags=native.KS_NODES_KEEP_UNLISTED | 4)
        # the bounds themselves are accepted
        rc, msg, st = raw_call(ctx, [R], [[(M, 1 << 40, 1 << 53), (M + 1, -(1 << 40), CAP_KEEP)]],
                               flags=native.KS_NODES_KEEP_UNLISTED)
        assert rc == native.KS_OK, msg
        assert (st["arcs_updated"], st["records"]) == (2, 2)
        assert Snapshot(ctx).table[(R, M)] == (0, 1 << 53, 1 << 40, 0)


# ---------------------------------------------------------------- the log line ---
def test_update_nodes_line():
    """tools/nodes_measure.py reads its phases out of the log_cycles line: exactly one line, and
    the record count in it is the stats' `records`."""
    spec_ = importlib.util.spec_from_file_location("delta_log_nodes_measure", os.path.join(TOOLS, "nodes_measure.py"))
    tool = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(tool)
    spec = cluster()
    with native.Context(0, log_cycles=1) as ctx:
        with tool.Stderr():
            ctx.load_graph(spec.graph(running=True))
        with tool.Stderr() as log:
            stats = ctx.update_nodes([spec.R0, spec.P0], [0, 2, 3], [spec.M0, spec.M0 + 70, spec.SINK], [5, 1, 2],
                                     [CAP_KEEP, 2, 3])
    lines = list(re.finditer(tool.NOD_RE, log.text))
    assert len(lines) == 1, log.text
    assert stats["records"] == 69 + 1 + 1 + 1                       # 69 dropped, one re-costed, one added, the PU's slots
    assert [int(x) for x in lines[0].groups()[:3]] == [2, 3, stats["records"]]
