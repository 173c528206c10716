"""CPU: the caller-and-model of tests/round_ref.py driven by the oracle instead of a device —
12 rounds of INTEGRATION §2.1 in both modes, with the invariants that tie the single-call rules
together asserted after every call, the coverage counters the GPU runs rely on, and one short
sequence on the toy network with every expected table written out by hand."""
import pytest

from nodes_ref import CAP_KEEP, InvalidNodes
from preempt_ref import TOY_ARCS, TOY_NTYPE, TOY_SUPPLY
from round_ref import (COST_ADD, COST_SET, PLACE, PREEMPT, OracleBackend, ReplayBackend, RoundFailure, RoundModel, Script, hub_case,
                       run, small_case, unsched_costs_reference, wave_case)

SEEDS = [1, 2, 3, 4, 5, 6]
# with classes: seeds at which the MODEL's inputs reach every counter below, whichever optimum a solver picks among
# the ties (checked with the oracle's two solvers); test_gpu_rounds.py runs two of them
CLASS_SEEDS = [1, 3, 7, 17, 19, 20]
BOTH_MODES = pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
ROUNDS = 12


@BOTH_MODES
@pytest.mark.parametrize("seed", SEEDS)
def test_twelve_rounds_keep_every_invariant_and_reach_every_path(seed, preemptive, tmp_path):
    """run() asserts after every call: no dangling arc; every aggregator → sink capacity is the
    number of live tasks holding an arc into the aggregator (absent at 0); the capacity refresh has
    nothing to write; bindings and running arcs agree; the next solve is feasible with one unit per
    live task (except while a task evicted after a pinned commit waits, arcless, for its return in
    the same round). Then the coverage counters."""
    m, script, _ = small_case(preemptive, seed, ROUNDS)
    n = run(m, script, OracleBackend(), ROUNDS, tmp_path)
    assert n["evictions"] > 0
    assert n["bound_id_reused"] > 0 and n["pu_id_reused"] > 0
    assert n["aggregator_recreated"] > 0 and n["new_jobs"] == 2
    assert n["superseded"] > 0
    if preemptive:
        assert n["migrations"] > 0 and n["preemptions"] > 0 and n["running_kept"] > 0
        assert n["stale_caps_repaired"] > 0      # the refresh after ks_add_resources had a capacity to put right
    else:
        assert n["ancestor_recreated"] > 0 and n["recipe_upserts"] > 0
    calls = {x["call"] for x in m.log}
    assert {"solve", "commit", "remove", "complete", "grow", "refresh_caps", "arrive", "refresh", "age"} <= calls
    assert all(x["round"] <= ROUNDS for x in m.log)


@BOTH_MODES
@pytest.mark.parametrize("case", [wave_case, hub_case])
def test_the_larger_cases_of_the_gpu_suite_reach_their_paths(case, preemptive, tmp_path):
    """The wave-and-class case (a 150-task job, a 65-task burst, a rack that grows by 12 machines a
    round) and the hub (more than 4,096 arcs into one aggregator), as test_gpu_rounds.py runs them."""
    m, script, rounds = case(preemptive)
    n = run(m, script, OracleBackend(), rounds, tmp_path)
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["pu_id_reused"] > 0 and n["aggregator_recreated"] > 0
    assert n["superseded"] > 0 and (preemptive or (n["ancestor_recreated"] > 0 and n["recipe_upserts"] > 0))
    big = max(m.aggs, key=lambda a: m.arcs.get((a, m.sink), (0, 0))[1])
    held = sum(1 for (s, d) in m.arcs if d == big)
    assert held > (4096 if case is hub_case else 64)
    if case is wave_case:
        sizes = [len(x["tasks"]) for x in m.log if x["round"] == 2 and x["call"] in ("complete", "arrive")]
        assert sizes[0] == 65 and sizes[1] >= 65


def check_class_counters(n, preemptive):
    """What the model's inputs must have held for ks_update_nodes. Under the preemptive rule a
    class arc is never listed with capacity 0 (a machine's room is its slots) and no commit deletes
    one, so class_arcs_zeroed, class_arc_recreated and chain_relisted are pinned mode's."""
    assert n["class_arcs_added"] > 0 and n["class_arcs_removed"] > 0 and n["cap_overwritten"] > 0
    assert n["resource_recosted"] > 0 and n["resource_unchanged"] > 0
    assert n["slots_raised"] == 1 and n["slots_lowered"] == 1
    if not preemptive:
        assert n["class_arcs_zeroed"] > 0 and n["class_arc_recreated"] > 0 and n["chain_relisted"] > 0


@BOTH_MODES
@pytest.mark.parametrize("seed", CLASS_SEEDS)
def test_twelve_rounds_with_classes_and_a_cost_model_that_moves(seed, preemptive, tmp_path):
    """The ten-call round: ks_update_nodes lists every class's and every resource's arcs from the
    caller's knowledge alone, after the commits, removals, completions and additions have deleted,
    re-created and re-sized those arcs. Every invariant after every call (the cap-1 classes' arcs
    are the cost model's after ks_update_nodes and the rule's after any later call that runs it; no
    class holds an arc outside its set), then the counters."""
    m, script, _ = small_case(preemptive, seed, ROUNDS, classes=True)
    n = run(m, script, OracleBackend(), ROUNDS, tmp_path)
    check_class_counters(n, preemptive)
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["pu_id_reused"] > 0
    assert n["aggregator_recreated"] > 0 and n["new_jobs"] == 2 and n["superseded"] > 0
    assert preemptive or n["recipe_upserts"] > 0
    calls = [x["call"] for x in m.log]
    assert {"solve", "commit", "remove", "complete", "grow", "refresh_caps", "arrive", "refresh", "nodes", "age"} <= set(calls)
    assert calls.count("nodes") == ROUNDS and len(m.classes) == 5
    after = [calls[i + 1] for i, c in enumerate(calls) if c == "nodes"]
    assert after.count("refresh_caps") == 2 and after.count("age") == ROUNDS - 2     # the refresh follows the two slot changes


@BOTH_MODES
def test_the_wide_case_with_classes_reaches_its_paths(preemptive, tmp_path):
    """wave_case with classes: the 150-task job's class holds more than 64 arcs at a
    ks_update_nodes (its segment is walked in chunks), the class of round 4's new job takes every
    machine of the growing rack in its first call, and the rack's own segment overflows."""
    m, script, rounds = wave_case(preemptive, classes=True)
    n = run(m, script, OracleBackend(), rounds, tmp_path)
    assert n["class_tail_over_64"] > 0 and n["class_arcs_added"] > 0 and n["resource_recosted"] > 0
    assert n["evictions"] > 0 and n["bound_id_reused"] > 0 and n["superseded"] > 0
    calls = [x for x in m.log if x["call"] == "nodes"]
    wide = [len(lst) for x in calls for t, lst in zip(x["tails"], x["lists"]) if t == script.wide]
    assert len(wide) == 2 and max(wide) > 48 and len(calls) == rounds
    grown = [sum(1 for node in x["nodes"] if node[1] == 4) for x in m.log if x["call"] == "grow"]
    assert sorted(grown)[-5:] >= [12] * 5        # the rack's segment: twelve machines in each of five ks_add_resources


@BOTH_MODES
def test_a_failure_names_seed_and_round_and_leaves_the_call_log(preemptive, tmp_path):
    import json
    m = RoundModel.cluster(preemptive, 1)

    class Wrong(OracleBackend):
        def solve(self, model):
            cost, flow, flows, mapping = super().solve(model)
            return (cost + (model.round == 2), flow, flows, mapping)
    with pytest.raises(RoundFailure) as e:
        run(m, Script(m, 4), Wrong(), 4, tmp_path)
    assert "seed 1" in str(e.value) and "round 2" in str(e.value)
    log = json.load(open(tmp_path / "round_log_seed1.json"))
    assert log["seed"] == 1 and log["calls"][-1]["call"] == "solve" and log["calls"][-1]["round"] == 2
    assert {"commit", "arrive", "age"} <= {x["call"] for x in log["calls"]}


@BOTH_MODES
def test_a_call_log_replays_the_run_with_the_same_optima(preemptive, tmp_path):
    """The log holds every solve's answer, so a run is replayed without a solver choosing again:
    the same calls with the same arguments, the same graph at the end."""
    replay(False, preemptive, tmp_path)


@BOTH_MODES
def test_a_call_log_with_classes_replays_the_run_with_the_same_optima(preemptive, tmp_path):
    """The same with ks_update_nodes in the log (KS_CAP_KEEP goes through JSON as the integer it is)."""
    replay(True, preemptive, tmp_path)


def replay(classes, preemptive, tmp_path):
    import json
    m, script, _ = small_case(preemptive, 3, 6, classes)
    run(m, script, OracleBackend(), 6)
    log = json.load(open(m.dump(tmp_path / "log.json")))
    assert classes == ("nodes" in {x["call"] for x in log["calls"]})
    again, script, _ = small_case(preemptive, 3, 6, classes)
    run(again, script, ReplayBackend(log), 6)
    assert again.arcs == m.arcs and again.bindings == m.bindings and again.alive == m.alive
    assert json.load(open(again.dump(tmp_path / "again.json"))) == log


def test_unsched_costs_rule():
    """SINK 1, U 2, V 3 (an aggregator that is not marked), PU 4, tasks 5 (waiting), 6 (running,
    keeps its aggregator arc: preemptive), 7 (pinned: no aggregator arc), 8 (waits on V)."""
    ntype = [3, 0, 0, 2, 1, 1, 1, 1]
    arcs = {(2, 1): (0, 2, 0, 0), (3, 1): (0, 1, 0, 0), (4, 1): (0, 2, 0, 0),
            (5, 2): (0, 1, 100, 0), (5, 4): (0, 1, 9, 0),
            (6, 2): (0, 1, 20, 0), (6, 4): (0, 1, 0, 1),
            (7, 4): (1, 1, 0, 1), (8, 3): (0, 1, 100, 0)}
    out, changed = unsched_costs_reference(ntype, arcs, [2], COST_ADD, 7, 5)
    assert changed == 2 and out == {**arcs, (5, 2): (0, 1, 107, 0), (6, 4): (0, 1, 5, 1)}
    out, changed = unsched_costs_reference(ntype, arcs, [2], COST_SET, 100, 0)
    assert changed == 0 and out == arcs                          # the same costs: nothing is counted
    out, changed = unsched_costs_reference(ntype, arcs, [2, 3], COST_SET, 1, 0)
    assert changed == 2 and out == {**arcs, (5, 2): (0, 1, 1, 0), (8, 3): (0, 1, 1, 0)}


def test_toy_sequence_by_hand():
    """The toy network of preempt_ref (SINK 1, U 2, M1 3, P1 4, M2 5, P2 6, M3 7, P3 8, T1..T3
    9..11), pinned: one commit, the removal of M1 with an eviction, the evicted task's return, one
    completion from a full PU. Every table below was computed by hand from include/ksmcmf.h."""
    m = RoundModel(False, TOY_NTYPE, TOY_SUPPLY, TOY_ARCS, parent={4: 3, 6: 5, 8: 7}, slots={4: 1, 6: 1, 8: 1},
                   job={9: 2, 10: 2, 11: 2}, prefs={9: [(3, 1), (5, 5)], 10: [(3, 2), (5, 3)], 11: [(3, 50), (5, 50)]})
    dev = OracleBackend()
    cost, flow, flows, mapping = dev.solve(m)
    assert (cost, flow, mapping) == (64, 3, {9: 4, 10: 6})
    deltas = m.check_solution(cost, flow, flows, mapping)
    assert deltas == [(PLACE, 9, 4), (PLACE, 10, 6)]
    _, out = m.commit(deltas)
    assert out["stats"] == dict(placed=2, arcs_removed=6, running_added=2, running_converted=0, unsched_updates=1,
                                cap_updates=2, records=11)
    pus = {(4, 1): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (8, 1): (0, 1, 0, 0)}
    t11 = {(11, 3): (0, 1, 50, 0), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0)}
    assert m.arcs == {(2, 1): (0, 1, 0, 0), (7, 8): (0, 1, 0, 0), **pus, (9, 4): (1, 1, 0, 1), (10, 6): (1, 1, 0, 1), **t11}
    assert m.bindings == {9: 4, 10: 6}
    m.check_invariants()

    args, out = m.remove([3])                                    # P1 is full: no arc leads to it, it is named too
    assert args["roots"] == [3, 4]
    assert out == dict(removed=[3, 4], evicted=[(PREEMPT, 9, 4)],
                       stats=dict(roots=2, nodes_removed=2, pus_removed=1, tasks_evicted=1, arcs_removed=3, cap_updates=0,
                                  records=2))
    assert m.arcs == {(2, 1): (0, 1, 0, 0), (7, 8): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (8, 1): (0, 1, 0, 0),
                      (10, 6): (1, 1, 0, 1), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0)}
    assert m.bindings == {10: 6} and m.returning == [9] and m.free == [3, 4] and m.prefs[9] == [(5, 5)]
    m.check_invariants(feasible=False)                           # task 9 has no arc until it returns

    _, out = m.refresh([9], [[(5, 5), (2, 100)]])
    assert out["stats"] == dict(tasks=1, arcs_added=2, cost_updates=0, arcs_unchanged=0, running_kept=0, arcs_removed=0,
                                unsched_updates=1, unsched_added=0, records=3)
    assert m.arcs == {(2, 1): (0, 2, 0, 0), (7, 8): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (8, 1): (0, 1, 0, 0),
                      (10, 6): (1, 1, 0, 1), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0),
                      (9, 5): (0, 1, 5, 0), (9, 2): (0, 1, 100, 0)}
    assert m.returning == []
    m.check_invariants()

    ask, ups = m.complete_recipe([10])                           # P2 is full: M2 → P2 left the store with the pin
    assert ask == dict(tasks=[10], pu=[6])
    assert [(int(x["kind"]), int(x["src"]), int(x["dst"]), int(x["cap"])) for x in ups] == [(2, 5, 6, 1)]
    assert m.arcs[(5, 6)] == (0, 1, 0, 0)
    _, out = m.complete([10])
    assert out == dict(left=[6], stats=dict(tasks=1, bound=1, arcs_removed=1, unsched_updates=0, cap_updates=0, records=1))
    assert m.arcs == {(2, 1): (0, 2, 0, 0), (5, 6): (0, 1, 0, 0), (7, 8): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0),
                      (8, 1): (0, 1, 0, 0), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0),
                      (9, 5): (0, 1, 5, 0), (9, 2): (0, 1, 100, 0)}
    assert m.bindings == {} and m.free == [3, 4, 10] and m.alloc() == 3
    m.check_invariants()
    cost, flow, flows, mapping = dev.solve(m)                    # 9 → M2 → P2 (5), 11 → U (60): M3 has no task arc
    assert (cost, flow, mapping) == (65, 2, {9: 6})
    assert m.check_solution(cost, flow, flows, mapping) == [(PLACE, 9, 6)]


def test_toy_sequence_with_a_class_by_hand():
    """The toy network with one class, C 12: every task → C at 10, C → M1 at 4 and C → M2 at 6,
    capacity 1 each (the machines' room). Pinned: the commit fills M1 and M2 and the rule deletes
    C's arcs into them; KS_CAP_KEEP on one is refused and nothing changes; a completion with the
    recipe frees P2; ks_update_nodes with the cost model's explicit capacities re-adds C → M2 and
    skips C → M1. Every table below was computed by hand from include/ksmcmf.h."""
    C = 12
    arcs = {**TOY_ARCS, (C, 3): (0, 1, 4, 0), (C, 5): (0, 1, 6, 0), **{(t, C): (0, 1, 10, 0) for t in (9, 10, 11)}}
    m = RoundModel(False, TOY_NTYPE + [0], TOY_SUPPLY + [0], arcs, parent={4: 3, 6: 5, 8: 7}, slots={4: 1, 6: 1, 8: 1},
                   job={9: 2, 10: 2, 11: 2}, prefs={9: [(3, 1), (5, 5)], 10: [(3, 2), (5, 3)], 11: [(3, 50), (5, 50)]})
    m.add_class(2, C)
    m.pref[C], m.base = [3, 5], {(C, 3): 4, (C, 5): 6}
    m.check_invariants()
    assert m.full_list(11, True) == [(3, 50), (5, 50), (C, 200), (2, 1000)]       # (the toy's own costs stand in the table)
    dev = OracleBackend()
    cost, flow, flows, mapping = dev.solve(m)
    assert (cost, flow, mapping) == (64, 3, {9: 4, 10: 6})                      # the class changes no optimum: 10 + 4 > 1
    _, out = m.commit(m.check_solution(cost, flow, flows, mapping))
    assert out["stats"] == dict(placed=2, arcs_removed=8, running_added=2, running_converted=0, unsched_updates=1,
                                cap_updates=4, records=15)
    pus = {(4, 1): (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (8, 1): (0, 1, 0, 0)}
    t11 = {(11, 3): (0, 1, 50, 0), (11, 5): (0, 1, 50, 0), (11, 2): (0, 1, 60, 0), (11, C): (0, 1, 10, 0)}
    after_commit = {(2, 1): (0, 1, 0, 0), (7, 8): (0, 1, 0, 0), **pus, (9, 4): (1, 1, 0, 1), (10, 6): (1, 1, 0, 1), **t11}
    assert m.arcs == after_commit and m.commit_dropped == {(C, 3), (C, 5)}      # C → M1 and C → M2 went with the rule
    m.check_invariants()

    with pytest.raises(InvalidNodes) as e:                       # there is nothing to keep
        m.nodes([C], [[(3, 11, CAP_KEEP), (5, 13, CAP_KEEP)]])
    assert e.value.args == (C, 3)
    assert m.arcs == after_commit and m.log[-1]["call"] == "commit" and m.caps_from == "rule"
    assert m.class_list(C, [3, 5]) == [(3, 11, 0), (5, 13, 0)]   # the cost model: 4 + 7 × 1 and 6 + 7 × 1, no room
    _, out = m.nodes([C], [m.class_list(C, [3, 5])])
    assert out["stats"] == dict(nodes=1, arcs_added=0, arcs_updated=0, arcs_unchanged=0, arcs_skipped=2, arcs_zeroed=0,
                                arcs_removed=0, records=0)
    assert m.arcs == after_commit and m.count["class_arc_recreated"] == 0

    ask, ups = m.complete_recipe([10])                           # P2 is full: M2 → P2 left the store with the pin
    assert ask == dict(tasks=[10], pu=[6])
    assert [(int(x["kind"]), int(x["src"]), int(x["dst"]), int(x["cap"])) for x in ups] == [(2, 5, 6, 1)]
    _, out = m.complete([10])
    assert out == dict(left=[6], stats=dict(tasks=1, bound=1, arcs_removed=1, unsched_updates=0, cap_updates=0, records=1))
    assert (C, 5) not in m.arcs                                  # the recipe's chain is the resource tree's: the class arc stays away
    assert m.class_list(C, [3, 5]) == [(3, 11, 0), (5, 6, 1)]
    _, out = m.nodes([C, 5], [m.class_list(C, [3, 5]), [(6, 1, CAP_KEEP)]])
    assert out["stats"] == dict(nodes=2, arcs_added=1, arcs_updated=1, arcs_unchanged=0, arcs_skipped=1, arcs_zeroed=0,
                                arcs_removed=0, records=2)
    after_commit.pop((10, 6))
    assert m.arcs == {**after_commit, (5, 6): (0, 1, 1, 0), (C, 5): (0, 1, 6, 0)}
    assert m.count["class_arc_recreated"] == 1 and m.count["class_arcs_added"] == 1 and m.count["resource_recosted"] == 1
    m.check_invariants()
    cost, flow, flows, mapping = dev.solve(m)                    # 11 → C → M2 → P2: 10 + 6 + 1 + 0, cheaper than 11 → M2 at 50
    assert (cost, flow, mapping) == (17, 2, {9: 4, 11: 6})
    assert m.check_solution(cost, flow, flows, mapping) == [(PLACE, 11, 6)]
