"""CPU: the caller-and-model of tests/round_ref.py driven by the oracle instead of a device —
12 rounds of INTEGRATION §2.1 in both modes, with the invariants that tie the single-call rules
together asserted after every call, the coverage counters the GPU runs rely on, and one short
sequence on the toy network with every expected table written out by hand."""
import pytest

from preempt_ref import TOY_ARCS, TOY_NTYPE, TOY_SUPPLY
from round_ref import (COST_ADD, COST_SET, PLACE, PREEMPT, OracleBackend, ReplayBackend, RoundFailure, RoundModel, Script, hub_case,
                       run, small_case, unsched_costs_reference, wave_case)

SEEDS = [1, 2, 3, 4, 5, 6]
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
    import json
    m, script, _ = small_case(preemptive, 3, 6)
    run(m, script, OracleBackend(), 6)
    log = json.load(open(m.dump(tmp_path / "log.json")))
    again, script, _ = small_case(preemptive, 3, 6)
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
