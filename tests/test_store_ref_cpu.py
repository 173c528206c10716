"""The store reference (tests/store_ref.py) checked on the CPU: its state against
graphs.apply_deltas_to_arcs and ks_coalesce_deltas, and its expected counters on
hand-written streams, one per rule of ks_store_stats (include/ksmcmf.h)."""
import numpy as np
import pytest

from graphs import ADVERSARIAL_SEEDS, graph_from_lists, random_hub_graphs, random_stream
from ksched_amd import native
from oracle import ko
from store_ref import StoreRef, delta, stream

ADD_NODE, REMOVE_NODE, ADD_ARC, UPDATE_ARC, SET_EXCESS = range(5)


def base():
    """1 → 2 → 3 → 4, 1 → 3, 2 → 4; node 5 isolated."""
    nodes = [(1, 2, 1), (2, 0, 0), (3, 0, 2), (4, -2, 3), (5, 0, 0)]
    arcs = [(1, 2, 0, 2, 1), (2, 3, 0, 2, 1), (3, 4, 0, 2, 1), (1, 3, 0, 1, 5), (2, 4, 0, 1, 7)]
    return StoreRef.from_graph(graph_from_lists(nodes, arcs))


def arc(kind, s, d, low=0, cap=1, cost=0, type=0):
    return delta(kind=kind, src=s, dst=d, low=low, cap=cap, cost=cost, type=type)


def test_remove_add_remove_add_of_one_id_with_arcs_before_between_and_after():
    ref = base()
    st = ref.apply(stream([
        arc(UPDATE_ARC, 1, 2, cap=3, cost=2),           # before the removals: dead (purged by the first removal)
        delta(kind=REMOVE_NODE, id=2),
        delta(kind=ADD_NODE, id=2, excess=0, type=5),
        arc(ADD_ARC, 1, 2, cap=4, cost=3, type=1),      # between: superseded by the record below, and killed anyway
        arc(ADD_ARC, 2, 4, cap=9, cost=9),              # between: killed by the second removal, key was in the store
        delta(kind=REMOVE_NODE, id=2),
        delta(kind=ADD_NODE, id=2, excess=0, type=4),
        arc(ADD_ARC, 1, 2, cap=5, cost=4, type=300),    # after: the arc as it stands, re-inserted; type clamped
    ]))
    assert ref.nodes[2] == [0, 4]
    assert ref.arcs == {(1, 2): (0, 5, 4), (3, 4): (0, 2, 1), (1, 3): (0, 1, 5)}
    assert ref.atype == {(1, 2): 255, (3, 4): 0, (1, 3): 0}
    # (1,2) has three records → 2 superseded; (2,3) and (2,4) were in the store and are gone
    assert st == {"superseded": 2, "killed": 2, "live_arcs": 3, "upserts_new": 1, "upserts_inplace": 0}


def test_update_zero_of_a_missing_key_and_add_on_an_existing_key_and_update_on_a_missing_key():
    ref = base()
    st = ref.apply(stream([
        arc(UPDATE_ARC, 1, 4, low=0, cap=0),            # delete of a key the store never had: nothing
        arc(ADD_ARC, 1, 2, low=1, cap=2, cost=8),       # ADD on an existing key: an upsert in place
        arc(UPDATE_ARC, 5, 4, cap=3, cost=1, type=1),   # UPDATE on a missing key: inserted
        arc(ADD_ARC, 3, 4, low=0, cap=0, cost=1),       # an ADD to capacity 0 keeps the arc (only UPDATE 0/0 deletes)
        arc(UPDATE_ARC, 2, 3, low=0, cap=0),            # the delete proper
    ]))
    assert ref.arcs == {(1, 2): (1, 2, 8), (3, 4): (0, 0, 1), (1, 3): (0, 1, 5), (2, 4): (0, 1, 7), (5, 4): (0, 3, 1)}
    assert ref.atype[(5, 4)] == 1
    assert st == {"superseded": 0, "killed": 1, "live_arcs": 5, "upserts_new": 1, "upserts_inplace": 2}


def test_delete_then_recreate_is_one_in_place_edit():
    ref = base()
    st = ref.apply(stream([arc(UPDATE_ARC, 1, 3, low=0, cap=0), arc(ADD_ARC, 1, 3, cap=6, cost=2),
                           arc(ADD_ARC, 1, 5, cap=1), arc(UPDATE_ARC, 1, 5, low=0, cap=0)]))
    assert ref.arcs[(1, 3)] == (0, 6, 2) and (1, 5) not in ref.arcs
    assert st == {"superseded": 2, "killed": 0, "live_arcs": 5, "upserts_new": 0, "upserts_inplace": 1}


def test_an_endpoint_removed_earlier_makes_a_kept_key_a_new_insert():
    ref = base()
    st = ref.apply(stream([delta(kind=REMOVE_NODE, id=3), delta(kind=ADD_NODE, id=3, excess=0, type=2),
                           arc(ADD_ARC, 3, 4, cap=2, cost=1),     # was in the store, its positions went with node 3
                           arc(UPDATE_ARC, 1, 2, cap=2, cost=2)]))
    assert st == {"superseded": 0, "killed": 2, "live_arcs": 3, "upserts_new": 1, "upserts_inplace": 1}


@pytest.mark.parametrize("seed,adversarial", [(5, False), (6, False), (24, True), (31, True), (28, True)])
def test_random_streams_against_the_restatement_and_coalescing(seed, adversarial):
    """Random streams: StoreRef's state is apply_deltas_to_arcs's, record for record
    (the generator applies that function itself as it emits), and the coalesced
    stream (ks_coalesce_deltas) leaves the same state with nothing superseded and
    the same killed and live_arcs."""
    rng = np.random.default_rng(seed)
    g = next(g for _, g in random_hub_graphs(seed, 20, n_lo=1500, n_hi=4000) if ko.ssp(g)[0] == 0)
    nodes = {i + 1: [int(g.supply[i]), int(g.ntype[i])] for i in range(g.n)}
    arcs = {(int(s), int(d)): (int(lo), int(c), int(k))
            for s, d, lo, c, k in zip(g.src, g.dst, g.low, g.cap, g.cost)}
    raw, coal = StoreRef.from_graph(g), StoreRef.from_graph(g)
    hubs_removed = 0
    for rnd in range(2):
        deg0 = {}
        for k in arcs:
            for i in k:
                deg0[i] = deg0.get(i, 0) + 1
        keys0 = set(arcs)
        s = random_stream(rng, nodes, arcs, 2000, g.hubs, adversarial)
        a = raw.apply(s)
        assert (raw.nodes, raw.arcs) == (nodes, arcs)
        c = native.coalesce_deltas(s)
        assert c.shape[0] < s.shape[0]
        b = coal.apply(c)
        assert (coal.nodes, coal.arcs, coal.atype) == (raw.nodes, raw.arcs, raw.atype)
        assert b["superseded"] == 0 and a["superseded"] > 0
        assert (b["killed"], b["live_arcs"]) == (a["killed"], a["live_arcs"])
        # what decides new against in place is the removal of an endpoint, which coalescing keeps
        assert (b["upserts_new"], b["upserts_inplace"]) == (a["upserts_new"], a["upserts_inplace"])
        rm = [int(x["id"]) for x in s if int(x["kind"]) == REMOVE_NODE]
        hubs_removed += sum(deg0.get(i, 0) >= 64 for i in rm)
        if adversarial:   # an arc of the store with both endpoints removed in this stream
            assert any(k[0] in rm and k[1] in rm for k in keys0)
    assert hubs_removed >= (1 if adversarial else 0)


@pytest.mark.parametrize("seed,solve_first", ADVERSARIAL_SEEDS)
def test_adversarial_seeds_keep_two_rounds_feasible(seed, solve_first):
    """The seeds of test_gpu_stress's adversarial cases, on the oracle alone: at least
    two of their four rounds are feasible (the condition that GPU test asserts)."""
    from graphs import graph_from_store
    rng = np.random.default_rng(seed)
    g = next(g for _, g in random_hub_graphs(seed, 20, n_lo=1500, n_hi=4000) if ko.ssp(g)[0] == 0)
    nodes = {i + 1: [int(g.supply[i]), int(g.ntype[i])] for i in range(g.n)}
    arcs = {(int(s), int(d)): (int(lo), int(c), int(k))
            for s, d, lo, c, k in zip(g.src, g.dst, g.low, g.cap, g.cost)}
    feasible = 0
    for rnd in range(4):
        random_stream(rng, nodes, arcs, 2000, g.hubs, True)
        feasible += ko.ssp(graph_from_store(nodes, arcs))[0] == 0
    assert feasible >= 2
