"""CPU: the restatement of ks_add_resources (tests/grow_ref.py) checked by hand on the 19-node
toy, against the store semantics (graphs.apply_deltas_to_arcs), against ks_remove_resources'
restatement (a machine removed and added back gives the graph it left) and against
ks_complete_tasks' (after a call with full chains its capacity refresh has nothing to write),
and the library's and the binding's new entry point with the layout of its three structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from commit_ref import arc_table
from complete_ref import complete_reference
from graphs import apply_deltas_to_arcs
from grow_ref import (EXTRA, STAT_KEYS, TREE, Growth, InvalidGrowth, OutOfRange, chain, grow_reference,
                      tree_parents)
from ksched_amd import gen, native
from preempt_ref import table_graph
from remove_ref import TOY_ARCS, TOY_BINDINGS, TOY_NTYPE, TOY_SUPPLY, remove_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINK, X, R1, R2, M1, M4, P1, P4 = 1, 2, 3, 4, 5, 8, 9, 12


def toy(arcs=None):
    return table_graph(TOY_NTYPE, TOY_SUPPLY, TOY_ARCS if arcs is None else arcs)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["id"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]),
             int(x["cost"]), int(x["type"]), int(x["excess"])) for x in stream]


def refreshed(g, preemptive, alive=None):
    """The capacity refresh of ks_complete_tasks(k = 0, resource caps): (table, records)."""
    r = complete_reference(g, [], {}, True, preemptive, unsched_ids=[], alive=alive)
    return r.arcs, r.stats["cap_updates"]


# ---- by hand on the toy ------------------------------------------------------------
def test_toy_a_machine_and_its_pu_under_a_rack():
    """Machine 20 with PU 21 (2 slots) under R1, the chain X → R1 listed last."""
    nodes = [(20, 4, 0, 0), (21, 2, 2, 7)]
    edges = [(R1, 20, 5, TREE), (20, 21, 6, TREE), (X, R1, 9, TREE)]
    r = grow_reference(toy(), nodes, edges)
    assert stream_rows(r.stream) == [(0, 20, 0, 0, 0, 0, 0, 4, 0), (0, 21, 0, 0, 0, 0, 0, 2, 0),
                                     (2, 0, 21, 1, 0, 2, 7, 0, 0),
                                     (2, 0, 3, 20, 0, 2, 5, 0, 0), (2, 0, 20, 21, 0, 2, 6, 0, 0),
                                     (3, 0, 2, 3, 0, 6, 0, 0, 0)]                 # X → R1: 4 + 2, its own cost kept
    assert r.stats == dict(nodes=2, pus=1, slots=2, sink_arcs=1, arcs_added=2, cap_updates=1, arcs_skipped=0, records=6)
    want = dict(TOY_ARCS)
    want.update({(21, 1): (0, 2, 7, 0), (3, 20): (0, 2, 5, 0), (20, 21): (0, 2, 6, 0), (2, 3): (0, 6, 0, 0)})
    assert r.arcs == want and r.S == {21: 2, 20: 2, 3: 2, 2: 2}
    assert r.alive == set(range(1, 22)) and r.ntype[19:] == [4, 2] and r.supply[19:] == [0, 0]


def test_toy_a_rack_of_two_machines_and_an_arc_the_store_lost():
    """Rack 30 under X with machines 31 (PUs 33 of 3 slots, 35 of 1) and 32 (PU 34, 5 slots); an
    EXTRA arc R2 → 31. A lone PU 40 joins the full machine M1 whose rack arc the store dropped:
    R1 → M1 is re-created with the input cost, M1 → P-new is new, X → R1 is raised."""
    arcs = dict(TOY_ARCS)
    del arcs[(R1, M1)]                                                           # capacity fell to 0: the arc left
    arcs[(X, R1)] = (1, 2, 40, 0)                                                # low and cost of a held arc are kept
    nodes = [(30, 0, 0, 0), (33, 2, 3, 1), (31, 4, 0, 0), (32, 4, 0, 0), (34, 2, 5, -2), (35, 2, 1, 0), (40, 2, 4, 0)]
    edges = [(31, 33, 0, TREE), (30, 31, 11, TREE), (X, 30, 12, TREE), (32, 34, 0, TREE), (30, 32, 13, TREE),
             (31, 35, 0, TREE), (R2, 31, 14, EXTRA), (M1, 40, 15, TREE), (R1, M1, 16, TREE), (X, R1, 17, TREE)]
    r = grow_reference(toy(arcs), nodes, edges)
    assert r.S == {33: 3, 35: 1, 34: 5, 31: 4, 32: 5, 30: 9, 40: 4, M1: 4, R1: 4, X: 13}
    rows = stream_rows(r.stream)
    assert [x[1] for x in rows[:7]] == [30, 33, 31, 32, 34, 35, 40]
    assert rows[7:11] == [(2, 0, 33, 1, 0, 3, 1, 0, 0), (2, 0, 34, 1, 0, 5, -2, 0, 0), (2, 0, 35, 1, 0, 1, 0, 0, 0),
                          (2, 0, 40, 1, 0, 4, 0, 0, 0)]
    assert rows[11:] == [(2, 0, 31, 33, 0, 3, 0, 0, 0), (2, 0, 30, 31, 0, 4, 11, 0, 0), (2, 0, 2, 30, 0, 9, 12, 0, 0),
                         (2, 0, 32, 34, 0, 5, 0, 0, 0), (2, 0, 30, 32, 0, 5, 13, 0, 0), (2, 0, 31, 35, 0, 1, 0, 0, 0),
                         (2, 0, 4, 31, 0, 4, 14, 0, 0), (2, 0, 5, 40, 0, 4, 15, 0, 0),
                         (2, 0, 3, 5, 0, 4, 16, 0, 0),                           # re-created: the input cost
                         (3, 0, 2, 3, 1, 6, 40, 0, 0)]                           # held: low 1 and cost 40 kept
    assert r.stats == dict(nodes=7, pus=4, slots=13, sink_arcs=4, arcs_added=9, cap_updates=1, arcs_skipped=0,
                           records=21)


def test_toy_an_empty_rack_then_a_machine_under_it():
    first = grow_reference(toy(), [(20, 0, 0, 0)], [(X, 20, 3, TREE), (R1, M1, 0, TREE)])
    assert stream_rows(first.stream) == [(0, 20, 0, 0, 0, 0, 0, 0, 0)]           # a capacity of 0 is an absent arc
    assert first.stats == dict(nodes=1, pus=0, slots=0, sink_arcs=0, arcs_added=0, cap_updates=0, arcs_skipped=2,
                               records=1)
    assert first.arcs == TOY_ARCS and first.S == {}
    g = table_graph(first.ntype, first.supply, first.arcs)
    second = grow_reference(g, [(21, 4, 0, 0), (22, 2, 2, 0)], [(21, 22, 0, TREE), (20, 21, 4, TREE), (X, 20, 3, TREE)])
    assert stream_rows(second.stream)[3:] == [(2, 0, 21, 22, 0, 2, 0, 0, 0), (2, 0, 20, 21, 0, 2, 4, 0, 0),
                                              (2, 0, 2, 20, 0, 2, 3, 0, 0)]      # the chain edge creates X → rack now
    assert second.stats["arcs_added"] == 3 and second.stats["cap_updates"] == 0
    none = grow_reference(toy(), [], [])
    assert none.stream.shape[0] == 0 and none.arcs == TOY_ARCS and not any(none.stats.values())
    only_chain = grow_reference(toy(), [], [(X, R1, 0, TREE), (R1, M1, 0, TREE)])
    assert only_chain.stream.shape[0] == 0 and only_chain.stats["arcs_skipped"] == 2


def test_toy_id_reuse_and_ids_beyond():
    alive = set(range(1, 20)) - {M1, P1}
    arcs = {k: a for k, a in TOY_ARCS.items() if M1 not in k and P1 not in k}
    r = grow_reference(toy(arcs), [(P1, 4, 0, 0), (M1, 2, 3, 0), (50, 2, 1, 0)],
                       [(P1, M1, 0, TREE), (R1, P1, 0, TREE), (P1, 50, 0, TREE), (X, R1, 0, TREE)], alive=alive)
    assert r.ntype[M1 - 1] == 2 and r.ntype[P1 - 1] == 4 and len(r.ntype) == 50   # the ids swap their roles
    assert r.arcs[(R1, P1)] == (0, 4, 0, 0) and r.arcs[(X, R1)] == (0, 8, 0, 0) and r.arcs[(M1, SINK)] == (0, 3, 0, 0)
    assert r.alive == alive | {M1, P1, 50}


def test_depths():
    def tower(depth):
        """A PU under depth − 1 new intermediate nodes under R1: depth tree edges up to R1, one more to X."""
        ids = list(range(100, 100 + depth))
        nodes = [(ids[0], 2, 1, 0)] + [(i, 5, 0, 0) for i in ids[1:]]
        edges = [(ids[k + 1], ids[k], 0, TREE) for k in range(depth - 1)] + [(R1, ids[-1], 0, TREE), (X, R1, 0, TREE)]
        return nodes, edges
    for depth in (1, 6, 31):                                                     # 2, 7 and 32 edges above the PU
        r = grow_reference(toy(), *tower(depth))
        assert r.arcs[(X, R1)][1] == 5 and r.stats["arcs_added"] == depth
    with pytest.raises(InvalidGrowth) as e:
        grow_reference(toy(), *tower(32))                                        # 33 edges
    assert e.value.args == (100, "depth")
    nodes, edges = tower(32)
    assert grow_reference(toy(), nodes, edges[:-1]).stats["arcs_added"] == 32    # 32 edges: the last legal depth
    with pytest.raises(InvalidGrowth) as e:                                      # a cycle among new nodes
        grow_reference(toy(), [(20, 4, 0, 0), (21, 4, 0, 0), (22, 2, 1, 0), (23, 2, 1, 0)],
                       [(20, 21, 0, TREE), (21, 20, 0, TREE), (R1, 23, 0, TREE), (20, 22, 0, TREE)])
    assert e.value.args == (22, "depth")


def test_refusals_of_the_rule():
    mach = (20, 4, 0, 0)
    for bad, err in ((0, OutOfRange), (1 << 30, OutOfRange), (14, InvalidGrowth), (M1, InvalidGrowth)):
        with pytest.raises(err) as e:
            grow_reference(toy(), [mach, (bad, 4, 0, 0), (0, 4, 0, 0)], [])
        assert e.value.args[0] == bad                                            # the first offending id is named
    with pytest.raises(InvalidGrowth) as e:
        grow_reference(toy(), [mach, (21, 4, 0, 0), mach], [])                   # listed twice: already present
    assert e.value.args == (20, "present")
    for ty in (1, 3, 6, -1):
        with pytest.raises(InvalidGrowth) as e:
            grow_reference(toy(), [mach, (21, ty, 0, 0)], [])
        assert e.value.args == (21, "type")
    for node in ((21, 2, 0, 0), (21, 4, 1, 0), (21, 0, 0, 5)):
        with pytest.raises(InvalidGrowth) as e:
            grow_reference(toy(), [mach, node], [])
        assert e.value.args == (21, "values")
    for node in ((21, 2, (1 << 53) + 1, 0), (21, 2, 1, (1 << 40) + 1), (21, 2, 1, -(1 << 40) - 1)):
        with pytest.raises(OutOfRange) as e:
            grow_reference(toy(), [mach, node], [])
        assert e.value.args[0] == 21
    with pytest.raises(OutOfRange) as e:                                         # the slots summed
        grow_reference(toy(), [(21, 2, 1 << 53, 0), (22, 2, 1, 0)], [])
    assert e.value.args[0] == 22
    assert grow_reference(toy(), [(21, 2, 1 << 53, 1 << 40)], []).stats["slots"] == 1 << 53
    two = table_graph(TOY_NTYPE + [3], TOY_SUPPLY + [0], TOY_ARCS)
    with pytest.raises(InvalidGrowth) as e:
        grow_reference(two, [(21, 2, 1, 0)], [])                                 # a PU needs exactly one sink
    assert e.value.args == (None, "sink")
    assert grow_reference(two, [(21, 4, 0, 0)], [(R1, 21, 0, TREE)]).stats["records"] == 1
    alive = set(range(1, 20)) - {15}
    pu = (21, 2, 1, 0)
    ok = (R1, 20, 0, TREE)
    for p in (0, 15, 14, SINK, P1, 21, 40):                                      # 0, dead, a task, the sink, a PU (live,
        with pytest.raises(InvalidGrowth) as e:                                  # new), beyond the graph
            grow_reference(toy(), [mach, pu], [ok, (p, 20, 0, TREE), (0, 0, 0, 9)], alive=alive)
        assert e.value.args == ((p, 20), "parent")
    for c in (0, 15, 14, SINK, 40):
        with pytest.raises(InvalidGrowth) as e:
            grow_reference(toy(), [mach, pu], [ok, (20, c, 1 << 41, 9)], alive=alive)
        assert e.value.args == ((20, c), "child")                                # the endpoints come before the cost
    for edge, what in (((20, 20, 0, TREE), "loop"), ((20, 21, 0, 2), "kind"), ((20, 21, 0, -1), "kind"),
                       ((20, M1, 0, TREE), "moves"), ((R1, 20, 0, EXTRA), "pair"), ((R2, 20, 0, TREE), "second parent")):
        with pytest.raises(InvalidGrowth) as e:
            grow_reference(toy(), [mach, pu], [ok, edge, (0, 0, 0, 0)])
        assert e.value.args == (edge[:2], what)
    assert grow_reference(toy(), [mach, pu], [ok, (20, M1, 0, EXTRA)]).stats["arcs_skipped"] == 2   # EXTRA moves nothing
    for cost in ((1 << 40) + 1, -(1 << 40) - 1):
        with pytest.raises(OutOfRange) as e:
            grow_reference(toy(), [mach, pu], [ok, (20, 21, cost, TREE)])
        assert e.value.args[0] == (20, 21)
    assert grow_reference(toy(), [mach, pu], [ok, (20, 21, -(1 << 40), TREE)]).arcs[(20, 21)] == (0, 1, -(1 << 40), 0)
    arcs = dict(TOY_ARCS)
    arcs[(X, R1)] = (0, 1 << 53, 0, 0)
    with pytest.raises(OutOfRange) as e:                                         # a raised capacity beyond 2^53
        grow_reference(toy(arcs), [mach, pu], [ok, (20, 21, 0, TREE), (X, R1, 0, TREE)])
    assert e.value.args[0] == (X, R1)


# ---- against the store semantics ----------------------------------------------------
CASES = [([(20, 4, 0, 0), (21, 2, 2, 7)], [(R1, 20, 5, TREE), (20, 21, 6, TREE), (X, R1, 9, TREE)]),
         ([(40, 2, 4, 0)], [(M1, 40, 15, TREE), (R1, M1, 16, TREE), (X, R1, 17, TREE)]),
         ([(30, 0, 0, 0), (31, 4, 0, 0), (33, 2, 3, 1)], [(31, 33, 0, TREE), (30, 31, 1, TREE), (X, 30, 2, TREE),
                                                          (R2, 31, 3, EXTRA)]),
         ([(25, 0, 0, 0)], [(X, 25, 3, TREE)])]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("lost", [False, True], ids=["held", "lost"])
def test_the_stream_reproduces_the_table(case, lost):
    """The returned records through the store's semantics give the returned table."""
    arcs = dict(TOY_ARCS)
    if lost:
        del arcs[(R1, M1)]
    nodes_in, edges = CASES[case]
    r = grow_reference(toy(arcs), nodes_in, edges)
    nodes = {i + 1: [TOY_SUPPLY[i], TOY_NTYPE[i]] for i in range(len(TOY_NTYPE))}
    low3 = {k: a[:3] for k, a in arcs.items()}
    apply_deltas_to_arcs(nodes, low3, r.stream)
    assert low3 == {k: a[:3] for k, a in r.arcs.items()}
    assert set(nodes) == r.alive and all(nodes[i] == [0, ty] for i, ty, _, _ in nodes_in)
    n = len(nodes_in)
    assert [int(x["id"]) for x in r.stream[:n]] == [x[0] for x in nodes_in]     # the fixed positions
    pus = [x[0] for x in nodes_in if x[1] == 2]
    assert r.stream["src"][n:n + len(pus)].tolist() == pus and set(r.stream["dst"][n:n + len(pus)].tolist()) <= {SINK}
    keys = list(zip(r.stream["src"][n:].tolist(), r.stream["dst"][n:].tolist()))
    assert len(set(keys)) == len(keys)                                           # no (src, dst) twice
    assert r.stats["records"] == r.stream.shape[0] == sum(r.stats[f] for f in ("nodes", "sink_arcs", "arcs_added",
                                                                                 "cap_updates"))
    assert r.stats["arcs_added"] + r.stats["cap_updates"] + r.stats["arcs_skipped"] == len(edges)


# ---- the round trip with ks_remove_resources' rule -----------------------------------
def pinned_toy():
    """The toy under the pinned rule's capacities (slots − running): the refresh of the loaded table."""
    table, n = refreshed(toy(), False)
    assert n == 8 and (M1, P1) not in table                                      # M1 is full: its arcs left
    return table


@pytest.mark.parametrize("preemptive", [True, False], ids=["preemptive", "pinned"])
def test_a_machine_removed_and_added_back(preemptive):
    """remove_ref takes a machine's subtree out with the resource capacities; the rule adds it
    back with its chain. Every resource arc is as it was; only the task arcs into the removed
    nodes are missing. Preemptive: M1 (its two tasks are evicted). Pinned: M4, which runs nothing
    (a machine that joins runs nothing, so a full one cannot come back as it was)."""
    before = dict(TOY_ARCS) if preemptive else pinned_toy()
    mach, pu = (M1, P1) if preemptive else (M4, P4)
    g = table_graph(TOY_NTYPE, TOY_SUPPLY, before)
    rm = remove_reference(g, [mach], TOY_BINDINGS, True, preemptive)
    assert rm.removed == [mach, pu]
    alive = set(range(1, 20)) - {mach, pu}
    parents = tree_parents(TOY_NTYPE, before)
    costs = {k: a[2] for k, a in before.items()}
    nodes = [(mach, 4, 0, 0), (pu, 2, before[(pu, SINK)][1], before[(pu, SINK)][2])]
    edges = [(mach, pu, 0, TREE)] + chain(parents, mach, costs)
    back = grow_reference(table_graph(TOY_NTYPE, TOY_SUPPLY, rm.arcs), nodes, edges, alive=alive)
    task_arcs = {k for k in before if TOY_NTYPE[k[0] - 1] == 1 and (k[1] in (mach, pu))}
    assert task_arcs and back.arcs == {k: a for k, a in before.items() if k not in task_arcs}
    assert back.alive == set(range(1, 20))
    assert refreshed(table_graph(back.ntype, back.supply, back.arcs), preemptive)[1] == 0


def test_a_quincy_machine_removed_and_added_back():
    g = gen.quincy(40, 6, 2, 3, 11)
    before = arc_table(g)
    ntype = g.ntype.tolist()
    mach, pu = 3 + 2 + 4, 3 + 2 + 6 + 4                                          # machine 4 and its PU
    parents = tree_parents(ntype, before)
    assert parents[pu] == mach
    for preemptive in (False, True):
        rm = remove_reference(g, [mach], {}, True, preemptive)
        assert rm.removed == [mach, pu]
        nodes = [(mach, 4, 0, 0), (pu, 2, before[(pu, 1)][1], 0)]
        edges = [(mach, pu, 0, TREE)] + chain(parents, mach)
        alive = set(range(1, g.n + 1)) - {mach, pu}
        back = grow_reference(table_graph(g.ntype, g.supply, rm.arcs), nodes, edges, alive=alive)
        lost = {k for k in before if k[1] == mach and ntype[k[0] - 1] == 1}
        assert lost and back.arcs == {k: a for k, a in before.items() if k not in lost}
        assert back.stats["cap_updates"] == 1 and back.stats["arcs_added"] == 2


# ---- the independent check: the capacity refresh has nothing to write ------------------
def growth_cases(ntype, table, top, extra=()):
    """Legal calls with full chains on a graph table: [(nodes, edges)]. A machine with a PU under
    an existing rack (or the root); a lone PU under an existing machine; a rack with two machines."""
    parents = tree_parents(ntype, table, extra)
    machines = [i + 1 for i, t in enumerate(ntype) if t == 4]
    m0 = machines[0]
    rack = parents[m0]
    root = rack
    while root in parents:
        root = parents[root]
    a, b, c, d, e = range(top + 1, top + 6)
    ex = [(x, a, 0, EXTRA) for x in extra]
    return [([(a, 4, 0, 0), (b, 2, 3, 0)], [(rack, a, 0, TREE), (a, b, 0, TREE)] + ex + chain(parents, rack)),
            ([(a, 2, 2, 0)], [(m0, a, 0, TREE)] + chain(parents, m0) + [(x, m0, 0, EXTRA) for x in extra]),
            ([(a, 0, 0, 0), (b, 4, 0, 0), (c, 4, 0, 0), (d, 2, 1, 0), (e, 2, 4, 0)],
             [(root, a, 0, TREE), (a, b, 0, TREE), (a, c, 0, TREE), (b, d, 0, TREE), (c, e, 0, TREE)])]


@pytest.mark.parametrize("preemptive", [False, True], ids=["pinned", "preemptive"])
@pytest.mark.parametrize("name", ["toy", "quincy", "trivial"])
def test_after_a_call_with_full_chains_the_refresh_writes_nothing(name, preemptive):
    """On a graph whose capacities are consistent, complete_ref with no task and the resource
    capacities generates no record after the call: its sums (a BFS from the sink, not the
    tree walk of this rule) agree with every capacity the rule wrote."""
    extra = ()
    if name == "toy":
        g = toy()
    elif name == "quincy":
        g = gen.quincy(40, 6, 2, 3, 5)
    else:
        g = gen.trivial(4, 3, 6)                  # the coordinator's arcs are built with capacity 0: refresh first
        extra = (3 + 2 * 4 + 1,)                  # the equivalence class: its arcs into machines are EXTRA
    table, n = refreshed(g, preemptive)
    if name == "trivial":
        assert n == 4
    if name == "toy":                             # pinned: M1 is full, the store lost R1 → M1 and the call re-creates it
        assert (n == 0 and (R1, M1) in table) if preemptive else (n == 8 and (R1, M1) not in table)
    ntype, supply = g.ntype.tolist(), g.supply.tolist()
    for nodes, edges in growth_cases(ntype, arc_table(g), g.n, extra):
        r = grow_reference(table_graph(ntype, supply, table), nodes, edges)
        assert r.stats["pus"] >= 1 and r.stats["arcs_added"] + r.stats["cap_updates"] >= 2
        after, writes = refreshed(table_graph(r.ntype, r.supply, r.arcs), preemptive)
        assert writes == 0 and after == r.arcs, (nodes, edges)
    # a chain cut short leaves the arcs above it one subtree short: the refresh repairs it (on a
    # machine whose arcs the store holds; arcs that fell to 0 need the pinned recipe first)
    last = max(i + 1 for i, t in enumerate(ntype) if t == 4)
    r = grow_reference(table_graph(ntype, supply, table), [(g.n + 1, 2, 2, 0)], [(last, g.n + 1, 0, TREE)])
    assert refreshed(table_graph(r.ntype, r.supply, r.arcs), preemptive)[1] > 0


# ---- the library and the binding ------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_grow_stats %zu\nks_res_node %zu\nks_res_arc %zu\n", sizeof(ks_grow_stats), sizeof(ks_res_node),
         sizeof(ks_res_arc));
  P(ks_res_node, id); P(ks_res_node, type); P(ks_res_node, slots); P(ks_res_node, sink_cost);
  P(ks_res_arc, parent); P(ks_res_arc, child); P(ks_res_arc, cost); P(ks_res_arc, kind);
""" + "".join(f"  P(ks_grow_stats, {f});\n" for f in STAT_KEYS + ("reserved",)) + r"""
  printf("abi %d\ntree %d\nextra %d\ndepth %d\n", KSMCMF_ABI_VERSION, KS_RES_TREE, KS_RES_EXTRA, KS_RES_MAX_DEPTH);
  return 0;
}
"""


def test_grow_structs_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_grow_stats"] == C.sizeof(native.KsGrowStats) == 96
    assert out["ks_res_node"] == native.RES_NODE_DT.itemsize == 32
    assert out["ks_res_arc"] == native.RES_ARC_DT.itemsize == 32
    for dt, cname in ((native.RES_NODE_DT, "ks_res_node"), (native.RES_ARC_DT, "ks_res_arc")):
        for f in dt.names:
            assert dt.fields[f][1] == out[f"{cname}.{f}"], (cname, f)
    assert [f for f, _ in native.KsGrowStats._fields_] == list(STAT_KEYS) + ["reserved"]
    for f in STAT_KEYS + ("reserved",):
        assert getattr(native.KsGrowStats, f).offset == out[f"ks_grow_stats.{f}"], f
    assert tuple(native.KsGrowStats().as_dict()) == STAT_KEYS
    assert (out["tree"], out["extra"], out["depth"]) == (native.KS_RES_TREE, native.KS_RES_EXTRA,
                                                          native.KS_RES_MAX_DEPTH) == (TREE, EXTRA, 32)
    assert out["abi"] == native.ABI_VERSION == 5          # an entry point and three structs were added, nothing moved


def test_library_exports_the_entry_point():
    """Fails on a library built before ks_add_resources."""
    lib = native.load(build_if_missing=True)
    assert "ks_add_resources" in native.EXPORTED_SYMBOLS
    assert hasattr(lib, "ks_add_resources")
    assert lib.ks_abi_version() == 5


def test_binding_has_add_resources():
    assert callable(getattr(native.Context, "add_resources", None))
    assert Growth._fields == ("arcs", "ntype", "supply", "alive", "stream", "stats", "S")
