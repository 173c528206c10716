"""CPU: the restatement of ks_update_nodes (tests/nodes_ref.py) checked by hand on the 19-node
toy, against the store semantics (graphs.apply_deltas_to_arcs) on the toy and on a churn-model
graph after a few of its rounds, every refusal of the rule with its ranking, and the library's
and the binding's new entry point with the layout of its structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from commit_ref import arc_table
from graphs import apply_deltas_to_arcs
from ksched_amd import churn, native
from ksched_amd.native import KS_CAP_KEEP, KS_NODES_KEEP_UNLISTED, NODE_ARC_DT, KsNodeStats   # (the binding under test)
from nodes_ref import (CAP_KEEP, KEEP_UNLISTED, STAT_KEYS, InvalidNodes, NodeRefresh, OutOfRange, nodes_reference,
                       offsets3)
from oracle import ko
from preempt_ref import table_graph
from remove_ref import TOY_ARCS, TOY_NTYPE, TOY_SUPPLY, TOY_U, BelowLowerBound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINK, X, R1, R2, M1, M2, M3, M4, P1, U = 1, 2, 3, 4, 5, 6, 7, 8, 9, TOY_U
# the toy with two class → machine arcs behind everything else in the table: X holds four arcs
WIDE = {**TOY_ARCS, (X, M1): (0, 2, 7, 0), (X, M2): (0, 2, 8, 0)}


def refresh(nodes, lists, arcs=None, **kw) -> NodeRefresh:
    return nodes_reference(TOY_NTYPE, TOY_ARCS if arcs is None else arcs, nodes, lists, **kw)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]), int(x["cost"]),
             int(x["old_cost"]), int(x["type"])) for x in stream]


def stats(**kw) -> dict:
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(kw)
    return st


# ---- the rule by hand ------------------------------------------------------------------
# X: R1 another cost, R2 another capacity, M1 as it is, M3 a new head, M4 skipped (cap 0), M2 zeroed
MIXED = [(R1, 5, 4), (R2, 0, 3), (M1, 7, 2), (M3, 1, 2), (M4, 1, 0), (M2, 8, 0)]


def test_toy_one_class_list_hits_six_rows_of_the_table():
    r = refresh([X], [MIXED], arcs=WIDE)
    assert stream_rows(r.stream) == [
        (3, X, R1, 0, 4, 5, 0, 0),     # ChangeArc: the cost moves, old_cost the cost it had
        (3, X, R2, 0, 3, 0, 0, 0),     # ChangeArc: the capacity moves
        (3, X, M2, 0, 0, 8, 8, 0),     # zeroed: UPDATE_ARC 0/0, the cost it had in both words
        (2, X, M3, 0, 2, 1, 0, 0),     # AddArc(0, cap, cost), type 0
    ]
    assert r.stats == stats(nodes=1, arcs_added=1, arcs_updated=2, arcs_unchanged=1, arcs_skipped=1, arcs_zeroed=1,
                            records=4)
    want = dict(WIDE)
    del want[(X, M2)]
    want.update({(X, R1): (0, 4, 5, 0), (X, R2): (0, 3, 0, 0), (X, M3): (0, 2, 1, 0)})
    assert r.arcs == want and (X, M4) not in r.arcs
    assert r.stats["records"] == sum(r.stats[f] for f in ("arcs_added", "arcs_updated", "arcs_zeroed", "arcs_removed"))


def test_toy_an_unlisted_class_arc_is_deleted_and_kept_under_the_flag():
    r = refresh([X], [[(R1, 0, 4)]])
    assert stream_rows(r.stream) == [(3, X, R2, 0, 0, 0, 0, 0)]
    assert r.stats == stats(nodes=1, arcs_unchanged=1, arcs_removed=1, records=1) and (X, R2) not in r.arcs
    r = refresh([X], [[(R1, 0, 4)]], flags=KEEP_UNLISTED)
    assert r.stream.shape[0] == 0 and r.arcs == TOY_ARCS and r.stats == stats(nodes=1, arcs_unchanged=1)


def test_toy_an_empty_list_keeps_the_arc_into_the_sink():
    """U's only out-arc ends at the sink: "no preferences" drops nothing of it; X loses both."""
    r = refresh([U], [[]])
    assert r.stream.shape[0] == 0 and r.arcs == TOY_ARCS and r.stats == stats(nodes=1)
    r = refresh([U, X], [[], []])
    assert stream_rows(r.stream) == [(3, X, R1, 0, 0, 0, 0, 0), (3, X, R2, 0, 0, 0, 0, 0)]
    assert r.arcs[(U, SINK)] == TOY_ARCS[(U, SINK)] and r.stats == stats(nodes=2, arcs_removed=2, records=2)


def test_toy_a_resource_tail_never_loses_an_arc():
    """M1 listed without its PU keeps M1 → P1, and P1 keeps its arc into the sink
    (updateResOutgoingArcs deletes nothing). The toy's racks are type 0: R1 is a class and loses
    what its list does not name."""
    r = refresh([M1], [[]])
    assert r.stream.shape[0] == 0 and r.arcs[(M1, P1)] == TOY_ARCS[(M1, P1)] and r.stats == stats(nodes=1)
    r = refresh([M1, P1], [[(P1, 3, CAP_KEEP)], []])
    assert stream_rows(r.stream) == [(3, M1, P1, 0, 2, 3, 0, 0)] and r.arcs[(P1, SINK)] == TOY_ARCS[(P1, SINK)]
    r = refresh([R1], [[(M1, 0, 2)]])                              # a type-0 rack is a class: M2 is dropped
    assert stream_rows(r.stream) == [(3, R1, M2, 0, 0, 0, 0, 0)]


def test_toy_cap_keep_on_a_held_and_on_an_absent_arc():
    r = refresh([X, P1], [[(R1, 9, CAP_KEEP), (R2, 0, CAP_KEEP)], [(SINK, 4, CAP_KEEP)]])
    assert stream_rows(r.stream) == [(3, X, R1, 0, 4, 9, 0, 0), (3, P1, SINK, 0, 2, 4, 0, 0)]
    assert r.stats == stats(nodes=2, arcs_updated=2, arcs_unchanged=1, records=2)
    with pytest.raises(InvalidNodes) as e:
        refresh([X], [[(R1, 9, CAP_KEEP), (M3, 1, CAP_KEEP)]])
    assert e.value.args == (X, M3)


def test_toy_a_capacity_below_a_lower_bound_of_one():
    arcs = {**TOY_ARCS, (X, R1): (1, 4, 0, 0), (P1, SINK): (1, 2, 0, 0)}
    for lst, tail, head in (([(R2, 0, 4), (R1, 0, 0)], X, R1), ([(SINK, 0, 0)], P1, SINK)):
        with pytest.raises(BelowLowerBound) as e:
            refresh([tail], [lst], arcs=arcs)
        assert e.value.args == (tail, head)
    r = refresh([X, P1], [[(R1, 0, 1), (R2, 0, 4)], [(SINK, 0, 3)]], arcs=arcs)     # at the bound: legal, low kept
    assert stream_rows(r.stream) == [(3, X, R1, 1, 1, 0, 0, 0), (3, P1, SINK, 1, 3, 0, 0, 0)]
    none = refresh([], [])
    assert none.stream.shape[0] == 0 and none.arcs == TOY_ARCS and not any(none.stats.values())


def test_toy_held_records_by_arc_slot_then_the_additions_in_input_order():
    tails = [P1, R1, X, M1]
    lists = [[(SINK, 1, 3)], [(M3, 2, 1), (M1, 5, 2)], [(M4, 1, 1), (R2, 3, 4)], [(P1, 1, CAP_KEEP), (10, 4, 1)]]
    r = refresh(tails, lists)
    rows = stream_rows(r.stream)
    slot = {k: i for i, k in enumerate(TOY_ARCS)}
    held = [(s, d) for kind, s, d, *_ in rows if kind == 3]
    assert held == sorted(held, key=slot.get) == [(X, R1), (X, R2), (R1, M1), (R1, M2), (M1, P1), (P1, SINK)]
    assert [(s, d) for kind, s, d, *_ in rows[len(held):]] == [(R1, M3), (X, M4), (M1, 10)]
    assert all(kind == 2 for kind, *_ in rows[len(held):])


# ---- the stream against the store semantics ---------------------------------------------
def replay(ntype, supply, alive, before: dict, r: NodeRefresh):
    nodes = {i: [int(supply[i - 1]), int(ntype[i - 1])] for i in alive}
    low3 = {k: a[:3] for k, a in before.items()}
    apply_deltas_to_arcs(nodes, low3, r.stream)
    assert low3 == {k: a[:3] for k, a in r.arcs.items()}
    pairs = list(zip(r.stream["src"].tolist(), r.stream["dst"].tolist()))
    assert len(pairs) == len(set(pairs))            # nothing is superseded


@pytest.mark.parametrize("case", range(4))
def test_the_stream_reproduces_the_table_on_the_toy(case):
    nodes, lists, kw = [([X], [MIXED], {}), ([X, M1], [MIXED, []], dict(flags=KEEP_UNLISTED)),
                        ([U, P1, R1], [[], [(SINK, 2, 1)], [(M2, 4, 1), (M4, 0, 2)]], {}),
                        ([X, R2], [[], [(M3, 1, CAP_KEEP)]], {})][case]
    r = refresh(nodes, lists, arcs=WIDE, **kw)
    replay(TOY_NTYPE, TOY_SUPPLY, range(1, 20), WIDE, r)
    assert r.stats["records"] == r.stream.shape[0] > 0


def test_the_stream_reproduces_the_table_on_a_churn_graph():
    """Three rounds of a small cell; then every node with an out-arc that is no task is listed:
    the classes with a cost per arc (their position), one head dropped and one new machine head,
    the machines and PUs with their arcs re-costed at the held capacity. The oracle finds the
    result feasible."""
    cell = churn.Cell(40, 8, 2, 6, 3)
    for rnd in range(3):
        g = cell.graph()
        st, _, _, fl = ko.cost_scaling(g)
        assert st == 0
        cell.step(ko.bfs_mapping(g, fl), 6, 8, age_cost=0, seed=100 + rnd)
    g = cell.graph()
    before = {k: a for k, a in arc_table(g).items() if a[1] > 0}
    alive = {i + 1 for i in range(g.n) if i + 1 < cell.TASK0 or g.ntype[i] == 1}
    tails = sorted({s for (s, d) in before if g.ntype[s - 1] in (0, 2, 4, 5) and s < cell.U0})
    lists = []
    for u in tails:
        mine = [(d, a) for (s, d), a in before.items() if s == u]
        if g.ntype[u - 1] == 0:
            lst = [(d, a[2] + j, a[1] + (j % 2)) for j, (d, a) in enumerate(mine)][1:]
            new = next(m for m in range(cell.MACH0, cell.MACH0 + cell.M) if m not in dict(mine) and m != u)
            lst.append((new, 11, 2))
        else:
            lst = [(d, a[2] + 3, CAP_KEEP) for d, a in mine]
        lists.append(lst)
    r = nodes_reference(g.ntype, before, tails, lists)
    replay(g.ntype, g.supply, alive, before, r)
    assert r.stats["arcs_updated"] > cell.M and r.stats["arcs_removed"] > 0 and r.stats["arcs_added"] > 0
    assert ko.cost_scaling(table_graph(g.ntype, g.supply, r.arcs))[0] == 0


# ---- refusals ---------------------------------------------------------------------------
def test_refusals_of_the_rule_change_nothing_and_rank_as_the_contract_says():
    table = dict(TOY_ARCS)
    alive = set(range(1, 20)) - {8, 12}                                       # M4 and P4 are dead
    one = [(R1, 0, 4)]
    BIG = (1 << 40) + 1

    def refused(err, names, nodes, lists, **kw):
        with pytest.raises(err) as e:
            refresh(nodes, lists, arcs=table, alive=alive, **kw)
        assert e.value.args[:len(names)] == tuple(names)
        assert table == TOY_ARCS and list(table) == list(TOY_ARCS)

    for bad in (0, 8, 14, SINK, 40):                                          # 0, dead, a task, a sink, beyond the graph
        refused(InvalidNodes, [bad], [X, bad, 0], [one, [], []])
    refused(InvalidNodes, [X], [X, R1, X, 0], [one, [], one, []])             # listed a second time
    for head in (0, 8, 14, 40, R1):                                           # 0, dead, a task, beyond, the tail itself
        refused(InvalidNodes, [R1, head], [X, R1], [one, [(M1, 0, 2), (head, BIG, 1 << 60)]])   # the head comes first
    refused(InvalidNodes, [P1, M1], [X, P1], [one, [(M1, 0, 1)]])             # a PU's only head is a sink
    refused(InvalidNodes, [M1, SINK], [X, M1], [one, [(SINK, 0, 1)]])         # a machine has no arc into a sink
    assert refresh([U, P1], [[(SINK, 1, 6)], [(SINK, 1, 2)]], arcs=table, alive=alive).stats["arcs_updated"] == 2
    refused(InvalidNodes, [R1, M1], [X, R1], [one, [(M1, 0, 2), (M2, 0, 2), (M1, BIG, 2)]])   # a held head twice, before its cost
    refused(InvalidNodes, [R1, M3], [X, R1], [one, [(M3, 0, 2), (M2, 0, 2), (M3, 0, 2)]])     # an absent head twice
    refused(OutOfRange, [R1, M1], [X, R1], [one, [(M1, BIG, 1 << 60)]])       # the cost before the capacity
    refused(OutOfRange, [R1, M1], [X, R1], [one, [(M1, -BIG, 2)]])
    refused(OutOfRange, [R1, M2], [X, R1], [one, [(M1, 0, 2), (M2, 0, (1 << 53) + 1)]])
    refused(OutOfRange, [X, R1], [X, R1], [[(R1, 0, CAP_KEEP - 1)], [(0, 0, 0)]])             # the first arc in input order
    ok = refresh([R1], [[(M1, 1 << 40, 1 << 53), (M2, -(1 << 40), CAP_KEEP)]], arcs=table, alive=alive)
    assert ok.stats["arcs_updated"] == 2                                      # the bounds themselves are legal
    # the arcs' form is checked on every arc before the store is asked about any
    refused(OutOfRange, [R1, M2], [X, R1], [[(M3, 0, CAP_KEEP)], [(M2, BIG, 2)]])
    refused(InvalidNodes, [X, M3], [X, R1], [[(M3, 0, CAP_KEEP)], [(M2, 0, 2)]])              # nothing to keep
    low = {**TOY_ARCS, (R1, M1): (2, 2, 0, 0)}
    with pytest.raises(BelowLowerBound) as e:                                 # the first in input order of the two
        nodes_reference(TOY_NTYPE, low, [R1, X], [[(M1, 0, 1)], [(M3, 0, CAP_KEEP)]])
    assert e.value.args == (R1, M1)
    with pytest.raises(InvalidNodes) as e:
        nodes_reference(TOY_NTYPE, low, [X, R1], [[(M3, 0, CAP_KEEP)], [(M1, 0, 1)]])
    assert e.value.args == (X, M3)
    refused(InvalidNodes, [None], [X], [one], flags=2)
    refused(InvalidNodes, [None], [X], [one], flags=KEEP_UNLISTED | 4)


def test_offsets3_is_the_abi_form():
    off, dst, cost, cap = offsets3([[(3, -1, 4)], [], [(5, 2, CAP_KEEP), (6, 0, 0)]])
    assert off.tolist() == [0, 1, 1, 3] and dst.tolist() == [3, 5, 6] and cost.tolist() == [-1, 2, 0]
    assert cap.tolist() == [4, CAP_KEEP, 0] and cap.dtype == np.uint64


# ---- the library and the binding ----------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_node_stats %zu\n", sizeof(ks_node_stats));
  printf("ks_node_arc %zu\n", sizeof(ks_node_arc));
  P(ks_node_arc, dst); P(ks_node_arc, cost); P(ks_node_arc, cap);
""" + "".join(f"  P(ks_node_stats, {f});\n" for f in STAT_KEYS + ("reserved",)) + r"""
  printf("abi %d\n", KSMCMF_ABI_VERSION);
  printf("keep %d\n", KS_NODES_KEEP_UNLISTED);
  printf("capkeep %d\n", KS_CAP_KEEP == UINT64_MAX);
  return 0;
}
"""


def test_node_structs_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_node_stats"] == C.sizeof(KsNodeStats) == 96
    assert out["ks_node_arc"] == NODE_ARC_DT.itemsize == 24
    for f in ("dst", "cost", "cap"):
        assert NODE_ARC_DT.fields[f][1] == out[f"ks_node_arc.{f}"]
    assert [f for f, _ in native.KsNodeStats._fields_] == list(STAT_KEYS) + ["reserved"]
    for f in STAT_KEYS + ("reserved",):
        assert getattr(native.KsNodeStats, f).offset == out[f"ks_node_stats.{f}"], f
    assert tuple(native.KsNodeStats().as_dict()) == STAT_KEYS
    assert out["keep"] == KS_NODES_KEEP_UNLISTED == KEEP_UNLISTED == 1
    assert out["capkeep"] == 1 and KS_CAP_KEEP == CAP_KEEP == 2 ** 64 - 1
    assert out["abi"] == native.ABI_VERSION == 5          # an entry point and two structs were added, nothing moved


def test_library_exports_the_entry_point():
    """Fails on a library built before ks_update_nodes."""
    lib = native.load(build_if_missing=True)
    assert "ks_update_nodes" in native.EXPORTED_SYMBOLS
    assert hasattr(lib, "ks_update_nodes")
    assert lib.ks_abi_version() == 5
    assert lib.ks_update_nodes(None, 0, None, 0, None, None, None) == native.KS_E_INVALID    # a null context


def test_binding_has_update_nodes():
    assert callable(getattr(native.Context, "update_nodes", None))
    assert NodeRefresh._fields == ("arcs", "stream", "stats")
