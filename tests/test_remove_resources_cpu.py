"""CPU: the restatement of ks_remove_resources (tests/remove_ref.py) checked by hand on a
toy, against the store semantics (graphs.apply_deltas_to_arcs), and the library's and
the binding's new entry point."""
import ctypes

import pytest

from graphs import apply_deltas_to_arcs
from ksched_amd import native
from preempt_ref import table_graph
from remove_ref import (TOY_ARCS, TOY_BINDINGS, TOY_M1, TOY_NTYPE, TOY_R1, TOY_SUPPLY, TOY_U, BelowLowerBound,
                        InvalidRoot, remove_reference)


def toy():
    return table_graph(TOY_NTYPE, TOY_SUPPLY, TOY_ARCS)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["id"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]),
             int(x["cost"]), int(x["type"])) for x in stream]


GONE_WITH_M1 = {(3, 5), (5, 9), (9, 1), (14, 5), (18, 5), (14, 9), (15, 9)}


def test_toy_one_machine_pinned_rule():
    """M1 (5) leaves with its PU (9); T1 and T2 ran there. Slots − running below: P2 and
    P3 run one task each, so M2 → P2, M3 → P3, R1 → M2 and R2 → M3 drop to 1, X → R1 to
    2 − 1 and X → R2 to 4 − 1."""
    r = remove_reference(toy(), [TOY_M1], TOY_BINDINGS, True, False)
    assert r.removed == [5, 9]
    assert r.evicted == [(14, 9), (15, 9)]
    assert r.bindings == {16: 10, 17: 11}
    want = {k: a for k, a in TOY_ARCS.items() if k not in GONE_WITH_M1}
    want.update({(6, 10): (0, 1, 0, 0), (7, 11): (0, 1, 0, 0), (3, 6): (0, 1, 0, 0), (4, 7): (0, 1, 0, 0),
                 (2, 3): (0, 1, 0, 0), (2, 4): (0, 3, 0, 0)})
    assert r.arcs == want
    assert r.arcs[(8, 12)] == r.arcs[(4, 8)] == (0, 2, 0, 0)
    assert stream_rows(r.stream) == [(1, 5, 0, 0, 0, 0, 0, 0), (1, 9, 0, 0, 0, 0, 0, 0),
                                     (3, 0, 2, 3, 0, 1, 0, 0), (3, 0, 2, 4, 0, 3, 0, 0),
                                     (3, 0, 3, 6, 0, 1, 0, 0), (3, 0, 4, 7, 0, 1, 0, 0),
                                     (3, 0, 6, 10, 0, 1, 0, 0), (3, 0, 7, 11, 0, 1, 0, 0)]
    assert r.stats == dict(roots=1, nodes_removed=2, pus_removed=1, tasks_evicted=2, arcs_removed=7, cap_updates=6,
                           records=8)


def test_toy_one_machine_preemptive_rule():
    """Slots below, running tasks not subtracted: only X → R1 changes (4 → 2)."""
    r = remove_reference(toy(), [TOY_M1], TOY_BINDINGS, True, True)
    assert r.removed == [5, 9] and r.evicted == [(14, 9), (15, 9)]
    want = {k: a for k, a in TOY_ARCS.items() if k not in GONE_WITH_M1}
    want[(2, 3)] = (0, 2, 0, 0)
    assert r.arcs == want
    assert stream_rows(r.stream) == [(1, 5, 0, 0, 0, 0, 0, 0), (1, 9, 0, 0, 0, 0, 0, 0), (3, 0, 2, 3, 0, 2, 0, 0)]
    assert r.stats == dict(roots=1, nodes_removed=2, pus_removed=1, tasks_evicted=2, arcs_removed=7, cap_updates=1,
                           records=3)


def test_toy_without_capacities():
    r = remove_reference(toy(), [TOY_M1], TOY_BINDINGS, False, False)
    assert r.arcs == {k: a for k, a in TOY_ARCS.items() if k not in GONE_WITH_M1}
    assert stream_rows(r.stream) == [(1, 5, 0, 0, 0, 0, 0, 0), (1, 9, 0, 0, 0, 0, 0, 0)]
    assert (r.stats["cap_updates"], r.stats["records"]) == (0, 2)


@pytest.mark.parametrize("preemptive", [False, True])
def test_rack_with_one_of_its_machines_is_the_rack(preemptive):
    a = remove_reference(toy(), [TOY_R1], TOY_BINDINGS, True, preemptive)
    b = remove_reference(toy(), [TOY_M1, TOY_R1, TOY_M1], TOY_BINDINGS, True, preemptive)
    assert a.removed == b.removed == [3, 5, 6, 9, 10]
    assert a.evicted == b.evicted == [(14, 9), (15, 9), (16, 10)]
    assert a.arcs == b.arcs and a.bindings == b.bindings == {17: 11}
    assert stream_rows(a.stream) == stream_rows(b.stream)
    assert (a.stats["roots"], b.stats["roots"]) == (1, 2)
    # the rack's own in-arcs went with it: X → R1 gets no record, X → R2 follows the rule
    assert (2, 3) not in a.arcs and a.arcs[(2, 4)] == (0, 4 if preemptive else 3, 0, 0)


def test_an_aggregator_goes_alone():
    r = remove_reference(toy(), [TOY_U], TOY_BINDINGS, True, True)
    assert r.removed == [13] and r.evicted == [] and r.bindings == TOY_BINDINGS
    assert set(TOY_ARCS) - set(r.arcs) == {(13, 1)} | {(t, 13) for t in range(14, 20)}
    assert r.stats["pus_removed"] == 0 and r.stats["cap_updates"] == 0


@pytest.mark.parametrize("roots", [[TOY_M1], [TOY_R1], [TOY_M1, 8], [9], [TOY_U, 4]])
@pytest.mark.parametrize("preemptive", [False, True])
def test_the_stream_reproduces_the_table(roots, preemptive):
    """The returned records through the store's semantics give the returned table."""
    r = remove_reference(toy(), roots, TOY_BINDINGS, True, preemptive)
    nodes = {i + 1: [TOY_SUPPLY[i], TOY_NTYPE[i]] for i in range(len(TOY_NTYPE))}
    arcs = {k: a[:3] for k, a in TOY_ARCS.items()}
    apply_deltas_to_arcs(nodes, arcs, r.stream)
    assert arcs == {k: a[:3] for k, a in r.arcs.items()}
    assert sorted(set(range(1, len(TOY_NTYPE) + 1)) - set(nodes)) == r.removed
    # no record names a removed node after its removal
    gone = set(r.removed)
    assert all(int(x["src"]) not in gone and int(x["dst"]) not in gone for x in r.stream[len(r.removed):])


def test_refusals_of_the_rule():
    for bad in (0, 14, 1, len(TOY_NTYPE) + 1):          # beyond the graph, a task, the sink
        with pytest.raises(InvalidRoot):
            remove_reference(toy(), [TOY_M1, bad], TOY_BINDINGS, True, False)
    with pytest.raises(InvalidRoot):
        remove_reference(toy(), [TOY_M1], TOY_BINDINGS, True, False, alive=set(range(1, 20)) - {TOY_M1})
    arcs = dict(TOY_ARCS)
    arcs[(2, 3)] = (3, 4, 0, 0)                         # lower bound 3, the new capacity would be 2
    with pytest.raises(BelowLowerBound):
        remove_reference(table_graph(TOY_NTYPE, TOY_SUPPLY, arcs), [TOY_M1], TOY_BINDINGS, True, True)


def test_library_exports_the_entry_point():
    """Fails on a library built before ks_remove_resources."""
    assert "ks_remove_resources" in native.EXPORTED_SYMBOLS
    lib = native.load(build_if_missing=True)
    assert hasattr(lib, "ks_remove_resources")


def test_binding_has_remove_resources():
    assert callable(getattr(native.Context, "remove_resources", None))
    assert (native.KS_REMOVE_RESOURCE_CAPS, native.KS_REMOVE_PREEMPTIVE) == (1, 2)
    assert ctypes.sizeof(native.KsRemoveStats) == 96
