"""CPU: the restatement of ks_add_tasks (tests/arrive_ref.py) checked by hand on the 19-node
toy, against the churn model's own arrivals (ksched_amd/churn.py steps 3 and 5), against the
store semantics (graphs.apply_deltas_to_arcs), and the library's and the binding's new entry
point with the layout of its two structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from arrive_ref import (STAT_KEYS, Arrival, InvalidArrival, OutOfRange, arrive_reference, offsets)
from commit_ref import arc_table
from graphs import apply_deltas_to_arcs
from ksched_amd import churn, native
from oracle import ko
from preempt_ref import table_graph
from remove_ref import TOY_ARCS, TOY_NTYPE, TOY_SUPPLY, TOY_U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, M1, SINK = 2, 5, 1


def toy(arcs=None):
    return table_graph(TOY_NTYPE, TOY_SUPPLY, TOY_ARCS if arcs is None else arcs)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["id"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]),
             int(x["cost"]), int(x["type"]), int(x["excess"])) for x in stream]


def test_toy_two_tasks_raise_the_capacity():
    """21 and 20 arrive in that order; only 21 has an arc into U (13): U → sink 6 → 7."""
    r = arrive_reference(toy(), [21, 20], [[(TOY_U, 7), (X, 3)], [(M1, 1)]], unsched_ids=[TOY_U], sink_cost=9)
    assert stream_rows(r.stream) == [(0, 21, 0, 0, 0, 0, 0, 1, 1), (0, 20, 0, 0, 0, 0, 0, 1, 1),
                                     (2, 0, 21, 13, 0, 1, 7, 0, 0), (2, 0, 21, 2, 0, 1, 3, 0, 0),
                                     (2, 0, 20, 5, 0, 1, 1, 0, 0), (3, 0, 13, 1, 0, 7, 0, 0, 0)]
    assert r.stats == dict(tasks=2, arcs_added=3, unsched_updates=1, unsched_added=0, records=6)
    want = dict(TOY_ARCS)
    want.update({(21, 13): (0, 1, 7, 0), (21, 2): (0, 1, 3, 0), (20, 5): (0, 1, 1, 0), (13, 1): (0, 7, 0, 0)})
    assert r.arcs == want and r.superseded == 0
    assert r.alive == set(range(1, 22)) and r.ntype[19:] == [1, 1] and r.supply[19:] == [1, 1]
    null = arrive_reference(toy(), [21], [[(TOY_U, 7), (X, 3)]])            # the NULL rule finds U by its sink arc
    assert stream_rows(null.stream)[-1] == (3, 0, 13, 1, 0, 7, 0, 0, 0)


def test_toy_kept_bounds_and_a_recreated_arc():
    arcs = dict(TOY_ARCS)
    arcs[(13, 1)] = (1, 6, 40, 0)                                            # low 1, cost 40: both kept
    r = arrive_reference(toy(arcs), [25, 30], [[(TOY_U, 1)], [(TOY_U, 2)]], unsched_ids=[TOY_U], sink_cost=9)
    assert stream_rows(r.stream)[-1] == (3, 0, 13, 1, 1, 8, 40, 0, 0) and r.arcs[(13, 1)] == (1, 8, 40, 0)
    assert r.alive == set(range(1, 20)) | {25, 30} and len(r.ntype) == 30 and r.ntype[19:24] == [0] * 5
    del arcs[(13, 1)]                                                        # the store no longer holds it
    r = arrive_reference(toy(arcs), [25, 30], [[(TOY_U, 1)], [(TOY_U, 2)]], unsched_ids=[TOY_U], sink_cost=9)
    assert stream_rows(r.stream)[-1] == (2, 0, 13, 1, 0, 2, 9, 0, 0) and r.arcs[(13, 1)] == (0, 2, 9, 0)
    assert r.stats == dict(tasks=2, arcs_added=2, unsched_updates=0, unsched_added=1, records=5)


def test_toy_reuse_no_arcs_a_repeated_head_and_nothing():
    alive = set(range(1, 20)) - {15}
    arcs = {k: a for k, a in TOY_ARCS.items() if 15 not in k}
    r = arrive_reference(toy(arcs), [15, 20], [[(M1, 5), (X, 2), (M1, 8)], []], unsched_ids=[TOY_U], alive=alive)
    assert r.superseded == 1 and r.arcs[(15, 5)] == (0, 1, 8, 0)             # the later record stands
    assert r.stats == dict(tasks=2, arcs_added=3, unsched_updates=0, unsched_added=0, records=5)
    assert r.arcs[(13, 1)] == TOY_ARCS[(13, 1)] and 15 in r.alive and 20 in r.alive
    none = arrive_reference(toy(), [], [])
    assert none.stream.shape[0] == 0 and none.arcs == TOY_ARCS and not any(none.stats.values())


def test_refusals_of_the_rule():
    u = [TOY_U]
    for bad, err in ((0, OutOfRange), (1 << 30, OutOfRange), (14, InvalidArrival), (13, InvalidArrival)):
        with pytest.raises(err) as e:
            arrive_reference(toy(), [20, bad, 0], [[], [], []], unsched_ids=u)
        assert e.value.args[0] == bad                                        # the first offending id is named
    with pytest.raises(InvalidArrival) as e:
        arrive_reference(toy(), [20, 21, 20], [[], [], []], unsched_ids=u)   # listed twice: already present
    assert e.value.args[0] == 20
    alive = set(range(1, 20)) - {15}
    for head in (0, 15, 14, 40, 21):                                         # 0, dead, a task, beyond, of this call
        with pytest.raises(InvalidArrival) as e:
            arrive_reference(toy(), [20, 21], [[(X, 1)], [(X, 1), (head, 1)]], unsched_ids=u, alive=alive)
        assert e.value.args == (21, head)
    with pytest.raises(InvalidArrival) as e:
        arrive_reference(toy(), [20], [[(TOY_U, 1), (X, 1), (TOY_U, 2)]], unsched_ids=u)       # one aggregator twice
    assert e.value.args[0] == 20
    with pytest.raises(InvalidArrival):
        arrive_reference(toy(), [20], [[(TOY_U, 1), (X, 1)]], unsched_ids=[TOY_U, X])         # two aggregators
    arcs = {k: a for k, a in TOY_ARCS.items() if k != (13, 1)}
    with pytest.raises(InvalidArrival) as e:                                 # the NULL rule cannot see a drained U
        arrive_reference(toy(arcs), [20], [[(TOY_U, 1), (X, 1)]])
    assert e.value.args[0] == 20
    assert arrive_reference(toy(arcs), [20], [[(X, 1)]], unsched_ids=u).stats["records"] == 2  # explicit ids: legal
    with pytest.raises(OutOfRange):
        arrive_reference(toy(), [20], [[(X, (1 << 40) + 1)]], unsched_ids=u)
    assert arrive_reference(toy(), [20], [[(X, 1 << 40), (M1, -(1 << 40))]], unsched_ids=u).stats["arcs_added"] == 2
    with pytest.raises(OutOfRange):
        arrive_reference(toy(), [20], [[]], unsched_ids=u, sink_cost=-(1 << 40) - 1)
    two = table_graph(TOY_NTYPE + [3], TOY_SUPPLY + [0], TOY_ARCS)
    with pytest.raises(InvalidArrival):
        arrive_reference(two, [21], [[(TOY_U, 1)]], unsched_ids=u)           # a unit needs exactly one sink
    assert arrive_reference(two, [21], [[(X, 1)]], unsched_ids=u).stats["records"] == 2


@pytest.mark.parametrize("case", range(4))
def test_the_stream_reproduces_the_table(case):
    """The returned records through the store's semantics give the returned table."""
    arcs = dict(TOY_ARCS)
    if case == 3:
        del arcs[(13, 1)]
    tasks, lists = [([20], [[(TOY_U, 3)]]), ([40, 22], [[(M1, 5), (X, 2), (M1, 8)], [(TOY_U, 1)]]),
                    ([20, 21, 22], [[], [(TOY_U, 1), (SINK, 4)], [(TOY_U, 2)]]), ([23], [[(TOY_U, 5), (3, 1)]])][case]
    r = arrive_reference(toy(arcs), tasks, lists, unsched_ids=[TOY_U], sink_cost=17)
    nodes = {i + 1: [TOY_SUPPLY[i], TOY_NTYPE[i]] for i in range(len(TOY_NTYPE))}
    low3 = {k: a[:3] for k, a in arcs.items()}
    apply_deltas_to_arcs(nodes, low3, r.stream)
    assert low3 == {k: a[:3] for k, a in r.arcs.items()}
    assert set(nodes) == r.alive and all(nodes[t] == [1, 1] for t in tasks)
    k, na = len(tasks), sum(len(x) for x in lists)
    assert [int(x["id"]) for x in r.stream[:k]] == tasks                     # the fixed positions
    flat = [(t, d) for t, lst in zip(tasks, lists) for d, _ in lst]
    assert list(zip(r.stream["src"][k:k + na].tolist(), r.stream["dst"][k:k + na].tolist())) == flat
    assert r.stats["records"] == r.stream.shape[0] == sum(r.stats[f] for f in STAT_KEYS[:4])
    off, dst, cost = offsets(lists)
    assert off.tolist() == np.cumsum([0] + [len(x) for x in lists]).tolist() and dst.shape == cost.shape == (na,)


# ---- against the churn model ---------------------------------------------------------
def positive(arcs: dict) -> dict:
    return {k: a for k, a in arcs.items() if a[1] > 0}


@pytest.mark.parametrize("preemption", [False, True], ids=["pinned", "preemptive"])
@pytest.mark.parametrize("shape", [(40, 8, 2, 6, 3), (200, 20, 4, 5, 3)])
def test_arrive_reference_equals_the_churn_model(shape, preemption):
    """A solve's placements are committed and a third of the running tasks complete (the
    cell's own steps 1, 2 and 5; pinned, whole jobs drain to 0 and lose their arc into the
    sink). Then a round of arrivals alone: the step-3 records of Cell.step with the arrivals'
    share of its U_j → sink records. The rule on the cell's graph before that round, as a
    device store holds it (without the arcs of capacity 0), gives the cell's graph after it."""
    cell = churn.Cell(*shape, preemption=preemption, preemption_cost=150)
    g = cell.graph()
    st, _, _, fl = ko.cost_scaling(g)
    assert st == 0
    cell.step(ko.bfs_mapping(g, fl), max(1, shape[0] // 3), 0, age_cost=0, seed=100)
    g = cell.graph()
    before = positive(arc_table(g))
    aggs = [cell.U0 + j for j in range(cell.J)]
    drained = [u for u in aggs if (u, cell.SINK) not in before]
    host = cell.step(None, 0, shape[0] // 2, age_cost=0, seed=200)
    ids = list(cell.last_arrived_ids)
    assert len(ids) == shape[0] // 2 and min(ids) < cell.TASK0 + shape[0] <= max(ids)      # reused and fresh ids
    sl = np.asarray(ids) - cell.TASK0
    lists = [list(zip(cell.adst[s].tolist(), cell.acost[s].tolist())) for s in sl]
    alive = {i + 1 for i in range(g.n) if i + 1 < cell.TASK0 or g.ntype[i] == 1}
    ref = arrive_reference(table_graph(g.ntype, g.supply, before), ids, lists, unsched_ids=aggs, alive=alive)
    assert positive(ref.arcs) == positive(arc_table(cell.graph()))
    assert ref.stats["unsched_added"] == len([u for u in drained if (u, cell.SINK) in ref.arcs])
    if not preemption and shape[0] == 40:                                    # the small cell places whole jobs
        assert drained and ref.stats["unsched_added"] > 0
    # the model's own records: a node and five arcs per arrival, one record per job that gained
    assert ref.stats["records"] == host.shape[0]
    assert ref.stats["unsched_updates"] + ref.stats["unsched_added"] == np.unique(cell.job[sl]).shape[0]
    nodes = {i: [int(g.supply[i - 1]), int(g.ntype[i - 1])] for i in alive}
    low3 = {k: a[:3] for k, a in before.items()}
    apply_deltas_to_arcs(nodes, low3, host)                                  # the host's stream, its own order
    assert low3 == {k: a[:3] for k, a in ref.arcs.items()}
    with pytest.raises(InvalidArrival):                                      # an id of the round before is live now
        arrive_reference(cell.graph(), ids[:1], lists[:1], unsched_ids=aggs)


# ---- the library and the binding ------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_add_stats %zu\n", sizeof(ks_add_stats));
  printf("ks_task_arc %zu\n", sizeof(ks_task_arc));
  P(ks_task_arc, dst);
  P(ks_task_arc, cost);
""" + "".join(f"  P(ks_add_stats, {f});\n" for f in STAT_KEYS + ("reserved",)) + r"""
  printf("abi %d\n", KSMCMF_ABI_VERSION);
  return 0;
}
"""


def test_add_structs_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_add_stats"] == C.sizeof(native.KsAddStats) == 96
    assert out["ks_task_arc"] == native.TASK_ARC_DT.itemsize == 16
    assert (out["ks_task_arc.dst"], out["ks_task_arc.cost"]) == (0, 8)
    assert (native.TASK_ARC_DT.fields["dst"][1], native.TASK_ARC_DT.fields["cost"][1]) == (0, 8)
    assert [f for f, _ in native.KsAddStats._fields_] == list(STAT_KEYS) + ["reserved"]
    for f in STAT_KEYS + ("reserved",):
        assert getattr(native.KsAddStats, f).offset == out[f"ks_add_stats.{f}"], f
    assert tuple(native.KsAddStats().as_dict()) == STAT_KEYS
    assert out["abi"] == native.ABI_VERSION == 5          # an entry point and two structs were added, nothing moved


def test_library_exports_the_entry_point():
    """Fails on a library built before ks_add_tasks."""
    lib = native.load(build_if_missing=True)
    assert "ks_add_tasks" in native.EXPORTED_SYMBOLS
    assert hasattr(lib, "ks_add_tasks")
    assert lib.ks_abi_version() == 5


def test_binding_has_add_tasks():
    assert callable(getattr(native.Context, "add_tasks", None))
    assert Arrival._fields == ("arcs", "ntype", "supply", "alive", "stream", "stats", "superseded")
