"""CPU: the restatement of ks_complete_tasks (tests/complete_ref.py) checked by hand on the
19-node toy, against the churn model's own completions in both modes (ksched_amd/churn.py
steps 2 and 5), against the store semantics (graphs.apply_deltas_to_arcs), and the library's
and the binding's new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from commit_ref import arc_table
from complete_ref import (STAT_KEYS, Completion, InvalidTask, chain_upserts, complete_reference, parent_chains)
from graphs import apply_deltas_to_arcs
from ksched_amd import churn, native
from oracle import ko
from preempt_ref import table_graph
from remove_ref import TOY_ARCS, TOY_BINDINGS, TOY_NTYPE, TOY_SUPPLY, TOY_U, BelowLowerBound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T1, T5, P1 = 14, 18, 9


def toy(arcs=None):
    return table_graph(TOY_NTYPE, TOY_SUPPLY, TOY_ARCS if arcs is None else arcs)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["id"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]),
             int(x["cost"]), int(x["type"])) for x in stream]


GONE_WITH_T1_T5 = {(14, 13), (14, 2), (14, 5), (14, 9), (18, 13), (18, 2), (18, 5), (18, 6)}


def test_toy_running_and_waiting_preemptive_rule():
    """T1 (14) ran on P1 (9), T5 (18) waited; both had an arc into U (13): U → sink 6 → 4.
    Slots below change with no completion: no resource arc gets a record."""
    r = complete_reference(toy(), [T1, T5], TOY_BINDINGS, True, True)
    assert r.left == [P1, 0] and r.removed == [14, 18]
    assert r.bindings == {15: 9, 16: 10, 17: 11}
    want = {k: a for k, a in TOY_ARCS.items() if k not in GONE_WITH_T1_T5}
    want[(13, 1)] = (0, 4, 0, 0)
    assert r.arcs == want
    assert stream_rows(r.stream) == [(1, 14, 0, 0, 0, 0, 0, 0), (1, 18, 0, 0, 0, 0, 0, 0), (3, 0, 13, 1, 0, 4, 0, 0)]
    assert r.stats == dict(tasks=2, bound=1, arcs_removed=8, unsched_updates=1, cap_updates=0, records=3)
    off = complete_reference(toy(), [T1, T5], TOY_BINDINGS, False, False)       # the flag off: the same edit
    assert off.arcs == want and stream_rows(off.stream) == stream_rows(r.stream) and off.stats == r.stats


def test_toy_pinned_rule_the_arcs_above_p1_gain_one():
    """slots − running below. The plain refresh (k == 0): P1 runs two tasks on two slots, so
    M1 → P1 and R1 → M1 fall to 0 and go, X → R1 is 4 − 3. With T1 completed each of the
    three stands one higher."""
    plain = complete_reference(toy(), [], TOY_BINDINGS, True, False)
    assert plain.removed == [] and plain.left == [] and plain.stats["tasks"] == 0
    assert (5, 9) not in plain.arcs and (3, 5) not in plain.arcs and plain.arcs[(2, 3)] == (0, 1, 0, 0)
    assert plain.arcs[(13, 1)] == (0, 6, 0, 0) and plain.stats["unsched_updates"] == 0
    r = complete_reference(toy(), [T1], TOY_BINDINGS, True, False)
    assert r.left == [P1] and r.stats["bound"] == 1
    assert r.arcs[(5, 9)] == r.arcs[(3, 5)] == (0, 1, 0, 0) and r.arcs[(2, 3)] == (0, 2, 0, 0)
    for k in ((6, 10), (3, 6), (7, 11), (4, 7)):                               # one task runs below each
        assert r.arcs[k] == plain.arcs[k] == (0, 1, 0, 0)
    assert r.arcs[(2, 4)] == plain.arcs[(2, 4)] == (0, 3, 0, 0)
    assert r.arcs[(8, 12)] == r.arcs[(4, 8)] == (0, 2, 0, 0)
    assert r.arcs[(13, 1)] == (0, 5, 0, 0)
    assert stream_rows(r.stream) == [(1, 14, 0, 0, 0, 0, 0, 0),
                                     (3, 0, 2, 3, 0, 2, 0, 0), (3, 0, 2, 4, 0, 3, 0, 0), (3, 0, 3, 5, 0, 1, 0, 0),
                                     (3, 0, 3, 6, 0, 1, 0, 0), (3, 0, 4, 7, 0, 1, 0, 0), (3, 0, 5, 9, 0, 1, 0, 0),
                                     (3, 0, 6, 10, 0, 1, 0, 0), (3, 0, 7, 11, 0, 1, 0, 0), (3, 0, 13, 1, 0, 5, 0, 0)]
    assert r.stats == dict(tasks=1, bound=1, arcs_removed=4, unsched_updates=1, cap_updates=8, records=10)


def test_duplicates_explicit_aggregators_and_a_whole_job():
    a = complete_reference(toy(), [T5, T1, T5], TOY_BINDINGS, False, False)
    assert a.left == [0, P1, 0] and a.removed == [14, 18] and a.stats["tasks"] == 2
    b = complete_reference(toy(), [T1, T5], TOY_BINDINGS, False, False, unsched_ids=[TOY_U])
    assert b.arcs == a.arcs and b.stats == a.stats
    none = complete_reference(toy(), [T1, T5], TOY_BINDINGS, False, False, unsched_ids=[])
    assert none.arcs[(13, 1)] == (0, 6, 0, 0) and none.stats["unsched_updates"] == 0
    every = complete_reference(toy(), list(range(14, 20)), TOY_BINDINGS, False, False)
    assert (13, 1) not in every.arcs and every.bindings == {}                  # capacity 0 removes the arc
    assert stream_rows(every.stream)[-1] == (3, 0, 13, 1, 0, 0, 0, 0)
    assert every.stats == dict(tasks=6, bound=4, arcs_removed=22, unsched_updates=1, cap_updates=0, records=7)


def test_refusals_of_the_rule():
    for bad in (0, 9, 1, 13, len(TOY_NTYPE) + 1):        # id 0, a PU, the sink, an aggregator, beyond the graph
        with pytest.raises(InvalidTask) as e:
            complete_reference(toy(), [T1, bad, 0], TOY_BINDINGS, True, False)
        assert e.value.args[0] == bad                     # the first illegal id is named
    with pytest.raises(InvalidTask):
        complete_reference(toy(), [T1], TOY_BINDINGS, True, False, alive=set(range(1, 20)) - {T1})
    arcs = dict(TOY_ARCS)
    arcs[(13, 1)] = (6, 6, 0, 0)                          # U → sink: lower bound 6, the new capacity would be 5
    with pytest.raises(BelowLowerBound):
        complete_reference(toy(arcs), [T5], TOY_BINDINGS, False, False)
    arcs = dict(TOY_ARCS)
    arcs[(2, 3)] = (3, 4, 0, 0)                           # X → R1: lower bound 3, slots − running below is 2
    with pytest.raises(BelowLowerBound):
        complete_reference(toy(arcs), [T1], TOY_BINDINGS, True, False)


@pytest.mark.parametrize("tasks", [[T1, T5], [T1], [15, 14], [16, 17, 19], list(range(14, 20)), []])
@pytest.mark.parametrize("caps,preemptive", [(False, False), (True, False), (True, True)])
def test_the_stream_reproduces_the_table(tasks, caps, preemptive):
    """The returned records through the store's semantics give the returned table."""
    r = complete_reference(toy(), tasks, TOY_BINDINGS, caps, preemptive)
    nodes = {i + 1: [TOY_SUPPLY[i], TOY_NTYPE[i]] for i in range(len(TOY_NTYPE))}
    arcs = {k: a[:3] for k, a in TOY_ARCS.items()}
    apply_deltas_to_arcs(nodes, arcs, r.stream)
    assert arcs == {k: a[:3] for k, a in r.arcs.items()}
    assert sorted(set(range(1, len(TOY_NTYPE) + 1)) - set(nodes)) == r.removed
    gone = set(r.removed)
    tail = r.stream[len(r.removed):]
    assert all(int(x["src"]) not in gone and int(x["dst"]) not in gone for x in tail)
    keys = list(zip(tail["src"].tolist(), tail["dst"].tolist()))
    assert len(keys) == len(set(keys))                    # no (src, dst) twice: nothing is superseded
    assert r.stats["records"] == r.stats["tasks"] + r.stats["unsched_updates"] + r.stats["cap_updates"]


# ---- against the churn model ---------------------------------------------------------
def positive(arcs: dict) -> dict:
    return {k: a for k, a in arcs.items() if a[1] > 0}


@pytest.mark.parametrize("preemption", [False, True], ids=["pinned", "preemptive"])
@pytest.mark.parametrize("shape", [(60, 8, 2, 3, 3), (200, 20, 4, 5, 3)])
def test_complete_reference_equals_the_churn_model(shape, preemption):
    """Two rounds: a solve's placements are committed by the cell's own step 1, then the
    cell completes a tenth of its running tasks (steps 2 and 5, no arrivals, no ageing). The
    rule on the cell's graph before that step — as a device store holds it: without the
    arcs of capacity 0, and in the pinned mode after the chain recipe — gives the cell's
    graph after it."""
    cell = churn.Cell(*shape, preemption=preemption, preemption_cost=150)
    g0 = cell.graph()                                     # the caller's own copy of the topology: every resource arc
    topology = {k: a for k, a in arc_table(g0).items() if g0.ntype[k[0] - 1] != 1}
    done_total = 0
    for rnd in range(2):
        g = cell.graph()
        st, _, _, fl = ko.cost_scaling(g)
        assert st == 0
        cell.step(ko.bfs_mapping(g, fl), 0, 0, age_cost=0, seed=100 + rnd)
        g = cell.graph()
        run = cell.task_ids(cell.RUN)
        bindings = dict(zip(run.tolist(), cell.pu[run - cell.TASK0].tolist()))
        host = cell.step(None, max(1, run.shape[0] // 10), 0, age_cost=0, seed=200 + rnd)
        done = host["id"][host["kind"] == churn.KS_REMOVE_NODE].astype(np.int64).tolist()
        assert done and set(done) <= set(bindings)
        done_total += len(done)
        ntype = [int(t) for t in g.ntype]
        before = positive(arc_table(g))
        if not preemption:                                # ks_get_bindings → the chains' upserts
            chain = parent_chains(ntype, topology, [bindings[t] for t in done])
            assert len(chain) >= 3
            nodes = {i + 1: [int(s), t] for i, (s, t) in enumerate(zip(g.supply, ntype))}
            low3 = {k: a[:3] for k, a in before.items()}
            apply_deltas_to_arcs(nodes, low3, chain_upserts(topology, chain))
            before = {k: (*a, before[k][3] if k in before else topology[k][3]) for k, a in low3.items()}
        ref = complete_reference(table_graph(ntype, g.supply, before), done, bindings, True, preemption)
        assert positive(ref.arcs) == positive(arc_table(cell.graph())), rnd
        assert ref.left == [bindings[t] for t in done] and ref.stats["bound"] == len(done)
        assert ref.stats["unsched_updates"] == (np.unique(cell.job[np.asarray(done) - cell.TASK0]).shape[0]
                                                if preemption else 0)
        if preemption:
            assert ref.stats["cap_updates"] == 0          # slots below: a completion moves no resource arc
            # the model's own records: the removals and the aggregators' capacities
            assert ref.stats["records"] == host.shape[0]
    assert done_total >= 2


# ---- the library and the binding ------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_complete_stats %zu\n", sizeof(ks_complete_stats));
""" + "".join(f"  P(ks_complete_stats, {f});\n" for f in STAT_KEYS + ("reserved",)) + r"""
  printf("flags %d\n", KS_COMPLETE_RESOURCE_CAPS * 16 + KS_COMPLETE_PREEMPTIVE);
  printf("abi %d\n", KSMCMF_ABI_VERSION);
  return 0;
}
"""


def test_complete_stats_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_complete_stats"] == C.sizeof(native.KsCompleteStats) == 96
    assert [f for f, _ in native.KsCompleteStats._fields_] == list(STAT_KEYS) + ["reserved"]
    for f in STAT_KEYS + ("reserved",):
        assert getattr(native.KsCompleteStats, f).offset == out[f"ks_complete_stats.{f}"], f
    assert tuple(native.KsCompleteStats().as_dict()) == STAT_KEYS
    assert out["flags"] == 16 * native.KS_COMPLETE_RESOURCE_CAPS + native.KS_COMPLETE_PREEMPTIVE == 18
    assert out["abi"] == native.ABI_VERSION == 5          # entry points and one struct were added, nothing moved


def test_library_exports_the_entry_points():
    """Fails on a library built before ks_complete_tasks."""
    lib = native.load(build_if_missing=True)
    for name in ("ks_complete_tasks", "ks_get_bindings"):
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ks_abi_version() == 5


def test_binding_has_complete_tasks_and_bindings():
    assert callable(getattr(native.Context, "complete_tasks", None))
    assert callable(getattr(native.Context, "bindings", None))
    assert Completion._fields == ("arcs", "left", "removed", "bindings", "stream", "stats")
