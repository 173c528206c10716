"""CPU suite: ks_commit_preemptive's host-visible pieces. The ks_preempt_stats layout
equals the ctypes struct; the rule the GPU tests hold the device to
(tests/preempt_ref.py) gives the listed deltas, records and statistics on the toy
network; and it equals the churn model's own preemptive step 1 (ksched_amd/churn.py),
arc for arc including the arc types, on inputs that hold every delta kind."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from commit_ref import arc_table
from ksched_amd import churn, native
from oracle import ko, sched_ref
from preempt_ref import (CELL_CASES, MIGRATE, PLACE, PREEMPT, TOY_ARCS, TOY_CONTINUATION, TOY_NTYPE,
                         TOY_PREEMPTION, TOY_ROUNDS, TOY_SUPPLY, apply_edits, preempt_reference, table_graph,
                         toy_stats)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("placed", "preempted", "migrated", "running_added", "running_converted", "running_removed",
          "unsched_cost_updates", "cap_updates", "records", "reserved")
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_preempt_stats %zu\n", sizeof(ks_preempt_stats));
""" + "".join(f"  P(ks_preempt_stats, {f});\n" for f in FIELDS) + r"""
  printf("ks_commit_stats %zu\n", sizeof(ks_commit_stats));
  return 0;
}
"""


def test_preempt_stats_layout_and_export(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_preempt_stats"] == C.sizeof(native.KsPreemptStats) == 96
    assert [f for f, _ in native.KsPreemptStats._fields_] == list(FIELDS)
    for f in FIELDS:
        assert getattr(native.KsPreemptStats, f).offset == out[f"ks_preempt_stats.{f}"], f
    assert "reserved" not in native.KsPreemptStats().as_dict()
    assert out["ks_commit_stats"] == 96                  # the pinned mode's struct is untouched
    assert "ks_commit_preemptive" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "ks_commit_preemptive")
    assert native.load().ks_abi_version() == 5           # no struct changed layout


def test_toy_network_rounds():
    """The oracle's optimum of every solve, the deltas of its mapping and the records
    and statistics the rule makes of them."""
    arcs = dict(TOY_ARCS)
    bindings: dict = {}
    for n, rnd in enumerate(TOY_ROUNDS):
        apply_edits(arcs, rnd["edits"])
        g = table_graph(TOY_NTYPE, TOY_SUPPLY, arcs)
        st, cost, flow, fl = ko.cost_scaling(g)
        assert (st, cost, flow) == (0, rnd["cost"], 3), n
        deltas = sched_ref.scheduling_deltas(bindings, ko.bfs_mapping(g, fl), [9, 10, 11])
        assert deltas == rnd["deltas"], n
        arcs, bindings, stats = preempt_reference(g, deltas, bindings, TOY_CONTINUATION, TOY_PREEMPTION, True)
        assert stats == toy_stats(rnd), n
        assert bindings == sched_ref.apply_deltas({}, [d for r in TOY_ROUNDS[:n + 1] for d in r["deltas"]]), n
    assert arcs[(9, 6)] == arcs[(10, 8)] == arcs[(11, 4)] == (0, 1, 0, 1)
    assert (9, 4) not in arcs and (10, 6) not in arcs
    assert arcs[(9, 2)][2] == arcs[(10, 2)][2] == arcs[(11, 2)][2] == TOY_PREEMPTION


def running_pinned(g):
    """g with every running arc's lower bound raised to 1: no running task may move."""
    low = g.low.copy()
    low[g.arc_types() == 1] = 1
    return type(g)(g.ntype, g.supply, g.src, g.dst, low, g.cap, g.cost, g.arc_types())


@pytest.mark.parametrize("shape", list(CELL_CASES))
def test_preempt_reference_equals_the_churn_model(shape):
    """Three rounds, 5 % churn in between, driven by the oracle's mappings: the rule
    applied to the cell's graph gives the cell's graph after its own step 1. The
    deltas hold every kind, and in a later round every optimum moves a running task:
    with the running arcs pinned the round's graph costs strictly more (or is
    infeasible)."""
    pc = CELL_CASES[shape]
    cell = churn.Cell(*shape, preemption=True, preemption_cost=pc)
    T = shape[0]
    kinds = {PLACE: 0, PREEMPT: 0, MIGRATE: 0}
    forced = 0
    for rnd in range(3):
        g = cell.graph()
        st, cost, _, fl = ko.cost_scaling(g)
        assert st == 0
        mp = ko.bfs_mapping(g, fl)
        run = cell.task_ids(cell.RUN)
        bindings = dict(zip(run.tolist(), cell.pu[run - cell.TASK0].tolist()))
        live = np.concatenate([run, cell.task_ids(cell.WAIT)])
        deltas = sched_ref.scheduling_deltas(bindings, mp, live)
        for k, _, _ in deltas:
            kinds[k] += 1
        want, nb, stats = preempt_reference(g, deltas, bindings, 0, pc, True)
        host = cell.step(mp, 0, 0, age_cost=0, seed=100 + rnd)
        got = {k: a for k, a in arc_table(cell.graph()).items() if a[1] > 0}
        assert got == want, rnd
        assert stats["records"] == host.shape[0] and stats["cap_updates"] == 0, rnd
        run = cell.task_ids(cell.RUN)
        assert dict(zip(run.tolist(), cell.pu[run - cell.TASK0].tolist())) == nb, rnd
        if rnd > 0:
            st1, cost1, _, _ = ko.cost_scaling(running_pinned(g))
            forced += st1 != 0 or cost1 > cost
            print(f"shape {shape} round {rnd}: cost {cost}, running arcs pinned: status {st1} cost {cost1}")
        cell.step(None, T // 20, T // 20, seed=200 + rnd)
    print(f"shape {shape}: deltas by kind {kinds}")
    assert kinds[PLACE] > 0 and kinds[PREEMPT] > 0 and kinds[MIGRATE] > 0
    assert forced > 0


def test_default_cell_is_unchanged():
    """Without preemption the model emits what it emitted before: two default
    instances agree step by step, with the record counts test_commit_cpu.py pins."""
    a, b = churn.Cell(200, 20, 4, 5, 3), churn.Cell(200, 20, 4, 5, 3, preemption=False, preemption_cost=0)
    T = 200
    for rnd in range(3):
        g = a.graph()
        assert arc_table(g) == arc_table(b.graph())
        st, _, _, fl = ko.cost_scaling(g)
        assert st == 0
        mp = ko.bfs_mapping(g, fl)
        waiting = set(a.task_ids(a.WAIT).tolist())
        ha, hb = a.step(mp, 0, 0, age_cost=0, seed=100 + rnd), b.step(dict(mp), 0, 0, age_cost=0, seed=100 + rnd)
        assert ha.tobytes() == hb.tobytes()
        if rnd == 0:
            assert (len([t for t in mp if t in waiting]), ha.shape[0]) == (193, 1207)
        ca, cb = a.step({}, T // 20, T // 20, seed=200 + rnd), b.step(None, T // 20, T // 20, seed=200 + rnd)
        assert ca.tobytes() == cb.tobytes()
    ga, gb = a.graph(), b.graph()
    for f in ("ntype", "supply", "src", "dst", "low", "cap", "cost"):
        assert getattr(ga, f).tobytes() == getattr(gb, f).tobytes(), f
