"""CPU: the restatement of ks_update_tasks (tests/refresh_ref.py) checked by hand on the 19-node
toy, against the store semantics (graphs.apply_deltas_to_arcs) on the toy and on a churn-model
graph after a few of its rounds, every refusal of the rule, and the library's and the binding's
new entry point with the layout of its struct."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from commit_ref import arc_table
from graphs import apply_deltas_to_arcs
from ksched_amd import churn, native
from oracle import ko
from preempt_ref import table_graph
from refresh_ref import KEEP_UNLISTED, STAT_KEYS, InvalidRefresh, OutOfRange, Refresh, refresh_reference
from remove_ref import TOY_ARCS, TOY_BINDINGS, TOY_NTYPE, TOY_SUPPLY, TOY_U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, R1, M1, M2, M3, P1, SINK = 2, 3, 5, 6, 7, 9, 1
U = [TOY_U]


def refresh(tasks, lists, arcs=None, bindings=TOY_BINDINGS, ids=U, **kw) -> Refresh:
    return refresh_reference(TOY_NTYPE, TOY_ARCS if arcs is None else arcs, tasks, lists, bindings, ids, **kw)


def stream_rows(stream) -> list:
    return [(int(x["kind"]), int(x["src"]), int(x["dst"]), int(x["low"]), int(x["cap"]), int(x["cost"]),
             int(x["old_cost"]), int(x["type"])) for x in stream]


def stats(**kw) -> dict:
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(kw)
    return st


def evicted(task, arcs=None) -> dict:
    """The toy after a pinned commit and an eviction of the task: it has no out-arc left."""
    return {k: a for k, a in (TOY_ARCS if arcs is None else arcs).items() if k[0] != task}


# ---- the rule by hand ------------------------------------------------------------------
MIXED = [(M1, 44), (M2, 6), (M3, 2), (TOY_U, 118)]    # 18: a cost change, unchanged, a new head; X is dropped


def test_toy_one_list_changes_adds_keeps_and_drops():
    r = refresh([18], [MIXED])
    # held arcs by arc slot: (18, X) stands before (18, M1) in the table; then the new head
    assert stream_rows(r.stream) == [(3, 18, X, 0, 0, 58, 58, 0), (3, 18, M1, 0, 1, 44, 4, 0), (2, 18, M3, 0, 1, 2, 0, 0)]
    assert r.stats == stats(tasks=1, arcs_added=1, cost_updates=1, arcs_unchanged=2, arcs_removed=1, records=3)
    want = dict(TOY_ARCS)
    del want[(18, X)]
    want.update({(18, M1): (0, 1, 44, 0), (18, M3): (0, 1, 2, 0)})
    assert r.arcs == want


def test_toy_keep_unlisted_deletes_nothing():
    r = refresh([18], [MIXED], flags=KEEP_UNLISTED)
    assert stream_rows(r.stream) == [(3, 18, M1, 0, 1, 44, 4, 0), (2, 18, M3, 0, 1, 2, 0, 0)]
    assert r.stats == stats(tasks=1, arcs_added=1, cost_updates=1, arcs_unchanged=2, records=2)
    assert r.arcs[(18, X)] == TOY_ARCS[(18, X)]


def test_toy_running_arcs_stay_listed_or_not():
    """14 lists its running arc with another cost, 15 does not list its own: neither gets a record."""
    r = refresh([14, 15], [[(P1, 77), (TOY_U, 114)], [(TOY_U, 115), (X, 55), (R1, 9)]])
    assert stream_rows(r.stream) == [(3, 14, X, 0, 0, 54, 54, 0), (3, 14, M1, 0, 0, 3, 3, 0)]
    assert r.stats == stats(tasks=2, arcs_unchanged=4, running_kept=1, arcs_removed=2, records=2)
    assert r.arcs[(14, P1)] == r.arcs[(15, P1)] == (0, 1, 0, 1)


def test_toy_an_unlisted_aggregator_arc_keeps_its_cost_and_no_record_keeps_everything():
    for ids in (U, None):                           # the NULL rule finds U by its arc into the sink
        r = refresh([19], [[(X, 59), (8, 5)]], ids=ids)
        assert r.stream.shape[0] == 0 and r.arcs == TOY_ARCS
        assert r.stats == stats(tasks=1, arcs_unchanged=2)
    none = refresh([], [])
    assert none.stream.shape[0] == 0 and none.arcs == TOY_ARCS and not any(none.stats.values())


def test_toy_a_pinned_evicted_task_regains_its_unit():
    arcs = evicted(16)
    arcs[(13, 1)] = (1, 6, 40, 0)                   # low 1, cost 40: both kept
    bind = {t: p for t, p in TOY_BINDINGS.items() if t != 16}
    r = refresh([16], [[(TOY_U, 116), (X, 56)]], arcs=arcs, bindings=bind, sink_cost=9)
    assert stream_rows(r.stream) == [(2, 16, 13, 0, 1, 116, 0, 0), (2, 16, X, 0, 1, 56, 0, 0), (3, 13, 1, 1, 7, 40, 40, 0)]
    assert r.stats == stats(tasks=1, arcs_added=2, unsched_updates=1, records=3)
    del arcs[(13, 1)]                               # the pin drained it: the store no longer holds it
    r = refresh([16], [[(TOY_U, 116), (X, 56)]], arcs=arcs, bindings=bind, sink_cost=9)
    assert stream_rows(r.stream)[-1] == (2, 13, 1, 0, 1, 9, 0, 0) and r.arcs[(13, 1)] == (0, 1, 9, 0)
    assert r.stats == stats(tasks=1, arcs_added=2, unsched_added=1, records=3)
    # after a preemptive commit the task still has the arc: its cost moves, no unit does
    r = refresh([16], [[(TOY_U, 300), (X, 56)]], bindings=bind)
    assert stream_rows(r.stream) == [(3, 16, 13, 0, 1, 300, 116, 0)] and r.stats["unsched_updates"] == 0


def test_toy_the_three_parts_of_the_stream():
    arcs = evicted(17, evicted(16))
    tasks = [18, 17, 14, 16]
    lists = [MIXED, [(X, 1), (TOY_U, 2)], [(M1, 8), (TOY_U, 114), (R1, 5)], [(TOY_U, 3)]]
    r = refresh(tasks, lists, arcs=arcs, bindings={14: 9, 15: 9})
    rows = stream_rows(r.stream)
    slot = {k: i for i, k in enumerate(arcs)}
    held = [(s, d) for kind, s, d, *_ in rows[:4]]
    assert held == sorted(held, key=slot.get) and set(held) == {(14, X), (18, X), (14, M1), (18, M1)}
    assert [(kind, s, d) for kind, s, d, *_ in rows[4:9]] == [(2, 18, M3), (2, 17, X), (2, 17, 13), (2, 14, R1), (2, 16, 13)]
    assert rows[9:] == [(3, 13, 1, 0, 8, 0, 0, 0)]
    assert r.stats == stats(tasks=4, arcs_added=5, cost_updates=2, arcs_unchanged=3, arcs_removed=2, unsched_updates=1,
                            records=10)
    assert r.stats["records"] == sum(r.stats[f] for f in ("arcs_added", "cost_updates", "arcs_removed",
                                                          "unsched_updates", "unsched_added"))


# ---- the stream against the store semantics ---------------------------------------------
def replay(ntype, supply, alive, before: dict, r: Refresh):
    nodes = {i: [int(supply[i - 1]), int(ntype[i - 1])] for i in alive}
    low3 = {k: a[:3] for k, a in before.items()}
    apply_deltas_to_arcs(nodes, low3, r.stream)
    assert low3 == {k: a[:3] for k, a in r.arcs.items()}
    pairs = list(zip(r.stream["src"].tolist(), r.stream["dst"].tolist()))
    assert len(pairs) == len(set(pairs))            # nothing is superseded


@pytest.mark.parametrize("case", range(4))
def test_the_stream_reproduces_the_table_on_the_toy(case):
    arcs = evicted(16)
    if case == 3:
        del arcs[(13, 1)]
    tasks, lists, kw = [([18], [MIXED], {}), ([18, 14], [MIXED, [(P1, 1)]], dict(flags=KEEP_UNLISTED)),
                        ([16, 19, 15], [[(TOY_U, 1), (M2, 4)], [], [(TOY_U, 115), (M1, 2)]], {}),
                        ([16], [[(TOY_U, 5), (R1, 1)]], {})][case]
    r = refresh(tasks, lists, arcs=arcs, bindings={14: 9, 15: 9, 17: 11}, sink_cost=17, **kw)
    replay(TOY_NTYPE, TOY_SUPPLY, range(1, 20), arcs, r)
    assert r.stats["records"] == r.stream.shape[0] > 0


@pytest.mark.parametrize("preemption", [False, True], ids=["pinned", "preemptive"])
def test_the_stream_reproduces_the_table_on_a_churn_graph(preemption):
    """Three rounds of a small cell; then every fourth live task is refreshed (two costs change,
    one head is new, one held arc is dropped) and, pinned, three running tasks are evicted (their
    running arc is gone, they are unbound) and listed with their arcs. The aggregators'
    capacities are the tasks with an arc into each, and the oracle finds the result feasible."""
    cell = churn.Cell(40, 8, 2, 6, 3, preemption=preemption, preemption_cost=150)
    for rnd in range(3):
        g = cell.graph()
        st, _, _, fl = ko.cost_scaling(g)
        assert st == 0
        cell.step(ko.bfs_mapping(g, fl), 6, 8, age_cost=0, seed=100 + rnd)
    g = cell.graph()
    before = {k: a for k, a in arc_table(g).items() if a[1] > 0}
    alive = {i + 1 for i in range(g.n) if i + 1 < cell.TASK0 or g.ntype[i] == 1}
    aggs = [cell.U0 + j for j in range(cell.J)]
    bind = {int(s): int(d) for (s, d), a in before.items() if a[3] == 1}
    gone = [] if preemption else sorted(bind)[:3]
    for t in gone:
        del before[(t, bind.pop(t))]
    waiting = sorted(t for t in alive if g.ntype[t - 1] == 1 and t not in bind and t not in gone)
    tasks, lists = [], []
    for t in waiting[::4] + gone:
        if t in gone:
            sl = t - cell.TASK0
            lst = list(dict(zip(cell.adst[sl].tolist(), cell.acost[sl].tolist())).items())
        else:
            mine = [(d, a[2]) for (s, d), a in before.items() if s == t]
            agg = [x for x in mine if x[0] in aggs]
            rest = [x for x in mine if x[0] not in aggs]
            new = next(m for m in range(cell.MACH0, cell.MACH0 + cell.M) if m not in dict(mine))
            lst = agg + [(d, c + 7) for d, c in rest[:2]] + rest[3:] + [(new, 11)]
        tasks.append(t)
        lists.append(lst)
    r = refresh_reference(g.ntype, before, tasks, lists, bind, aggs)
    replay(g.ntype, g.supply, alive, before, r)
    assert r.stats["cost_updates"] > 0 and r.stats["arcs_removed"] > 0 and r.stats["arcs_added"] > 0
    assert (r.stats["unsched_updates"] + r.stats["unsched_added"] > 0) == bool(gone)
    for u in aggs:
        assert r.arcs.get((u, cell.SINK), (0, 0))[1] == sum(1 for (s, d) in r.arcs if d == u)
    assert ko.cost_scaling(table_graph(g.ntype, g.supply, r.arcs))[0] == 0


# ---- refusals ---------------------------------------------------------------------------
def test_refusals_of_the_rule_change_nothing():
    table = dict(TOY_ARCS)
    alive = set(range(1, 20)) - {17}
    one = [(X, 1)]

    def refused(err, names, tasks, lists, **kw):
        kw.setdefault("ids", U)
        with pytest.raises(err) as e:
            refresh(tasks, lists, arcs=table, alive=alive, **kw)
        assert e.value.args[:len(names)] == tuple(names)
        assert table == TOY_ARCS and list(table) == list(TOY_ARCS)

    for bad in (0, 17, 13, 40):                                              # 0, dead, no task, beyond the graph
        refused(InvalidRefresh, [bad], [18, bad, 0], [one, one, one])
    refused(InvalidRefresh, [18], [18, 19, 18, 0], [one, one, one, one])     # listed a second time
    for head in (0, 17, 14, 40):                                             # 0, dead, a task, beyond the graph
        refused(InvalidRefresh, [19, head], [18, 19], [one, [(X, 1), (head, (1 << 40) + 1)], ])   # the head before the cost
    refused(InvalidRefresh, [19, M1], [18, 19], [one, [(M1, 1), (X, 1), (M1, 1)]])           # a held head twice
    refused(InvalidRefresh, [19, M3], [18, 19], [one, [(M3, 1), (X, 1), (M3, 2)]])           # an absent head twice
    refused(InvalidRefresh, [18, X], [18, 19], [[(X, 1), (X, 1 << 41)], [(0, 1)]])           # the first arc in input order
    refused(OutOfRange, [19], [18, 19], [one, [(X, (1 << 40) + 1)]])
    refused(OutOfRange, [18], [18], [[(X, -(1 << 40) - 1)]])
    assert refresh([18], [[(X, 1 << 40), (M1, -(1 << 40))]], arcs=table, alive=alive).stats["cost_updates"] == 2
    refused(OutOfRange, [None], [18], [one], sink_cost=(1 << 40) + 1)
    refused(OutOfRange, [None], [18], [one], sink_cost=-(1 << 40) - 1)
    refused(InvalidRefresh, [19], [18, 19], [one, [(TOY_U, 1), (8, 2)]], ids=[TOY_U, 8])      # two aggregators, listed
    refused(InvalidRefresh, [19], [18, 19], [one, [(8, 2)]], ids=[TOY_U, 8])                  # one held, one listed
    refused(InvalidRefresh, [None], [18], [one], flags=2)
    refused(InvalidRefresh, [None], [18], [one], flags=KEEP_UNLISTED | 4)
    # the NULL rule cannot see a drained U: an unbound task is refused, a bound one passes
    drained = {k: a for k, a in TOY_ARCS.items() if k != (13, 1)}
    with pytest.raises(InvalidRefresh) as e:
        refresh([14, 18], [[(TOY_U, 1)], [(TOY_U, 1), (X, 1)]], arcs=drained, ids=None)
    assert e.value.args[0] == 18
    gone = evicted(14, drained)
    gone[(14, P1)] = (1, 1, 0, 1)                                            # pinned: the running arc alone
    assert refresh([14], [[]], arcs=gone, ids=None).stats == stats(tasks=1)
    with pytest.raises(InvalidRefresh):
        refresh([14], [[]], arcs=gone, ids=None, bindings={})                # the same task unbound
    assert refresh([18], [[(X, 58)]], arcs=evicted(18), ids=U, bindings={}).stats["arcs_added"] == 1   # ids: legal
    # a gain needs exactly one sink
    two = TOY_NTYPE + [3]
    with pytest.raises(InvalidRefresh) as e:
        refresh_reference(two, evicted(16), [16], [[(TOY_U, 1)]], {}, U)
    assert e.value.args[0] is None
    assert refresh_reference(two, evicted(16), [16], [[(X, 1)]], {}, U).stats["records"] == 1


# ---- the library and the binding ----------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_update_stats %zu\n", sizeof(ks_update_stats));
""" + "".join(f"  P(ks_update_stats, {f});\n" for f in STAT_KEYS + ("reserved",)) + r"""
  printf("abi %d\n", KSMCMF_ABI_VERSION);
  printf("keep %d\n", KS_UPDATE_KEEP_UNLISTED);
  return 0;
}
"""


def test_update_stats_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_update_stats"] == C.sizeof(native.KsUpdateStats) == 96
    assert [f for f, _ in native.KsUpdateStats._fields_] == list(STAT_KEYS) + ["reserved"]
    for f in STAT_KEYS + ("reserved",):
        assert getattr(native.KsUpdateStats, f).offset == out[f"ks_update_stats.{f}"], f
    assert tuple(native.KsUpdateStats().as_dict()) == STAT_KEYS
    assert out["keep"] == native.KS_UPDATE_KEEP_UNLISTED == KEEP_UNLISTED == 1
    assert out["abi"] == native.ABI_VERSION == 5          # an entry point and a struct were added, nothing moved


def test_library_exports_the_entry_point():
    """Fails on a library built before ks_update_tasks."""
    lib = native.load(build_if_missing=True)
    assert "ks_update_tasks" in native.EXPORTED_SYMBOLS
    assert hasattr(lib, "ks_update_tasks")
    assert lib.ks_abi_version() == 5


def test_binding_has_update_tasks():
    assert callable(getattr(native.Context, "update_tasks", None))
    assert Refresh._fields == ("arcs", "stream", "stats")
