#!/usr/bin/env python3
"""The task side of a batch round on config 5: the device calls against host-built streams.

64 cells of config 2 (seeds 1000..1063). Per round and cell 5 % of the live tasks complete, as
many arrive on the ids just freed (five arcs each: the job's aggregator, the cluster node, a rack,
two machines), and 5 % of the remaining tasks are refreshed (every held arc re-costed by +1). The
choice is seeded per (cell, round) and does not depend on the solver's mapping, so the variants go
through identical graphs. Per variant a FRESH batch is loaded and solved, one warm-up round runs
untimed, then five rounds are timed, with a cold solve (untimed) between rounds; the medians go to
profiles/batch_tasks_config5.json:

  a   ks_batch_complete_tasks + ks_batch_add_tasks + ks_batch_update_tasks (the lists are built
      outside the timer: they are what a caller knows without reading the device, except the
      refreshed tasks' held heads, which the caller's cost model produces)
  b   three ks_batch_apply_deltas calls with the identical records, prebuilt outside the timer
  c   building those records on the host from ks_batch_get_graph of every cell (numpy)

--check compares every cell of variant a with variant b after every round, arc for arc.

    python tools/batch_tasks_measure.py [--cells 64] [--rounds 5] [--out FILE] [--check]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ksched_amd import churn, gen, native  # noqa: E402

SPARE = 512
SINK_COST = 0
D = native.DELTA_DT


class Plan:
    """One cell's round: who completes, who arrives with which arcs, who is refreshed."""

    def __init__(self, cell, live, rnd, g):
        rng = np.random.default_rng(1_000_003 * g + rnd)
        k = max(1, live.shape[0] // 20)
        order = rng.permutation(live.shape[0])
        self.done = np.sort(live[order[:k]]).astype(np.uint64)
        self.refresh = np.sort(live[order[k:2 * k]]).astype(np.uint64)
        self.new = self.done.copy()                       # the freed ids come back
        t = self.new.astype(np.int64)
        self.new_dst = np.stack([cell.U0 + (t + rnd) % cell.J, np.full_like(t, cell.X), cell.RACK0 + t % cell.R,
                                 cell.MACH0 + t % cell.M, cell.MACH0 + (t + 7) % cell.M], axis=1).astype(np.uint64)
        same = self.new_dst[:, 3] == self.new_dst[:, 4]
        self.new_dst[same, 4] = (cell.MACH0 + (t[same] + 1) % cell.M).astype(np.uint64)
        self.new_cost = (40 * np.arange(1, 6)[None, :] + (t % 13)[:, None]).astype(np.int64)


def records(n):
    return np.zeros(n, D)


def arc_records(kind, src, dst, low, cap, cost, old, typ):
    r = records(len(src))
    r["kind"], r["src"], r["dst"], r["low"], r["cap"], r["cost"], r["old_cost"], r["type"] = \
        kind, src, dst, low, cap, cost, old, typ
    return r


def agg_records(cell, caps, delta, present):
    """U_j → sink records for the aggregators whose capacity moves by delta (a capacity of 0 deletes)."""
    j = np.nonzero(delta)[0]
    new = caps[j] + delta[j]
    kind = np.where(present[j], native.KS_UPDATE_ARC, native.KS_ADD_ARC)
    return arc_records(kind, cell.U0 + j, np.full(j.shape[0], cell.SINK), 0, new, SINK_COST, SINK_COST, 0), new, j


def host_streams(cell, arcs, plan):
    """(c): the three streams of one cell from its graph as the device holds it."""
    src, dst = arcs["src"].astype(np.int64), arcs["dst"].astype(np.int64)
    J = cell.J
    to_sink = (dst == cell.SINK) & (src >= cell.U0) & (src < cell.U0 + J)
    caps = np.zeros(J, np.int64)
    caps[src[to_sink] - cell.U0] = arcs["cap"][to_sink].astype(np.int64)
    present = caps > 0
    into_agg = (dst >= cell.U0) & (dst < cell.U0 + J)
    # complete: "r id", then the aggregators' losses
    m = into_agg & np.isin(src, plan.done.astype(np.int64))
    lost = np.bincount(dst[m] - cell.U0, minlength=J)
    rm = records(plan.done.shape[0])
    rm["kind"], rm["id"] = native.KS_REMOVE_NODE, plan.done
    ar, new, j = agg_records(cell, caps, -lost, present)
    caps[j] = new
    present = caps > 0
    s1 = np.concatenate([rm, ar])
    # add: "n id", the five arcs of each, the aggregators' gains
    k = plan.new.shape[0]
    nd = records(k)
    nd["kind"], nd["id"], nd["type"], nd["excess"] = native.KS_ADD_NODE, plan.new, 1, 1
    ta = arc_records(native.KS_ADD_ARC, np.repeat(plan.new, 5), plan.new_dst.reshape(-1), 0, 1,
                     plan.new_cost.reshape(-1), 0, 0)
    gain = np.bincount(plan.new_dst[:, 0].astype(np.int64) - cell.U0, minlength=J)
    ar, new, j = agg_records(cell, caps, gain, present)
    s2 = np.concatenate([nd, ta, ar])
    # update: every held arc of a refreshed task, re-costed
    m = np.isin(src, plan.refresh.astype(np.int64))
    s3 = arc_records(native.KS_UPDATE_ARC, arcs["src"][m], arcs["dst"][m], arcs["low"][m], arcs["cap"][m],
                     arcs["cost"][m] + 1, arcs["cost"][m], arcs["type"][m])
    return s1, s2, s3


def refresh_lists(arcs, plan):
    """The refreshed tasks' lists for variant a: their held arcs, each cost + 1 (tasks ascending)."""
    src = arcs["src"]
    m = np.isin(src, plan.refresh)
    order = np.argsort(src[m], kind="stable")
    s, d, c = src[m][order], arcs["dst"][m][order], arcs["cost"][m][order] + 1
    off = np.searchsorted(s, plan.refresh, side="left").astype(np.uint64)
    return plan.refresh, np.append(off, np.uint64(s.shape[0])), d, c


def live_tasks(nodes):
    return nodes["id"][nodes["type"] == 1].astype(np.uint64)


def run(args, variant):
    T, M, R, J, _ = gen.CONFIGS["config2"]
    cells = [churn.Cell(T, M, R, J, 1000 + i) for i in range(args.cells)]
    n = args.cells
    b = native.Batch(devices=[0])
    rows, graphs = [], []
    try:
        b.reserve(SPARE)
        b.load([c.graph() for c in cells])
        for rnd in range(args.rounds + 1):
            b.solve()
            t_g0 = time.perf_counter()
            snap = [b.get_graph(g) for g in range(n)]       # (c) times this read; (a) only plans from it
            t_g1 = time.perf_counter()
            plans = [Plan(cells[g], live_tasks(snap[g][0]), rnd, g) for g in range(n)]
            aggs = [np.arange(c.U0, c.U0 + c.J, dtype=np.uint64) for c in cells]
            row = {"round": rnd}
            if variant == "a":
                done = [p.done for p in plans]
                arrive = [(p.new, np.arange(0, 5 * p.new.shape[0] + 1, 5, dtype=np.uint64), p.new_dst.reshape(-1),
                           p.new_cost.reshape(-1)) for p in plans]
                refresh = [refresh_lists(snap[g][1], plans[g]) for g in range(n)]
                t0 = time.perf_counter()
                _, st1 = b.complete_tasks(done, resource_caps=False, unsched_ids=aggs)
                t1 = time.perf_counter()
                st2 = b.add_tasks(arrive, unsched_ids=aggs, unsched_sink_cost=SINK_COST)
                t2 = time.perf_counter()
                st3 = b.update_tasks(refresh, unsched_ids=aggs, unsched_sink_cost=SINK_COST)
                t3 = time.perf_counter()
                row |= {"complete_ms": 1e3 * (t1 - t0), "add_ms": 1e3 * (t2 - t1), "update_ms": 1e3 * (t3 - t2),
                        "total_ms": 1e3 * (t3 - t0), "records": st1["records"] + st2["records"] + st3["records"]}
            else:
                t1 = time.perf_counter()
                streams = [host_streams(cells[g], snap[g][1], plans[g]) for g in range(n)]
                t2 = time.perf_counter()
                for i in range(3):
                    b.apply_deltas([s[i] for s in streams])
                t3 = time.perf_counter()
                row |= {"get_graph_ms": 1e3 * (t_g1 - t_g0), "build_ms": 1e3 * (t2 - t1),
                        "host_ms": 1e3 * (t_g1 - t_g0 + t2 - t1), "apply_ms": 1e3 * (t3 - t2),
                        "records": int(sum(sum(x.shape[0] for x in s) for s in streams))}
            print(f"{variant} round {rnd}: {row}", file=sys.stderr)
            if rnd:
                rows.append(row)
            if args.check:
                graphs.append([tuple(np.sort(x, order=list(x.dtype.names)).tobytes() for x in b.get_graph(g))
                               for g in range(n)])
    finally:
        b.close()
    return rows, graphs


def med(rows, key):
    return statistics.median(r[key] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_tasks_config5.json"))
    args = ap.parse_args()
    a, ga = run(args, "a")
    bc, gb = run(args, "b")
    if args.check:
        for rnd, (x, y) in enumerate(zip(ga, gb)):
            for g, (p, q) in enumerate(zip(x, y)):
                assert p == q, f"round {rnd}, cell {g}: the device calls and the host streams disagree"
    out = {
        "workload": f"config5 batch: {args.cells} config-2 cells (seeds 1000..{999 + args.cells}), per cell and round "
                    f"5 % completions, as many arrivals, 5 % refreshed; medians of {args.rounds} rounds after one "
                    f"warm-up, fresh batch per variant, a cold solve between rounds",
        "a_three_device_calls": {k: med(a, k) for k in ("complete_ms", "add_ms", "update_ms", "total_ms", "records")}
                                | {"rounds": a},
        "b_apply_identical_records": {"apply_ms": med(bc, "apply_ms"), "records": med(bc, "records")},
        "c_build_records_on_host": {k: med(bc, k) for k in ("get_graph_ms", "build_ms", "host_ms")} | {"rounds": bc},
        "checked_equal": bool(args.check),
    }
    out["a_beats_b"] = out["a_three_device_calls"]["total_ms"] < out["b_apply_identical_records"]["apply_ms"]
    out["a_beats_b_plus_c"] = out["a_three_device_calls"]["total_ms"] < (
        out["b_apply_identical_records"]["apply_ms"] + out["c_build_records_on_host"]["host_ms"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "rounds"} if isinstance(v, dict) else v)
                      for k, v in out.items()}))


if __name__ == "__main__":
    main()
