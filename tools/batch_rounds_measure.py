#!/usr/bin/env python3
"""Batch rounds on config 5: what a scheduling round of the 64-cell batch costs.

64 cells of config 2 (seeds 1000..1063), each driven by its own churn.Cell at 5 %
churn (5 % of its tasks complete, as many arrive). Per variant a FRESH batch is loaded
and solved, one warm-up round runs untimed, then five rounds are timed; the medians go
to profiles/batch_rounds_config5.json:

  a   ks_batch_apply_deltas + a warm solve (warm_start 1), all 64 cells changed
  b   the same with only 8 of the 64 cells changed (cells 0, 8, ..., 56)
  c   what a caller had to do before the batch had rounds: ks_batch_load of the 64
      updated graphs + a cold solve (the graphs are built outside the timer)

The gather between rounds feeds the cells and is not timed. Every round's per-cell
costs are checked against the CPU oracle with --check (slow: 64 oracle solves a round).

    python tools/batch_rounds_measure.py [--cells 64] [--rounds 5] [--out FILE] [--check]
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

SPARE = 512   # ids reserved per cell: a config-2 cell (12,127 nodes) stays under the cell solver's LDS limit


def mappings(cells, pu):
    out = []
    for g, cell in enumerate(cells):
        graph = cell.graph()
        tasks = np.nonzero(graph.ntype == 1)[0] + 1
        out.append({int(t): int(p) for t, p in zip(tasks, pu[g]) if p})
    return out


def check(cells, cost, flow, which):
    from oracle import ko
    for g in which:
        st, c, f, _ = ko.cost_scaling(cells[g].graph())
        assert st == 0 and (int(cost[g]), int(flow[g])) == (c, f), f"cell {g}: {cost[g]}/{flow[g]} vs {c}/{f}"


def run_delta_rounds(args, changed, label):
    """Variants a and b: resident batch, apply + warm solve per round."""
    T, M, R, J, _ = gen.CONFIGS["config2"]
    cells = [churn.Cell(T, M, R, J, 1000 + i) for i in range(args.cells)]
    b = native.Batch(devices=[0], warm_start=1)
    rows = []
    try:
        b.reserve(SPARE)
        b.load([c.graph() for c in cells])
        b.solve()
        maxt = T + SPARE
        for rnd in range(args.rounds + 1):
            pu, _, _ = b.gather(maxt)
            mps = mappings(cells, pu)
            streams = [cells[g].step(mps[g], done=T // 20, arrive=T // 20) if g in changed else None
                       for g in range(args.cells)]
            t0 = time.perf_counter()
            b.apply_deltas(streams)
            t1 = time.perf_counter()
            r = b.solve()[0]
            t2 = time.perf_counter()
            if args.check:
                _, cost, flow = b.gather(maxt)
                check(cells, cost, flow, changed)
            row = {"round": rnd, "apply_ms": 1e3 * (t1 - t0), "solve_ms": 1e3 * (t2 - t1),
                   "total_ms": 1e3 * (t2 - t0), "cells_run": r.raw["cells_run"], "cells": r.raw["cells"],
                   "solver": r.raw["solver"], "rebuilt": r.raw["rebuilt"], "warm_started": r.raw["warm_started"],
                   "records": int(sum(0 if s is None else s.shape[0] for s in streams))}
            print(f"{label} round {rnd}: {row}", file=sys.stderr)
            if rnd:                      # round 0 is the warm-up
                rows.append(row)
    finally:
        b.close()
    return rows


def run_reload_rounds(args):
    """Variant c: every round reloads the 64 updated graphs and solves cold."""
    T, M, R, J, _ = gen.CONFIGS["config2"]
    cells = [churn.Cell(T, M, R, J, 1000 + i) for i in range(args.cells)]
    b = native.Batch(devices=[0], warm_start=0)
    rows = []
    try:
        b.load([c.graph() for c in cells])
        b.solve()
        for rnd in range(args.rounds + 1):
            pu, _, _ = b.gather(T + SPARE)
            mps = mappings(cells, pu)
            for g, cell in enumerate(cells):
                cell.step(mps[g], done=T // 20, arrive=T // 20)
            graphs = [c.graph() for c in cells]          # prebuilt outside the timer
            arrs = [native.graph_arrays(g) for g in graphs]
            t0 = time.perf_counter()
            b.load_arrays(arrs)
            t1 = time.perf_counter()
            r = b.solve()[0]
            t2 = time.perf_counter()
            if args.check:
                _, cost, flow = b.gather(T + SPARE)
                check(cells, cost, flow, range(args.cells))
            row = {"round": rnd, "load_ms": 1e3 * (t1 - t0), "solve_ms": 1e3 * (t2 - t1),
                   "total_ms": 1e3 * (t2 - t0), "cells_run": r.raw["cells_run"], "solver": r.raw["solver"]}
            print(f"c round {rnd}: {row}", file=sys.stderr)
            if rnd:
                rows.append(row)
    finally:
        b.close()
    return rows


def med(rows, key):
    return statistics.median(r[key] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_rounds_config5.json"))
    args = ap.parse_args()
    every = set(range(args.cells))
    some = set(range(0, args.cells, max(1, args.cells // 8)))
    a = run_delta_rounds(args, every, "a")
    bb = run_delta_rounds(args, some, "b")
    c = run_reload_rounds(args)
    out = {
        "workload": f"config5 batch: {args.cells} config-2 cells (seeds 1000..{999 + args.cells}), 5 % churn per "
                    f"round, medians of {args.rounds} rounds after one warm-up, fresh batch per variant",
        "a_all_cells_changed": {"apply_ms": med(a, "apply_ms"), "solve_ms": med(a, "solve_ms"),
                                "total_ms": med(a, "total_ms"), "rounds": a},
        "b_8_of_64_changed": {"changed": sorted(some), "apply_ms": med(bb, "apply_ms"),
                              "solve_ms": med(bb, "solve_ms"), "total_ms": med(bb, "total_ms"), "rounds": bb},
        "c_reload_and_cold_solve": {"load_ms": med(c, "load_ms"), "solve_ms": med(c, "solve_ms"),
                                    "total_ms": med(c, "total_ms"), "rounds": c},
    }
    out["a_beats_c"] = out["a_all_cells_changed"]["total_ms"] < out["c_reload_and_cold_solve"]["total_ms"]
    out["b_over_a"] = out["b_8_of_64_changed"]["total_ms"] / out["a_all_cells_changed"]["total_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)} |
                     {k: {kk: vv for kk, vv in v.items() if kk != "rounds"} for k, v in out.items()
                      if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
