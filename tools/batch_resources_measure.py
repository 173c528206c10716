#!/usr/bin/env python3
"""The resource side of a batch round on config 5: the device calls against host-built streams.

64 cells of config 2 (seeds 1000..1063), solved and committed (pinned, then preemptive). In every
cell one machine leaves (machine g mod M of cell g, with its PU) and comes back beneath its rack
under the ids it had. Per repeat a FRESH batch is loaded, solved and committed; a twin batch is
loaded with the committed graphs for the host path (two solves may pick different optima). One
warm-up repeat is dropped; the medians go to profiles/batch_resources_config5.json:

  a   one ks_batch_remove_resources, then one ks_batch_add_resources (buffers sized beforehand,
      no probe; the lists are what a caller knows without reading the device: its topology)
  b   two ks_batch_apply_deltas calls with the identical records, prebuilt outside the timer
  c   building those records in numpy from ks_batch_get_graph copies of every cell (the read
      and the construction, for the removal and, on the graph after it, for the growth)

After a pinned commit a full machine has lost the arc into its PU, so the roots name the machine
and its PU; after a preemptive commit the machine alone. --check compares every cell of a with b
after both steps, arc for arc.

    python tools/batch_resources_measure.py [--cells 64] [--repeats 5] [--out FILE] [--check]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ksched_amd import churn, gen, native  # noqa: E402
from tools.remove_measure import build_stream  # noqa: E402

SPARE = 64
D = native.DELTA_DT
MACHINE, PU = 4, 2


def arc_of(arcs, s, d):
    i = np.nonzero((arcs["src"] == s) & (arcs["dst"] == d))[0]
    return arcs[i[0]] if i.size else None


def add_stream(cell, before, after, mid, pid):
    """The records that bring machine mid and its PU pid back beneath their rack: the nodes, the
    PU's arc into the sink, the arcs of the new subtree with the PU's slots, and the slots added
    to the arc above the rack (re-created where the graph no longer holds it)."""
    rack = cell.RACK0 + (mid - cell.MACH0) % cell.R
    sink_arc, m_arc, r_arc = arc_of(before, pid, cell.SINK), arc_of(before, mid, pid), arc_of(before, rack, mid)
    S = int(sink_arc["cap"])
    costs = [0 if a is None else int(a["cost"]) for a in (sink_arc, r_arc, m_arc)]
    out = np.zeros(6, D)
    out["kind"][:2], out["id"][:2], out["type"][:2] = native.KS_ADD_NODE, (mid, pid), (MACHINE, PU)
    out["kind"][2:5] = native.KS_ADD_ARC
    out["src"][2:5], out["dst"][2:5], out["cap"][2:5], out["cost"][2:5] = (pid, rack, mid), (cell.SINK, mid, pid), S, costs
    top = arc_of(after, cell.X, rack)
    x = out[5]
    x["src"], x["dst"] = cell.X, rack
    if top is None:
        x["kind"], x["cap"] = native.KS_ADD_ARC, S
    else:
        x["kind"], x["type"], x["low"], x["cap"] = native.KS_UPDATE_ARC, top["type"], top["low"], int(top["cap"]) + S
        x["cost"] = x["old_cost"] = top["cost"]
    nodes = [(mid, MACHINE, 0, 0), (pid, PU, S, costs[0])]
    edges = [(rack, mid, costs[1], native.KS_RES_TREE), (mid, pid, costs[2], native.KS_RES_TREE),
             (cell.X, rack, 0, native.KS_RES_TREE)]
    return out, (nodes, edges)


def sorted_graph(b, g):
    return tuple(np.sort(x, order=list(x.dtype.names)).tobytes() for x in b.get_graph(g))


def one_repeat(args, preemptive):
    T, M, R, J, _ = gen.CONFIGS["config2"]
    n = args.cells
    cells = [churn.Cell(T, M, R, J, 1000 + i) for i in range(n)]
    row = {}
    a, b = native.Batch(devices=[0]), native.Batch(devices=[0])
    try:
        for x in (a, b):
            x.reserve(SPARE)
        a.load([c.graph() for c in cells])
        a.solve()
        deltas, _ = a.commit_preemptive(preemption=150) if preemptive else a.commit_schedule()
        b.load_arrays([a.get_graph(g) for g in range(n)])
        mach = [c.MACH0 + g % c.M for g, c in enumerate(cells)]
        pus = [c.PU0 + g % c.M for g, c in enumerate(cells)]
        # (c) the removal's records from the host's copies
        t0 = time.perf_counter()
        snap = [b.get_graph(g) for g in range(n)]
        t1 = time.perf_counter()
        rm_streams = []
        for g in range(n):
            nodes, arcs = snap[g]
            ntype = np.zeros(int(nodes["id"].max()), np.int32)
            ntype[nodes["id"].astype(np.int64) - 1] = nodes["type"]
            mine = deltas["graph"] == g
            rm_streams.append(build_stream(ntype, arcs, [mach[g], pus[g]], deltas["task"][mine], deltas["pu"][mine],
                                           preemptive)[0])
        t2 = time.perf_counter()
        row["get_graph_ms"], row["build_remove_ms"] = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
        # (b) ks_batch_apply_deltas of the removal
        t0 = time.perf_counter()
        b.apply_deltas(rm_streams)
        t1 = time.perf_counter()
        row["apply_remove_ms"] = 1e3 * (t1 - t0)
        # (c) the growth's records from the copies after the removal
        t0 = time.perf_counter()
        after = [b.get_graph(g) for g in range(n)]
        t1 = time.perf_counter()
        built = [add_stream(cells[g], snap[g][1], after[g][1], mach[g], pus[g]) for g in range(n)]
        t2 = time.perf_counter()
        row["get_graph_ms"] += 1e3 * (t1 - t0)
        row["build_add_ms"] = 1e3 * (t2 - t1)
        t0 = time.perf_counter()
        b.apply_deltas([s for s, _ in built])
        t1 = time.perf_counter()
        row["apply_add_ms"] = 1e3 * (t1 - t0)
        row["host_records"] = int(sum(s.shape[0] for s in rm_streams) + sum(s.shape[0] for s, _ in built))
        # (a) the two device calls: lists and buffers outside the timer
        flags = native.KS_REMOVE_RESOURCE_CAPS | (native.KS_REMOVE_PREEMPTIVE if preemptive else 0)
        ls = (native.KsBatchResList * n)()
        roots = [np.asarray([mach[g]] if preemptive else [mach[g], pus[g]], np.uint64) for g in range(n)]
        for g in range(n):
            ls[g].roots, ls[g].k = roots[g].ctypes.data, roots[g].shape[0]
        rm = np.zeros(2 * n + 8, np.uint64)
        ev = np.zeros(int(deltas.shape[0]) + 8, native.BATCH_DELTA_DT)
        off = np.zeros(n + 1, np.uintp)
        nr, ne, st = C.c_size_t(), C.c_size_t(), native.KsRemoveStats()
        t0 = time.perf_counter()
        rc = a._L.ks_batch_remove_resources(a._h, flags, n, ls, rm.ctypes.data, rm.shape[0], C.byref(nr), off.ctypes.data,
                                            ev.ctypes.data, ev.shape[0], C.byref(ne), C.byref(st))
        t1 = time.perf_counter()
        a._check(rc)
        per = [x for _, x in built]
        t2 = time.perf_counter()
        gst = a.add_resources(per)
        t3 = time.perf_counter()
        row |= {"remove_ms": 1e3 * (t1 - t0), "add_ms": 1e3 * (t3 - t2), "nodes_removed": int(nr.value),
                "tasks_evicted": int(ne.value), "records": int(st.records) + gst["records"]}
        if args.check:
            for g in range(n):
                assert sorted_graph(a, g) == sorted_graph(b, g), f"cell {g}: the device calls and the host streams disagree"
    finally:
        a.close()
        b.close()
    row["a_total_ms"] = row["remove_ms"] + row["add_ms"]
    row["b_total_ms"] = row["apply_remove_ms"] + row["apply_add_ms"]
    row["c_total_ms"] = row["get_graph_ms"] + row["build_remove_ms"] + row["build_add_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_resources_config5.json"))
    args = ap.parse_args()
    out = {"workload": f"config5 batch: {args.cells} config-2 cells (seeds 1000..{999 + args.cells}) after a solve and a "
                       f"commit; one machine per cell leaves and comes back; medians of {args.repeats} repeats after one "
                       f"warm-up, fresh batches per repeat",
           "checked_equal": bool(args.check)}
    for mode in ("pinned", "preemptive"):
        runs = [one_repeat(args, mode == "preemptive") for _ in range(args.repeats + 1)][1:]
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        out[mode] = {"a_two_device_calls": {k: med[k] for k in ("remove_ms", "add_ms", "a_total_ms", "records",
                                                                 "nodes_removed", "tasks_evicted")},
                     "b_apply_identical_records": {k: med[k] for k in ("apply_remove_ms", "apply_add_ms", "b_total_ms",
                                                                        "host_records")},
                     "c_build_records_on_host": {k: med[k] for k in ("get_graph_ms", "build_remove_ms", "build_add_ms",
                                                                      "c_total_ms")},
                     "a_beats_b": med["a_total_ms"] < med["b_total_ms"],
                     "a_beats_b_plus_c": med["a_total_ms"] < med["b_total_ms"] + med["c_total_ms"],
                     "runs": runs}
        print(json.dumps({"commit": mode, **{k: v for k, v in out[mode].items() if k != "runs"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
