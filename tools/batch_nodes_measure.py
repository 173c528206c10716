#!/usr/bin/env python3
"""Class and resource arcs of a batch round on config 5: the device call against host-built streams.

64 cells of config 2 (seeds 1000..1063), solved and committed (pinned, then preemptive). In every
cell every rack → machine arc is re-costed with an explicit capacity (the machine's room under the
commit's capacity rule: its slots, minus its bound tasks when pinned) and every PU → sink arc is
re-costed with KS_CAP_KEEP; the new costs follow the load the commit's deltas report. Per repeat a
FRESH batch is loaded, solved and committed; a twin batch is loaded with the committed graphs for
the host path (two solves may pick different optima). One warm-up repeat is dropped; the medians go
to profiles/batch_nodes_config5.json:

  a   one ks_batch_update_nodes (the lists are what a caller knows without reading the device: its
      topology, its slots and the bindings; they are packed outside the timer)
  b   one ks_batch_apply_deltas call on the UPDATE_ARC records of the same changes, prebuilt outside
      the timer
  c   building those records in numpy from ks_batch_get_graph copies of every cell (the read and
      the construction): an UPDATE_ARC record carries the arc's type, lower bound and old cost, which
      only the store knows after a commit

--check compares every cell of a with b afterwards, arc for arc.

    python tools/batch_nodes_measure.py [--cells 64] [--repeats 5] [--out FILE] [--check]
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

SPARE = 64
D = native.DELTA_DT
RACK_BASE = 7


def sorted_graph(b, g):
    return tuple(np.sort(x, order=list(x.dtype.names)).tobytes() for x in b.get_graph(g))


def load_of(cell, deltas, g):
    """Bound tasks per machine index of cell g, from the commit's deltas (a fresh batch: every PLACE)."""
    mine = deltas[deltas["graph"] == g]
    return np.bincount(mine["pu"].astype(np.int64) - cell.PU0, minlength=cell.M)[:cell.M]


def caller_lists(cell, load, preemptive):
    """What the caller lists for one cell: (nodes, arc_off, dst, cost, cap) of ks_update_nodes."""
    k = np.arange(cell.M, dtype=np.int64)
    room = cell.slots.astype(np.int64) - (0 if preemptive else load)
    order = np.argsort(cell.rack_of, kind="stable")                 # rack by rack
    per_rack = np.bincount(cell.rack_of, minlength=cell.R)
    nodes = np.concatenate([cell.RACK0 + np.arange(cell.R), cell.PU0 + k]).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(per_rack), cell.M + 1 + k]).astype(np.uint64)
    dst = np.concatenate([cell.MACH0 + order, np.full(cell.M, cell.SINK)]).astype(np.uint64)
    cost = np.concatenate([RACK_BASE + load[order], load // 2]).astype(np.int64)
    cap = np.concatenate([room[order].astype(np.uint64), np.full(cell.M, native.KS_CAP_KEEP, np.uint64)])
    return nodes, off, dst, cost, cap


def host_stream(cell, arcs, load):
    """The UPDATE_ARC records of the same changes from a copy of the cell's arcs (held arcs only: an
    arc into a full machine went with the pinned commit and is listed with capacity 0, no record)."""
    s, d = arcs["src"].astype(np.int64), arcs["dst"].astype(np.int64)
    rm = (s >= cell.RACK0) & (s < cell.RACK0 + cell.R) & (d >= cell.MACH0) & (d < cell.MACH0 + cell.M)
    ps = (s >= cell.PU0) & (s < cell.PU0 + cell.M) & (d == cell.SINK)
    pick = np.nonzero(rm | ps)[0]
    out = np.zeros(pick.shape[0], D)
    a = arcs[pick]
    out["kind"] = native.KS_UPDATE_ARC
    for f in ("src", "dst", "low", "cap", "type"):
        out[f] = a[f]
    out["old_cost"] = a["cost"]
    is_rm = rm[pick]
    out["cost"] = np.where(is_rm, RACK_BASE + load[np.clip(d[pick] - cell.MACH0, 0, cell.M - 1)],
                           load[np.clip(s[pick] - cell.PU0, 0, cell.M - 1)] // 2)
    return out


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
        loads = [load_of(cells[g], deltas, g) for g in range(n)]
        # (c) the records from the host's copies
        t0 = time.perf_counter()
        snap = [b.get_graph(g) for g in range(n)]
        t1 = time.perf_counter()
        streams = [host_stream(cells[g], snap[g][1], loads[g]) for g in range(n)]
        t2 = time.perf_counter()
        row["get_graph_ms"], row["build_ms"] = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
        # (b) ks_batch_apply_deltas on the prebuilt stream
        t0 = time.perf_counter()
        b.apply_deltas(streams)
        t1 = time.perf_counter()
        row["apply_ms"] = 1e3 * (t1 - t0)
        row["host_records"] = int(sum(s.shape[0] for s in streams))
        # (a) the device call: lists packed outside the timer
        ls, keep = native.pack_node_lists(n, [caller_lists(cells[g], loads[g], preemptive) for g in range(n)])
        st = native.KsNodeStats()
        t0 = time.perf_counter()
        rc = a._L.ks_batch_update_nodes(a._h, 0, n, ls, C.byref(st))
        t1 = time.perf_counter()
        a._check(rc)
        del keep
        row |= {"update_nodes_ms": 1e3 * (t1 - t0), "records": int(st.records), "listed_arcs": int(
            st.arcs_added + st.arcs_updated + st.arcs_unchanged + st.arcs_skipped + st.arcs_zeroed),
                "arcs_added": int(st.arcs_added), "arcs_zeroed": int(st.arcs_zeroed), "arcs_removed": int(st.arcs_removed)}
        if args.check:
            for g in range(n):
                assert sorted_graph(a, g) == sorted_graph(b, g), f"cell {g}: the device call and the host stream disagree"
    finally:
        a.close()
        b.close()
    row["a_total_ms"] = row["update_nodes_ms"]
    row["b_total_ms"] = row["apply_ms"]
    row["c_total_ms"] = row["get_graph_ms"] + row["build_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_nodes_config5.json"))
    args = ap.parse_args()
    out = {"workload": f"config5 batch: {args.cells} config-2 cells (seeds 1000..{999 + args.cells}) after a solve and a "
                       f"commit; every rack -> machine arc re-costed with an explicit capacity, every PU -> sink arc "
                       f"with KS_CAP_KEEP; medians of {args.repeats} repeats after one warm-up, fresh batches per repeat",
           "checked_equal": bool(args.check)}
    for mode in ("pinned", "preemptive"):
        runs = [one_repeat(args, mode == "preemptive") for _ in range(args.repeats + 1)][1:]
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        out[mode] = {"a_one_device_call": {k: med[k] for k in ("update_nodes_ms", "a_total_ms", "records", "listed_arcs",
                                                                "arcs_added", "arcs_zeroed", "arcs_removed")},
                     "b_apply_prebuilt_records": {k: med[k] for k in ("apply_ms", "b_total_ms", "host_records")},
                     "c_build_records_on_host": {k: med[k] for k in ("get_graph_ms", "build_ms", "c_total_ms")},
                     "a_beats_b": med["a_total_ms"] < med["b_total_ms"],
                     "a_beats_b_plus_c": med["a_total_ms"] < med["b_total_ms"] + med["c_total_ms"],
                     "runs": runs}
        print(json.dumps({"commit": mode, **{k: v for k, v in out[mode].items() if k != "runs"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
