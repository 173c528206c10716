#!/usr/bin/env python3
"""ks_complete_tasks against the host path it replaces, on the config-3 cell after its
first solve, a commit and a second solve: 5,000 running tasks complete
in one call, each repeat on freshly loaded contexts. Three variants: after a pinned commit
with KS_COMPLETE_RESOURCE_CAPS (slots − running), after a preemptive commit without the
flag (what the header tells such callers: no resource capacity changes), and after a
preemptive commit with it (the cost of the BFS alone).

  (a) ks_complete_tasks: wall time of the one call and its split seed / aggregator counts /
      caps / emit + apply (ks_opts.log_cycles);
  (b) the host path at its most favourable: the same records built outside the timer,
      ks_apply_deltas alone timed (wall, and the library's "store kernels + wait" share);
  (c) the construction of that stream in Python (numpy) from the host's copy of the graph:
      the aggregators' losses, the sums and the changed capacities.

After a pinned commit a full PU has lost the arc from its machine (capacity 0 removes an
arc), and config 3 fills every PU. The recipe that re-creates the arcs (ADD_ARC upserts of
the finishing tasks' parent chains, then a solve) is the caller's step before either path
and runs untimed: both paths start from the graph the store then holds. The
two paths' graphs and the bindings returned are compared after every repeat. One warm-up
repeat is dropped. Writes one JSON (medians and the raw lists).

    python tools/complete_measure.py --repeats 5 --out profiles/complete_tasks_config3.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ksched_amd import churn, gen, native  # noqa: E402
from tools.commit_measure import APPLY_RE, Stderr  # noqa: E402
from tools.remove_measure import committed, rows  # noqa: E402

COMPLETE_RE = (r"complete: (\d+) tasks, (\d+) records, seed ([\d.]+) ms, aggregator counts ([\d.]+) ms, "
               r"caps ([\d.]+) ms, emit \+ apply ([\d.]+) ms")
TASK, PU, SINK, MACHINE, INTERMEDIATE = 1, 2, 3, 4, 5
VARIANTS = {"pinned": (False, True), "preemptive": (True, False), "preemptive_caps": (True, True)}


def build_stream(ntype, arcs, done, preemptive, caps):
    """The records of the completions from a host's copy of the graph (arcs: ARC_DT in
    arc-slot order, ntype by id − 1) → stream DELTA_DT. The rule of ks_complete_tasks for a
    layered topology (PU → machine → type-0 rack → type-0 root), vectorised."""
    n = ntype.shape[0]
    src, dst = arcs["src"].astype(np.int64) - 1, arcs["dst"].astype(np.int64) - 1
    cap = arcs["cap"].astype(np.int64)
    ts, td = ntype[src], ntype[dst]
    removed = np.unique(np.asarray(done, np.int64))
    gone = np.zeros(n, bool)
    gone[removed - 1] = True
    keep = ~(gone[src] | gone[dst])
    agg = np.zeros(n, bool)
    agg[src[(td == SINK) & (ts == 0)]] = True               # the NULL rule: type-0 nodes with an arc into the sink
    lost = np.bincount(dst[gone[src] & agg[dst]], minlength=n)
    new = cap.copy()
    to_sink = keep & (td == SINK) & (lost[src] > 0)
    new[to_sink] = cap[to_sink] - lost[src[to_sink]]
    if caps:
        slots = np.zeros(n, np.int64)
        running = np.zeros(n, np.int64)
        pu_sink = keep & (td == SINK) & (ts == PU)
        slots[src[pu_sink]] = cap[pu_sink]
        run_arc = keep & (arcs["type"] == 1)
        running += np.bincount(dst[run_arc], minlength=n)
        running[ntype != PU] = 0
        for head in (PU, MACHINE, 0):                       # sums up the layers: machines, racks, the root
            up = keep & (ts != TASK) & (td == head) & (td != SINK)
            if head == 0:
                up &= slots[dst] > 0
            slots += np.bincount(src[up], weights=slots[dst[up]], minlength=n).astype(np.int64)
            running += np.bincount(src[up], weights=running[dst[up]], minlength=n).astype(np.int64)
        resarc = keep & (ts != TASK) & (td != SINK) & (np.isin(td, (PU, MACHINE, INTERMEDIATE)) |
                                                       ((td == 0) & (slots[dst] > 0)))
        new[resarc] = (slots[dst] if preemptive else slots[dst] - running[dst])[resarc]
    ch = np.nonzero(keep & (new != cap))[0]
    stream = np.zeros(removed.shape[0] + ch.shape[0], native.DELTA_DT)
    stream["kind"][:removed.shape[0]] = native.KS_REMOVE_NODE
    stream["id"][:removed.shape[0]] = removed
    x = stream[removed.shape[0]:]
    x["kind"], x["type"], x["src"], x["dst"] = native.KS_UPDATE_ARC, arcs["type"][ch], arcs["src"][ch], arcs["dst"][ch]
    x["cap"], x["cost"], x["old_cost"] = new[ch], arcs["cost"][ch], arcs["cost"][ch]
    x["low"] = np.where(new[ch] > 0, arcs["low"][ch], 0)
    return stream


def chain_upserts(cell, pus):
    """The pinned recipe's second step: ADD_ARC upserts (capacity 64: any positive one) of
    machine → PU, rack → machine and X → rack above the finishing tasks' PUs."""
    p = np.unique(np.asarray(pus, np.int64))
    k = p - cell.PU0
    m, r = cell.MACH0 + k, np.unique(cell.RACK0 + cell.rack_of[k])
    src = np.concatenate([m, cell.RACK0 + cell.rack_of[k], np.full(r.shape[0], cell.X, np.int64)])
    dst = np.concatenate([p, m, r])
    recs = np.zeros(src.shape[0], native.DELTA_DT)
    recs["kind"], recs["src"], recs["dst"], recs["cap"] = native.KS_ADD_ARC, src, dst, 64
    return recs


def one_repeat(shape, variant, count):
    preemptive, caps = VARIANTS[variant]
    out = {}
    cell = churn.Cell(*shape)
    flags = (native.KS_COMPLETE_RESOURCE_CAPS if caps else 0) | (native.KS_COMPLETE_PREEMPTIVE if preemptive and caps else 0)
    with native.Context(0, log_cycles=1) as ctx, native.Context(0, log_cycles=1) as twin:
        deltas = committed(ctx, cell, preemptive)
        order = np.argsort(deltas["task"], kind="stable")
        pick = order[::max(1, order.shape[0] // count)][:count]
        done = np.ascontiguousarray(deltas["task"][pick], np.uint64)
        if not preemptive:
            with Stderr():
                ctx.apply_deltas(chain_upserts(cell, deltas["pu"][pick]))
                ctx.solve()
        # the host path's context holds the same graph (two solves may pick different optima)
        nodes, arcs = ctx.graph()
        with Stderr():
            twin.load_arrays(nodes, arcs)
            twin.solve()
            twin.graph()   # (a download: whatever the solve left queued on the stream has run before the timer starts)
        # (c) the stream from the host's copy (downloaded outside the timer: a host keeps its own)
        ntype = np.zeros(int(nodes["id"].max()), np.int32)
        ntype[nodes["id"].astype(np.int64) - 1] = nodes["type"]
        t0 = time.perf_counter()
        stream = build_stream(ntype, arcs, done, preemptive, caps)
        t1 = time.perf_counter()
        out["stream_build_ms"] = 1e3 * (t1 - t0)
        # (b) ks_apply_deltas alone
        with Stderr() as log:
            t0 = time.perf_counter()
            twin.apply_deltas(stream)
            t1 = time.perf_counter()
        m = re.search(APPLY_RE, log.text)
        out["apply_wall_ms"] = 1e3 * (t1 - t0)
        out["apply_upload_call_ms"], out["apply_kernels_wait_ms"] = float(m.group(1)), float(m.group(3))
        out["host_records"] = int(stream.shape[0])
        # (a) the one call
        left = np.zeros(done.shape[0], np.uint64)
        st = native.KsCompleteStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_complete_tasks(ctx._h, flags, done.ctypes.data, done.shape[0], None, 0, left.ctypes.data,
                                          C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(COMPLETE_RE, log.text)
        out["complete_wall_ms"] = 1e3 * (t1 - t0)
        out["complete_seed_ms"], out["complete_agg_ms"], out["complete_caps_ms"], out["complete_apply_ms"] = (
            float(x) for x in m.groups()[2:])
        for k in ("tasks", "bound", "arcs_removed", "unsched_updates", "cap_updates", "records"):
            out[k] = int(getattr(st, k))
        if left.tolist() != deltas["pu"][pick].tolist():
            raise SystemExit(f"{variant}: the bindings returned differ from the commit's")
        if out["records"] != out["host_records"] or not (rows(ctx) == rows(twin)).all():
            raise SystemExit(f"{variant}: the two paths' graphs differ")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(gen.CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shape = gen.CONFIGS[a.config]
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats, "completions": a.tasks}
    for variant in VARIANTS:
        runs = [one_repeat(shape, variant, a.tasks) for _ in range(a.repeats + 1)][1:]   # the first: warm-up
        res[variant] = {"median": {k: statistics.median(r[k] for r in runs) for k in runs[0]}, "runs": runs}
        print(json.dumps({"config": a.config, "variant": variant, **res[variant]["median"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
