#!/usr/bin/env python3
"""ks_remove_resources against the host path it replaces, on the config-3 cell after its
first solve and a pinned commit, and the same after a preemptive
commit. Two removals, each on freshly loaded contexts per repeat: (i) 100 machines spread
over the racks, (ii) one whole rack.

  (a) ks_remove_resources: wall time of the one call (buffers sized beforehand, no probe)
      and its split mark / evict / caps / emit + apply (ks_opts.log_cycles);
  (b) the host path at its most favourable: the same records built outside the timer,
      ks_apply_deltas alone timed (wall, and the library's "store kernels + wait" share);
  (c) the construction of that stream in Python (numpy): the walk over the host's copy of
      the topology, the bindings, the sums and the changed capacities.

After a pinned commit a full machine has lost its arc into its PU and a rack's arc into
it (capacity 0 removes an arc), so the roots name the machines and their PUs (and the
rack): the host knows its topology. After a preemptive commit no capacity is 0 and the
roots are the machines, or the rack, alone: the descent finds the rest. The two paths' graphs are compared after every repeat.
One warm-up repeat is dropped. Writes one JSON (medians and the raw lists).

    python tools/remove_measure.py --repeats 5 --out profiles/remove_resources_config3.json
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

REMOVE_RE = (r"remove: (\d+) nodes, (\d+) evictions, (\d+) records, (\d+) levels, mark ([\d.]+) ms, evict ([\d.]+) ms, "
             r"caps ([\d.]+) ms, emit \+ apply ([\d.]+) ms")
TASK, PU, SINK, MACHINE, INTERMEDIATE = 1, 2, 3, 4, 5


def build_stream(ntype, arcs, roots, bind_task, bind_pu, preemptive=False):
    """The records of the removal from a host's copy of the graph (arcs: ARC_DT, ntype by
    id − 1, the bindings as parallel arrays) → (stream DELTA_DT, removed ids, evicted tasks).
    The rule of ks_remove_resources with KS_REMOVE_RESOURCE_CAPS (pinned: slots − running)
    for a layered topology (PU → machine → type-0 rack → type-0 root), vectorised."""
    n = ntype.shape[0]
    src, dst = arcs["src"].astype(np.int64) - 1, arcs["dst"].astype(np.int64) - 1
    cap = arcs["cap"].astype(np.int64)
    res = np.isin(ntype, (PU, MACHINE, INTERMEDIATE))
    gone = np.zeros(n, bool)
    gone[np.asarray(roots, np.int64) - 1] = True
    while True:                                            # traverseAndRemoveTopology, level by level
        nxt = dst[gone[src] & res[dst] & ~gone[dst]]
        if nxt.size == 0:
            break
        gone[nxt] = True
    removed = np.nonzero(gone)[0] + 1
    evicted = bind_task[gone[bind_pu.astype(np.int64) - 1]]
    keep = ~(gone[src] | gone[dst])
    ts, td = ntype[src], ntype[dst]
    slots = np.zeros(n, np.int64)
    running = np.zeros(n, np.int64)
    pu_sink = keep & (td == SINK) & (ts == PU)
    slots[src[pu_sink]] = cap[pu_sink]
    run_arc = keep & (arcs["type"] == 1)
    running += np.bincount(dst[run_arc], minlength=n)
    running[ntype != PU] = 0
    for head in (PU, MACHINE, 0):                          # sums up the layers: machines, racks, the root
        up = keep & (ts != TASK) & (td == head) & (td != SINK)
        if head == 0:
            up &= slots[dst] > 0
        slots += np.bincount(src[up], weights=slots[dst[up]], minlength=n).astype(np.int64)
        running += np.bincount(src[up], weights=running[dst[up]], minlength=n).astype(np.int64)
    resarc = keep & (ts != TASK) & (td != SINK) & (np.isin(td, (PU, MACHINE, INTERMEDIATE)) | ((td == 0) & (slots[dst] > 0)))
    new = slots[dst] if preemptive else slots[dst] - running[dst]
    ch = np.nonzero(resarc & (new != cap))[0]
    stream = np.zeros(removed.shape[0] + ch.shape[0], native.DELTA_DT)
    stream["kind"][:removed.shape[0]] = native.KS_REMOVE_NODE
    stream["id"][:removed.shape[0]] = removed
    x = stream[removed.shape[0]:]
    x["kind"], x["type"], x["src"], x["dst"] = native.KS_UPDATE_ARC, arcs["type"][ch], arcs["src"][ch], arcs["dst"][ch]
    x["cap"], x["cost"], x["old_cost"] = new[ch], arcs["cost"][ch], arcs["cost"][ch]
    x["low"] = np.where(new[ch] > 0, arcs["low"][ch], 0)
    return stream, removed, evicted


def roots_of(cell, which, preemptive):
    """(i) 100 machines spread over the racks, (ii) rack 0. Pinned: with their machines and
    PUs (above); preemptive: the machines or the rack alone, the walk finds the rest."""
    M, R = cell.M, cell.R
    if which == "machines":
        k = np.arange(100, dtype=np.int64) * (M // 100)
        return (cell.MACH0 + k if preemptive else np.concatenate([cell.MACH0 + k, cell.PU0 + k])).astype(np.uint64)
    k = np.arange(0, M, R, dtype=np.int64)                  # machine k sits in rack k mod R
    return np.asarray([cell.RACK0] if preemptive else np.concatenate([[cell.RACK0], cell.MACH0 + k, cell.PU0 + k]),
                      np.uint64)


def committed(ctx, cell, preemptive):
    """The steady state between two rounds: solved, committed, and solved again (the
    residual CSR valid, with an edited graph's slack)."""
    with Stderr():
        ctx.load_graph(cell.graph())
        ctx.solve()
        deltas, _ = ctx.commit_preemptive(preemption=150) if preemptive else ctx.commit_schedule()
        ctx.solve()
    return deltas


def rows(ctx):
    _, a = ctx.graph()
    return np.sort(a, order=["src", "dst"])


def one_repeat(shape, which, preemptive):
    out = {}
    cell = churn.Cell(*shape)
    roots = roots_of(cell, which, preemptive)
    flags = native.KS_REMOVE_RESOURCE_CAPS | (native.KS_REMOVE_PREEMPTIVE if preemptive else 0)
    with native.Context(0, log_cycles=1) as ctx, native.Context(0, log_cycles=1) as twin:
        deltas = committed(ctx, cell, preemptive)
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
        stream, removed_h, evicted_h = build_stream(ntype, arcs, roots, deltas["task"], deltas["pu"], preemptive)
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
        rm = np.zeros(removed_h.shape[0] + 8, np.uint64)
        ev = np.zeros(evicted_h.shape[0] + 8, native.SCHED_DELTA_DT)
        nr, ne, st = C.c_size_t(), C.c_size_t(), native.KsRemoveStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_remove_resources(ctx._h, flags, roots.ctypes.data, roots.shape[0],
                                            rm.ctypes.data, rm.shape[0], C.byref(nr), ev.ctypes.data, ev.shape[0],
                                            C.byref(ne), C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(REMOVE_RE, log.text)
        out["remove_wall_ms"] = 1e3 * (t1 - t0)
        out["remove_levels"] = int(m.group(4))
        out["remove_mark_ms"], out["remove_evict_ms"], out["remove_caps_ms"], out["remove_apply_ms"] = (
            float(x) for x in m.groups()[4:])
        for k in ("nodes_removed", "pus_removed", "tasks_evicted", "arcs_removed", "cap_updates", "records"):
            out[k] = int(getattr(st, k))
        if rm[:nr.value].tolist() != removed_h.tolist() or ev["task"][:ne.value].tolist() != np.sort(evicted_h).tolist():
            raise SystemExit(f"{which}: the device's removed ids or evictions differ from the host's")
        if out["records"] != out["host_records"] or not (rows(ctx) == rows(twin)).all():
            raise SystemExit(f"{which}: the two paths' graphs differ")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(gen.CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shape = gen.CONFIGS[a.config]
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats}
    for mode in ("pinned", "preemptive"):
        res[mode] = {}
        for which in ("machines", "rack"):
            runs = [one_repeat(shape, which, mode == "preemptive") for _ in range(a.repeats + 1)][1:]   # the first: warm-up
            res[mode][which] = {"median": {k: statistics.median(r[k] for r in runs) for k in runs[0]}, "runs": runs}
            print(json.dumps({"config": a.config, "commit": mode, "removal": which, **res[mode][which]["median"]}),
                  flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
