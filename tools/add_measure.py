#!/usr/bin/env python3
"""ks_add_tasks against the host path it replaces, on the config-3 cell:
5,000 tasks of five arcs arrive in one call, each repeat on freshly loaded contexts. Two
states: "first", after the first solve and a preemptive commit (the commit's running arcs
overflowed the load's tight segments, so a rebuild of the residual CSR is pending and both
paths edit the tables only), and "steady", after one more solve (the CSR valid, with an edited
graph's slack: both paths insert in place where there is room).

  (a) ks_add_tasks: wall time of the one call and its split upload + checks + counts / node
      table + sizing / emit + apply (ks_opts.log_cycles);
  (b) the host path at its most favourable: the identical records built outside the timer,
      ks_apply_deltas alone timed (wall, and the library's "store kernels + wait" share);
  (c) the construction of that stream in numpy from the arrivals and the host's copy of the
      aggregators' arcs into the sink.

The arrivals are the churn model's own (ksched_amd/churn.py step 3: fresh ids, the five
preference arcs of the Quincy shape). The two paths' graphs are compared after every repeat.
One warm-up repeat is dropped. Writes one JSON (medians and the raw lists).

    python tools/add_measure.py --repeats 5 --out profiles/add_tasks_config3.json
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
from tools.remove_measure import rows  # noqa: E402

ADD_RE = (r"add: (\d+) tasks, (\d+) arcs, (\d+) records, upload \+ checks \+ counts ([\d.]+) ms, "
          r"node table \+ sizing ([\d.]+) ms, emit \+ apply ([\d.]+) ms")
STATES = ("first", "steady")


def build_stream(ids, dst, cost, arcs, aggs, sink, sink_cost=0):
    """The records of the arrivals in the order ks_add_tasks fixes: the ADD_NODE records, the
    task arcs, one record per gaining aggregator in ascending id (arcs: the host's copy, ARC_DT)."""
    k, per = dst.shape
    heads = dst.reshape(-1).astype(np.int64)
    gain = np.bincount(heads[np.isin(heads, aggs.astype(np.int64))], minlength=int(aggs.max()) + 1)
    up = np.nonzero(gain)[0]
    held = arcs[(arcs["dst"] == sink) & np.isin(arcs["src"].astype(np.int64), up)]
    held = held[np.argsort(held["src"])]
    stream = np.zeros(k + k * per + up.shape[0], native.DELTA_DT)
    n = stream[:k]
    n["kind"], n["type"], n["id"], n["excess"] = native.KS_ADD_NODE, 1, ids, 1
    a = stream[k:k + k * per]
    a["kind"], a["src"], a["dst"], a["cap"], a["cost"] = native.KS_ADD_ARC, np.repeat(ids, per), dst.reshape(-1), 1, \
        cost.reshape(-1)
    u = stream[k + k * per:]
    u["kind"], u["src"], u["dst"], u["cap"], u["cost"] = native.KS_ADD_ARC, up, sink, gain[up], sink_cost
    hs = held["src"].astype(np.int64)
    at = np.searchsorted(up, hs)                               # the arcs the store holds: low, cost and type kept
    u["kind"][at], u["type"][at], u["low"][at] = native.KS_UPDATE_ARC, held["type"], held["low"]
    u["cap"][at], u["cost"][at], u["old_cost"][at] = held["cap"] + gain[hs].astype(np.uint64), held["cost"], held["cost"]
    return stream


def one_repeat(shape, state, count):
    out = {}
    cell = churn.Cell(*shape, preemption=True, preemption_cost=150)
    aggs = cell.U0 + np.arange(cell.J, dtype=np.uint64)
    with native.Context(0, log_cycles=1) as ctx, native.Context(0, log_cycles=1) as twin:
        with Stderr():
            ctx.load_graph(cell.graph())
            ctx.solve()
            ctx.commit_preemptive(preemption=150, resource_caps=False)
            if state == "steady":
                ctx.solve()
            # the host path's context holds the same graph in the same state: "first", no residual
            # CSR (a load leaves none, as the pending rebuild does); "steady", one built with an
            # edited graph's slack (a no-op upsert before the solve marks the graph as edited)
            nodes, arcs = ctx.graph()
            twin.load_arrays(nodes, arcs)
            if state == "steady":
                noop = np.zeros(1, native.DELTA_DT)
                noop["kind"] = native.KS_ADD_ARC
                for f in ("src", "dst", "low", "cap", "cost", "type"):
                    noop[f] = arcs[f][0]
                twin.apply_deltas(noop)
                twin.solve()
            twin.graph()   # (a download: whatever the solve left queued on the stream has run before the timer starts)
        cell.step(None, 0, count, age_cost=0)                   # the arrivals (untimed: the scheduler has them)
        ids = np.asarray(cell.last_arrived_ids, np.uint64)
        sl = ids.astype(np.int64) - cell.TASK0
        dst, cost = cell.adst[sl].astype(np.uint64), cell.acost[sl].copy()
        # (c) the stream from the arrivals and the host's copy of the aggregators' arcs
        t0 = time.perf_counter()
        stream = build_stream(ids, dst, cost, arcs, aggs, cell.SINK)
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
        out["host_stream_bytes"] = int(stream.nbytes)
        # (a) the one call
        off = np.arange(ids.shape[0] + 1, dtype=np.uint64) * dst.shape[1]
        ta = np.zeros(dst.size, native.TASK_ARC_DT)
        ta["dst"], ta["cost"] = dst.reshape(-1), cost.reshape(-1)
        out["device_input_bytes"] = int(ids.nbytes + off.nbytes + ta.nbytes + aggs.nbytes)
        st = native.KsAddStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_add_tasks(ctx._h, 0, ids.ctypes.data, ids.shape[0], off.ctypes.data, ta.ctypes.data,
                                     aggs.ctypes.data, aggs.shape[0], 0, C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(ADD_RE, log.text)
        out["add_wall_ms"] = 1e3 * (t1 - t0)
        out["add_check_ms"], out["add_host_ms"], out["add_apply_ms"] = (float(x) for x in m.groups()[3:])
        for k in ("tasks", "arcs_added", "unsched_updates", "unsched_added", "records"):
            out[k] = int(getattr(st, k))
        if out["records"] != out["host_records"] or not (rows(ctx) == rows(twin)).all():
            raise SystemExit(f"{state}: the two paths' graphs differ")
        with Stderr():                                          # both re-solve to the same optimum
            ra, rb = ctx.solve(), twin.solve()
        if (ra.cost, ra.flow) != (rb.cost, rb.flow):
            raise SystemExit(f"{state}: the two paths' solves differ")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(gen.CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tasks", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shape = gen.CONFIGS[a.config]
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats, "arrivals": a.tasks}
    for state in STATES:
        runs = [one_repeat(shape, state, a.tasks) for _ in range(a.repeats + 1)][1:]   # the first: warm-up
        res[state] = {"median": {k: statistics.median(r[k] for r in runs) for k in runs[0]}, "runs": runs}
        print(json.dumps({"config": a.config, "state": state, **res[state]["median"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
