#!/usr/bin/env python3
"""ks_update_tasks against the host path it replaces, on the config-3 cell:
5,000 waiting tasks are refreshed in one call with five listed arcs each (the aggregator arc and
one preference unchanged, two preferences re-costed, one new head; one held preference is
dropped), each repeat on freshly loaded contexts. Two states, as in tools/add_measure.py:
"first", after the first solve and a preemptive commit (a rebuild of the residual CSR is
pending), and "steady", after one more solve (the CSR valid); each with and without
KS_UPDATE_KEEP_UNLISTED (with it nothing is dropped and no CSR is needed).

  (a) ks_update_tasks: wall time of the one call and its split upload + checks + diff / sizing /
      emit + apply (ks_opts.log_cycles); in "first" without the flag the call also pays the
      pending rebuild, reported with it;
  (b) the host path at its most favourable: the identical records built outside the timer,
      ks_apply_deltas alone timed (wall, and the library's "store kernels + wait" share);
  (c) the construction of that stream in numpy from a ks_get_graph shadow of the tasks' arcs.

The two paths' graphs are compared after every repeat. One warm-up repeat is dropped. Writes one
JSON (medians and the raw lists).

    python tools/update_measure.py --repeats 5 --out profiles/update_tasks_config3.json
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

UPD_RE = (r"update: (\d+) tasks, (\d+) arcs, (\d+) records, upload \+ checks \+ diff ([\d.]+) ms, "
          r"sizing ([\d.]+) ms, emit \+ apply ([\d.]+) ms")
STATES = ("first", "steady")


def choose(cell, arcs, bound, count):
    """count tasks that hold exactly five type-0 arcs, the waiting ones first; → (ids, heads
    [k, 5] with the aggregator first, costs [k, 5])."""
    src = arcs["src"].astype(np.int64)
    mine = arcs[(src >= cell.TASK0) & (arcs["type"] == 0)]
    mine = mine[np.argsort(mine["src"], kind="stable")]
    ids, start, cnt = np.unique(mine["src"].astype(np.int64), return_index=True, return_counts=True)
    ok = cnt == 5
    ids, start = ids[ok], start[ok]
    order = np.argsort(np.isin(ids, bound), kind="stable")[:count]          # unbound first
    ids, start = ids[order], start[order]
    at = start[:, None] + np.arange(5)
    heads, costs = mine["dst"][at].astype(np.int64), mine["cost"][at].astype(np.int64)
    agg = (heads >= cell.U0) & (heads < cell.TASK0)
    col = np.argsort(~agg, axis=1, kind="stable")
    return ids, np.take_along_axis(heads, col, 1), np.take_along_axis(costs, col, 1)


def wishes(cell, ids, heads, costs):
    """Five listed arcs per task: the aggregator arc and one preference as they are, two
    preferences re-costed, one machine the task has no arc into; the fourth preference is left out."""
    new = cell.MACH0 + ids % cell.M
    for _ in range(8):
        clash = (heads == new[:, None]).any(1)
        new = np.where(clash, cell.MACH0 + (new - cell.MACH0 + 1) % cell.M, new)
    dst = np.stack([heads[:, 0], heads[:, 1], heads[:, 2], heads[:, 3], new], 1)
    cost = np.stack([costs[:, 0], costs[:, 1] + 7, costs[:, 2] + 7, costs[:, 3], np.full(ids.shape[0], 11)], 1)
    return dst.astype(np.uint64), cost.astype(np.int64)


def build_stream(ids, dst, cost, arcs, aggs, keep):
    """The records in the order ks_update_tasks fixes, from the host's shadow (arcs: ARC_DT in
    arc-slot order): the cost changes and deletions on held arcs by slot, then the new arcs in
    input order. (No aggregator gains a unit here: every listed aggregator arc is held.)"""
    key = lambda s, d: (s.astype(np.int64) << 32) | d.astype(np.int64)
    at = np.nonzero(np.isin(arcs["src"], ids))[0]                           # the listed tasks' held arcs, by slot
    held = arcs[at]
    hk = key(held["src"], held["dst"])
    lk = key(np.repeat(ids, dst.shape[1]), dst.reshape(-1))
    lc = cost.reshape(-1)
    order = np.argsort(lk)
    pos = np.searchsorted(lk[order], hk)
    pos[pos == lk.shape[0]] = 0
    listed = lk[order][pos] == hk
    want = lc[order][pos]
    plain = held["type"] == 0
    change = listed & plain & (want != held["cost"])
    drop = ~listed & plain & ~np.isin(held["dst"], aggs) & (not keep)
    sel = change | drop
    part1 = np.zeros(int(sel.sum()), native.DELTA_DT)
    h = held[sel]
    part1["kind"], part1["type"], part1["src"], part1["dst"] = native.KS_UPDATE_ARC, h["type"], h["src"], h["dst"]
    part1["old_cost"] = h["cost"]
    ch = change[sel]
    part1["low"], part1["cap"] = np.where(ch, h["low"], 0), np.where(ch, h["cap"], 0)
    part1["cost"] = np.where(ch, want[sel], h["cost"])
    absent = ~np.isin(lk, hk)
    part2 = np.zeros(int(absent.sum()), native.DELTA_DT)
    part2["kind"], part2["cap"] = native.KS_ADD_ARC, 1
    part2["src"], part2["dst"], part2["cost"] = lk[absent] >> 32, lk[absent] & 0xFFFFFFFF, lc[absent]
    return np.concatenate([part1, part2])


def one_repeat(shape, state, count, keep):
    out = {}
    cell = churn.Cell(*shape, preemption=True, preemption_cost=150)
    aggs = cell.U0 + np.arange(cell.J, dtype=np.uint64)
    with native.Context(0, log_cycles=1) as ctx, native.Context(0, log_cycles=1) as twin:
        with Stderr():
            ctx.load_graph(cell.graph())
            ctx.solve()
            deltas, _ = ctx.commit_preemptive(preemption=150, resource_caps=False)
            if state == "steady":
                ctx.solve()
            # the host path's context holds the same graph in the same state (tools/add_measure.py)
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
        ids, heads, costs = choose(cell, arcs, deltas["task"].astype(np.int64), count)
        dst, cost = wishes(cell, ids, heads, costs)
        out["waiting"] = int((~np.isin(ids, deltas["task"].astype(np.int64))).sum())   # the rest run (and keep their arcs)
        ids = ids.astype(np.uint64)
        # (c) the stream from the lists and the host's shadow of the tasks' arcs
        t0 = time.perf_counter()
        stream = build_stream(ids, dst, cost, arcs, aggs, keep)
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
        st = native.KsUpdateStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_update_tasks(ctx._h, native.KS_UPDATE_KEEP_UNLISTED if keep else 0, ids.ctypes.data,
                                        ids.shape[0], off.ctypes.data, ta.ctypes.data, aggs.ctypes.data, aggs.shape[0],
                                        0, C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(UPD_RE, log.text)
        out["update_wall_ms"] = 1e3 * (t1 - t0)
        out["update_check_ms"], out["update_sizing_ms"], out["update_apply_ms"] = (float(x) for x in m.groups()[3:])
        # (the wall time beyond the three: the pending rebuild of the residual CSR, "first" without the flag)
        out["update_before_ms"] = out["update_wall_ms"] - out["update_check_ms"] - out["update_sizing_ms"] - \
            out["update_apply_ms"]
        for k, _ in native.KsUpdateStats._fields_[:-1]:
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
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats, "refreshed": a.tasks}
    for keep in (False, True):
        for state in STATES:
            name = state + ("_keep_unlisted" if keep else "")
            runs = [one_repeat(shape, state, a.tasks, keep) for _ in range(a.repeats + 1)][1:]   # the first: warm-up
            res[name] = {"median": {k: statistics.median(r[k] for r in runs) for k in runs[0]}, "runs": runs}
            print(json.dumps({"config": a.config, "state": name, **res[name]["median"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
