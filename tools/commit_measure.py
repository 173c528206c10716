#!/usr/bin/env python3
"""ks_commit_schedule against the host path it replaces, on the config-3 cell after
its first solve. Per repeat, on freshly loaded contexts:

  (a) ks_commit_schedule: wall time of the one call, and its device share (the
      event-timed span the library reports with ks_opts.log_cycles);
  (b) the host path at its most favourable: the pin and capacity stream built
      outside the timer, ks_apply_deltas alone timed (wall, and the library's own
      "store kernels + wait" share);
  (c) churn.Cell.step's construction of that stream.

One warm-up repeat is dropped. Writes one JSON (medians and the raw lists).

    python tools/commit_measure.py --repeats 5 --out profiles/commit_schedule_config3.json

With --preemptive the same three timings for ks_commit_preemptive against
Cell(preemption=True).step, twice per repeat: after the first solve (placements only)
and after one 5 % churn round and a re-solve (the round that holds PREEMPT and
MIGRATE). The model and both contexts follow the device context's mapping.

    python tools/commit_measure.py --preemptive --repeats 5 --out profiles/commit_preemptive_config3.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ksched_amd import churn, gen, native  # noqa: E402


class Stderr:
    """The library's log_cycles lines (written to fd 2) of the enclosed calls."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def one_repeat(shape):
    out = {}
    # (a) the device path
    cell = churn.Cell(*shape)
    with native.Context(0, log_cycles=1) as ctx:
        with Stderr():
            ctx.load_graph(cell.graph())
            ctx.solve()
            mp = ctx.task_mapping_arrays()
        buf = np.zeros(shape[0], native.SCHED_DELTA_DT)
        cnt, st = C.c_size_t(), native.KsCommitStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_commit_schedule(ctx._h, native.KS_COMMIT_RESOURCE_CAPS, 0, None, 0, buf.ctypes.data,
                                           buf.shape[0], C.byref(cnt), C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(r"commit: (\d+) records, deltas ([\d.]+) ms, count passes ([\d.]+) ms, emit \+ apply ([\d.]+) ms, "
                      r"device span after the deltas ([\d.]+) ms", log.text)
        out["commit_wall_ms"] = 1e3 * (t1 - t0)
        out["commit_deltas_ms"], out["commit_count_ms"], out["commit_apply_ms"], out["commit_device_span_ms"] = (
            float(x) for x in m.groups()[1:])
        out["commit_records"] = int(st.records)
        out["placed"] = int(st.placed)
        out["store_rebuilds"] = int(ctx.store_stats()["rebuilds"])
    # (b), (c) the host path on the same graph
    cell = churn.Cell(*shape)
    with native.Context(0, log_cycles=1) as ctx:
        with Stderr():
            ctx.load_graph(cell.graph())
            ctx.solve()
            mp = ctx.task_mapping_arrays()
        t0 = time.perf_counter()
        stream = cell.step(mp, 0, 0, age_cost=0)
        t1 = time.perf_counter()
        stream = np.ascontiguousarray(stream, native.DELTA_DT)
        with Stderr() as log:
            t2 = time.perf_counter()
            ctx.apply_deltas(stream)
            t3 = time.perf_counter()
        m = re.search(r"apply: upload call ([\d.]+) ms \(([\d.]+) MB\), store kernels \+ wait ([\d.]+) ms", log.text)
        out["step_build_ms"] = 1e3 * (t1 - t0)
        out["apply_wall_ms"] = 1e3 * (t3 - t2)
        out["apply_upload_call_ms"], out["apply_upload_mb"], out["apply_kernels_wait_ms"] = (float(x) for x in m.groups())
        out["host_records"] = int(stream.shape[0])
    return out


COMMIT_RE = (r"commit: (\d+) records, deltas ([\d.]+) ms, count passes ([\d.]+) ms, emit \+ apply ([\d.]+) ms, "
             r"device span after the deltas ([\d.]+) ms")
APPLY_RE = r"apply: upload call ([\d.]+) ms \(([\d.]+) MB\), store kernels \+ wait ([\d.]+) ms"


def preemptive_repeat(shape, pcost):
    out = {}
    T = shape[0]
    cell = churn.Cell(*shape, preemption=True, preemption_cost=pcost)
    with native.Context(0, log_cycles=1) as a, native.Context(0, log_cycles=1) as b:
        with Stderr():
            for c in (a, b):
                c.load_graph(cell.graph())
        for stage in ("first", "churn"):
            with Stderr():
                a.solve()
                b.solve()
                mp = b.task_mapping_arrays()
            # (c) the stream's construction, (b) ks_apply_deltas alone on it
            t0 = time.perf_counter()
            stream = cell.step(mp, 0, 0, age_cost=0)
            t1 = time.perf_counter()
            stream = np.ascontiguousarray(stream, native.DELTA_DT)
            with Stderr() as log:
                t2 = time.perf_counter()
                a.apply_deltas(stream)
                t3 = time.perf_counter()
            m = re.search(APPLY_RE, log.text)
            out[f"{stage}_step_build_ms"] = 1e3 * (t1 - t0)
            out[f"{stage}_apply_wall_ms"] = 1e3 * (t3 - t2)
            out[f"{stage}_apply_kernels_wait_ms"] = float(m.group(3))
            out[f"{stage}_host_records"] = int(stream.shape[0])
            # (a) the one call
            buf = np.zeros(2 * T, native.SCHED_DELTA_DT)
            cnt, st = C.c_size_t(), native.KsPreemptStats()
            with Stderr() as log:
                t0 = time.perf_counter()
                rc = b._L.ks_commit_preemptive(b._h, native.KS_COMMIT_RESOURCE_CAPS, 0, pcost, None, 0, buf.ctypes.data,
                                               buf.shape[0], C.byref(cnt), C.byref(st))
                t1 = time.perf_counter()
            b._check(rc)
            m = re.search(COMMIT_RE, log.text)
            out[f"{stage}_commit_wall_ms"] = 1e3 * (t1 - t0)
            (out[f"{stage}_commit_deltas_ms"], out[f"{stage}_commit_count_ms"], out[f"{stage}_commit_apply_ms"],
             out[f"{stage}_commit_device_span_ms"]) = (float(x) for x in m.groups()[1:])
            for k in ("records", "placed", "preempted", "migrated"):
                out[f"{stage}_{k}"] = int(getattr(st, k))
            if out[f"{stage}_records"] != out[f"{stage}_host_records"]:
                raise SystemExit(f"{stage}: {out[f'{stage}_records']} device records, "
                                 f"{out[f'{stage}_host_records']} host records")
            if stage == "first":
                with Stderr():
                    stream = cell.step(None, T // 20, T // 20)
                    a.apply_deltas(stream)
                    b.apply_deltas(stream)
        out["store_rebuilds"] = int(b.store_stats()["rebuilds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(gen.CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--preemptive", action="store_true", help="measure ks_commit_preemptive")
    ap.add_argument("--preemption-cost", type=int, default=150)
    a = ap.parse_args()
    shape = gen.CONFIGS[a.config]
    one = (lambda: preemptive_repeat(shape, a.preemption_cost)) if a.preemptive else (lambda: one_repeat(shape))
    runs = [one() for _ in range(a.repeats + 1)][1:]   # the first is the warm-up
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats, "median": med, "runs": runs}
    if a.preemptive:
        res["preemptive"], res["preemption_cost"] = True, a.preemption_cost
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"config": a.config, **med}))


if __name__ == "__main__":
    main()
