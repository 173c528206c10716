#!/usr/bin/env python3
"""ks_add_resources against the host path it replaces, on the config-3 graph (DESIGN §8 item
12): after the first solve 500 machines of one PU each join under existing racks, with their
chains, in one call; each repeat runs on freshly loaded contexts.

  (a) ks_add_resources: wall time of the one call and its split upload + checks + sums / node
      table + sizing / emit + apply (ks_opts.log_cycles);
  (b) the host path at its most favourable: the identical records built outside the timer,
      ks_apply_deltas alone timed (wall, and the library's "store kernels + wait" share);
  (c) the construction of that stream in numpy from the new topology and the host's copy of
      the arcs (the capacities of the root's arcs into the racks, which only that copy has).

Machine i joins rack i mod R; the chain of a rack is the root's arc into it, listed once. The
two paths' graphs are compared after every repeat. One warm-up repeat is dropped. Writes one
JSON (medians and the raw lists).

    python tools/grow_measure.py --repeats 5 --out profiles/add_resources_config3.json
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

from ksched_amd import gen, native  # noqa: E402
from tools.commit_measure import APPLY_RE, Stderr  # noqa: E402
from tools.remove_measure import rows  # noqa: E402

GROW_RE = (r"grow: (\d+) nodes, (\d+) edges, (\d+) records, upload \+ checks \+ sums ([\d.]+) ms, "
           r"node table \+ sizing ([\d.]+) ms, emit \+ apply ([\d.]+) ms")
SINK, X, RACK0 = 1, 2, 3


def inputs(first_id, count, R, slots):
    """The call's two arrays: machine and PU interleaved, their two edges each, then the chains."""
    nd = np.zeros(2 * count, native.RES_NODE_DT)
    mach = first_id + 2 * np.arange(count, dtype=np.uint64)
    nd["id"][0::2], nd["type"][0::2] = mach, 4
    nd["id"][1::2], nd["type"][1::2], nd["slots"][1::2] = mach + 1, 2, slots
    rack = (RACK0 + np.arange(count) % R).astype(np.uint64)
    racks = np.unique(rack)
    ar = np.zeros(2 * count + racks.shape[0], native.RES_ARC_DT)
    ar["parent"][0:2 * count:2], ar["child"][0:2 * count:2] = rack, mach
    ar["parent"][1:2 * count:2], ar["child"][1:2 * count:2] = mach, mach + 1
    ar["parent"][2 * count:], ar["child"][2 * count:] = X, racks
    return nd, ar


def build_stream(nd, ar, arcs):
    """The records in the order ks_add_resources fixes (arcs: the host's copy, ARC_DT): every
    new head's arc is created with the slots beneath it, the root's arcs into the racks are held
    and rise by their racks' gains."""
    n = nd.shape[0]
    pus = nd[nd["type"] == 2]
    new = ar[np.isin(ar["child"], nd["id"])]
    chain = ar[~np.isin(ar["child"], nd["id"])]
    slots_of = dict(zip(pus["id"].tolist(), pus["slots"].tolist()))
    below = {int(e["child"]): slots_of[int(e["child"])] for e in new if int(e["child"]) in slots_of}
    for e in new:                                                # machine → PU listed after rack → machine
        if int(e["child"]) in slots_of:
            below[int(e["parent"])] = below.get(int(e["parent"]), 0) + slots_of[int(e["child"])]
    gain: dict = {}
    for e in new:
        if int(e["child"]) not in slots_of:
            gain[int(e["parent"])] = gain.get(int(e["parent"]), 0) + below[int(e["child"])]
    stream = np.zeros(n + pus.shape[0] + ar.shape[0], native.DELTA_DT)
    s = stream[:n]
    s["kind"], s["type"], s["id"] = native.KS_ADD_NODE, nd["type"], nd["id"]
    s = stream[n:n + pus.shape[0]]
    s["kind"], s["src"], s["dst"], s["cap"], s["cost"] = native.KS_ADD_ARC, pus["id"], SINK, pus["slots"], pus["sink_cost"]
    s = stream[n + pus.shape[0]:]
    s["kind"], s["src"], s["dst"], s["cost"] = native.KS_ADD_ARC, ar["parent"], ar["child"], ar["cost"]
    k = new.shape[0]
    s["cap"][:k] = [below[int(c)] for c in new["child"]]
    held = arcs[(arcs["src"] == X) & np.isin(arcs["dst"], chain["child"])]
    held = held[np.argsort(held["dst"])]
    assert (held["dst"] == chain["child"]).all()                 # (ascending racks on both sides, every arc held)
    c = s[k:]
    c["kind"], c["type"], c["low"], c["cost"], c["old_cost"] = native.KS_UPDATE_ARC, held["type"], held["low"], held["cost"], \
        held["cost"]
    c["cap"] = held["cap"] + np.asarray([gain[int(r)] for r in chain["child"]], np.uint64)
    return stream


def one_repeat(shape, count, slots):
    out = {}
    g = gen.quincy(*shape)
    R = shape[2]
    with native.Context(0, log_cycles=1) as ctx, native.Context(0, log_cycles=1) as twin:
        with Stderr():
            for c in (ctx, twin):
                c.load_graph(g)
                c.solve()
            nodes, arcs = ctx.graph()
            twin.graph()   # (a download: whatever the solve left queued on the stream has run before the timer starts)
        nd, ar = inputs(g.n + 1, count, R, slots)
        # (c) the stream from the new topology and the host's copy of the arcs
        t0 = time.perf_counter()
        stream = build_stream(nd, ar, arcs)
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
        out["device_input_bytes"] = int(nd.nbytes + ar.nbytes)
        st = native.KsGrowStats()
        with Stderr() as log:
            t0 = time.perf_counter()
            rc = ctx._L.ks_add_resources(ctx._h, 0, nd.ctypes.data, nd.shape[0], ar.ctypes.data, ar.shape[0], C.byref(st))
            t1 = time.perf_counter()
        ctx._check(rc)
        m = re.search(GROW_RE, log.text)
        out["grow_wall_ms"] = 1e3 * (t1 - t0)
        out["grow_check_ms"], out["grow_host_ms"], out["grow_apply_ms"] = (float(x) for x in m.groups()[3:])
        for k in ("nodes", "pus", "slots", "sink_arcs", "arcs_added", "cap_updates", "arcs_skipped", "records"):
            out[k] = int(getattr(st, k))
        if out["records"] != out["host_records"] or not (rows(ctx) == rows(twin)).all():
            raise SystemExit("the two paths' graphs differ")
        with Stderr():                                          # both re-solve to the same optimum
            ra, rb = ctx.solve(), twin.solve()
        if (ra.cost, ra.flow) != (rb.cost, rb.flow):
            raise SystemExit("the two paths' solves differ")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3", choices=sorted(gen.CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--machines", type=int, default=500)
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shape = gen.CONFIGS[a.config]
    runs = [one_repeat(shape, a.machines, a.slots) for _ in range(a.repeats + 1)][1:]   # the first: warm-up
    res = {"config": a.config, "shape": list(shape), "repeats": a.repeats, "machines": a.machines, "slots": a.slots,
           "median": {k: statistics.median(r[k] for r in runs) for k in runs[0]}, "runs": runs}
    print(json.dumps({"config": a.config, **res["median"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
