"""ctypes binding of libksmcmf.so (include/ksmcmf.h).

The product path: every call goes to the in-tree HIP library. There is no CPU
fallback — if the library or a HIP device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _build

KS_OK, KS_E_INVALID, KS_E_INFEASIBLE, KS_E_DEVICE, KS_E_VERIFY, KS_E_RANGE = 0, -1, -2, -3, -4, -5
KS_ADD_NODE, KS_REMOVE_NODE, KS_ADD_ARC, KS_UPDATE_ARC, KS_SET_EXCESS = 0, 1, 2, 3, 4

EXPORTED_SYMBOLS = (
    "ks_abi_version", "ks_default_opts", "ks_create", "ks_destroy", "ks_last_error", "ks_load_graph",
    "ks_apply_deltas", "ks_solve", "ks_get_flows", "ks_get_task_mapping", "ks_get_task_pu_device", "ks_solve_many",
    "ks_coalesce_deltas", "ks_get_store_stats", "ks_set_bindings", "ks_scheduling_deltas",
    "ks_update_unsched_costs", "ks_topology_stats", "ks_get_graph", "ks_commit_schedule",
    "ks_commit_preemptive", "ks_remove_resources", "ks_complete_tasks", "ks_get_bindings",
    "ks_add_tasks", "ks_add_resources", "ks_update_tasks", "ks_update_nodes",
    "ks_batch_create", "ks_batch_create_rank", "ks_batch_unique_id", "ks_batch_destroy", "ks_batch_last_error",
    "ks_batch_load", "ks_batch_solve", "ks_batch_gather",
    "ks_batch_slots", "ks_batch_owner", "ks_batch_block_len", "ks_batch_unpack",
    "ks_batch_node_offsets", "ks_batch_translate_deltas", "ks_batch_reserve", "ks_batch_apply_deltas",
    "ks_batch_get_graph", "ks_batch_set_bindings", "ks_batch_commit_schedule", "ks_batch_commit_preemptive",
    "ks_batch_add_tasks", "ks_batch_complete_tasks", "ks_batch_update_tasks", "ks_batch_get_bindings",
    "ks_batch_update_unsched_costs",
    "ks_batch_remove_resources", "ks_batch_add_resources", "ks_batch_update_nodes",
)
ABI_VERSION = 5
KS_DELTA_PLACE, KS_DELTA_PREEMPT, KS_DELTA_MIGRATE, KS_DELTA_NOOP = 0, 1, 2, 3
KS_COST_SET, KS_COST_ADD = 0, 1
KS_COMMIT_RESOURCE_CAPS = 1
KS_REMOVE_RESOURCE_CAPS, KS_REMOVE_PREEMPTIVE = 1, 2
KS_COMPLETE_RESOURCE_CAPS, KS_COMPLETE_PREEMPTIVE = 1, 2
KS_UPDATE_KEEP_UNLISTED = 1
KS_NODES_KEEP_UNLISTED = 1
KS_CAP_KEEP = (1 << 64) - 1   # a listed arc of ks_update_nodes keeps the held arc's capacity

NODE_DT = np.dtype({"names": ["id", "excess", "type", "_pad"],
                    "formats": ["<u8", "<i8", "<i4", "<i4"], "offsets": [0, 8, 16, 20], "itemsize": 24})
ARC_DT = np.dtype({"names": ["src", "dst", "low", "cap", "cost", "type", "_pad"],
                   "formats": ["<u8", "<u8", "<u8", "<u8", "<i8", "<i4", "<i4"],
                   "offsets": [0, 8, 16, 24, 32, 40, 44], "itemsize": 48})
DELTA_DT = np.dtype({"names": ["kind", "type", "id", "src", "dst", "low", "cap", "cost", "old_cost", "excess"],
                     "formats": ["<i4", "<i4", "<u8", "<u8", "<u8", "<u8", "<u8", "<i8", "<i8", "<i8"],
                     "offsets": [0, 4, 8, 16, 24, 32, 40, 48, 56, 64], "itemsize": 72})
SCHED_DELTA_DT = np.dtype({"names": ["type", "_pad", "task", "pu"], "formats": ["<i4", "<i4", "<u8", "<u8"],
                           "offsets": [0, 4, 8, 16], "itemsize": 24})
BATCH_DELTA_DT = np.dtype({"names": ["type", "graph", "task", "pu"], "formats": ["<i4", "<i4", "<u8", "<u8"],
                           "offsets": [0, 4, 8, 16], "itemsize": 24})
FLOW_DT = np.dtype({"names": ["src", "dst", "flow"], "formats": ["<u8", "<u8", "<i8"],
                    "offsets": [0, 8, 16], "itemsize": 24})


class KsOpts(C.Structure):
    """ks_opts (include/ksmcmf.h): 0 in a tuning field selects the library default."""
    _fields_ = [("alpha", C.c_int32), ("verify", C.c_int32), ("auto_sink", C.c_int32),
                ("price_refine", C.c_int32), ("gu_interval", C.c_int32), ("warm_start", C.c_int32),
                ("walk_slack", C.c_int32), ("final_div", C.c_int32), ("pr_rounds", C.c_int32),
                ("phase_exit", C.c_int32), ("phase_frac", C.c_int32), ("tail_sweeps", C.c_int32),
                ("bf_margin", C.c_int32), ("two_hop", C.c_int32), ("log_cycles", C.c_int32),
                ("fault_inject", C.c_int32), ("walk_passes", C.c_int32), ("tail_nodes", C.c_int32),
                ("bf_bound", C.c_int32), ("fwd_nodes", C.c_int32), ("cell_nodes", C.c_int32),
                ("warm_shift", C.c_int32),
                ("warm_canon", C.c_int32),
                ("compact_pos", C.c_int32)]


class KsResult(C.Structure):
    _fields_ = [("total_cost", C.c_int64), ("flow_value", C.c_int64), ("status", C.c_int32),
                ("phases", C.c_int32), ("sweeps", C.c_uint64), ("arc_scans", C.c_uint64),
                ("node_visits", C.c_uint64), ("pushes", C.c_uint64), ("relabels", C.c_uint64),
                ("global_updates", C.c_uint64), ("gu_iterations", C.c_uint64), ("gu_arc_scans", C.c_uint64),
                ("ms_phase", C.c_double * 6), ("n_nodes", C.c_int64), ("n_arcs", C.c_int64),
                ("sweep_launches", C.c_uint64), ("ms_sweep_kernels", C.c_double),
                ("gu_launches", C.c_uint64), ("ms_gu_kernels", C.c_double), ("warm_started", C.c_int32),
                ("rebuilt", C.c_int32), ("recoveries", C.c_int32), ("solver", C.c_int32),
                ("fs_launches", C.c_uint64), ("ms_fs_kernels", C.c_double), ("fwd_updates", C.c_uint64),
                ("cells", C.c_int32), ("compact", C.c_int32), ("ms_cell_kernel", C.c_double),
                ("cell_ticks_max", C.c_uint64), ("cell_ticks_sum", C.c_uint64), ("fs_arc_scans", C.c_uint64),
                ("cell_fallbacks", C.c_uint64), ("cycles_cancelled", C.c_uint64), ("fb_resets", C.c_uint64),
                ("cycles_rejected", C.c_uint64), ("gu_leaf_scans", C.c_uint64), ("cells_run", C.c_int32),
                ("reserved4", C.c_int32), ("reserved3", C.c_uint64 * 1)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("ms_phase", "reserved3", "reserved4")}
        names = ("build", "saturate", "cycles", "price_refine", "verify", "total")
        d["ms"] = dict(zip(names, list(self.ms_phase)))
        return d


class KsStoreStats(C.Structure):
    _fields_ = [("live_arcs", C.c_int64), ("inserted", C.c_int64), ("updated", C.c_int64),
                ("killed", C.c_int64), ("superseded", C.c_int64), ("rebuilds", C.c_int64),
                ("residual_slots", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsCommitStats(C.Structure):
    """ks_commit_stats: what one ks_commit_schedule generated on device."""
    _fields_ = [("placed", C.c_int64), ("arcs_removed", C.c_int64), ("running_added", C.c_int64),
                ("running_converted", C.c_int64), ("unsched_updates", C.c_int64), ("cap_updates", C.c_int64),
                ("records", C.c_int64), ("reserved", C.c_int64 * 5)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsPreemptStats(C.Structure):
    """ks_preempt_stats: what one ks_commit_preemptive generated on device."""
    _fields_ = [("placed", C.c_int64), ("preempted", C.c_int64), ("migrated", C.c_int64),
                ("running_added", C.c_int64), ("running_converted", C.c_int64), ("running_removed", C.c_int64),
                ("unsched_cost_updates", C.c_int64), ("cap_updates", C.c_int64), ("records", C.c_int64),
                ("reserved", C.c_int64 * 3)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsRemoveStats(C.Structure):
    """ks_remove_stats: what one ks_remove_resources removed and generated on device."""
    _fields_ = [("roots", C.c_int64), ("nodes_removed", C.c_int64), ("pus_removed", C.c_int64),
                ("tasks_evicted", C.c_int64), ("arcs_removed", C.c_int64), ("cap_updates", C.c_int64),
                ("records", C.c_int64), ("reserved", C.c_int64 * 5)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsCompleteStats(C.Structure):
    """ks_complete_stats: what one ks_complete_tasks removed and generated on device."""
    _fields_ = [("tasks", C.c_int64), ("bound", C.c_int64), ("arcs_removed", C.c_int64),
                ("unsched_updates", C.c_int64), ("cap_updates", C.c_int64), ("records", C.c_int64),
                ("reserved", C.c_int64 * 6)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsAddStats(C.Structure):
    """ks_add_stats: what one ks_add_tasks generated on device."""
    _fields_ = [("tasks", C.c_int64), ("arcs_added", C.c_int64), ("unsched_updates", C.c_int64),
                ("unsched_added", C.c_int64), ("records", C.c_int64), ("reserved", C.c_int64 * 7)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsUpdateStats(C.Structure):
    """ks_update_stats: what one ks_update_tasks found and generated on device."""
    _fields_ = [("tasks", C.c_int64), ("arcs_added", C.c_int64), ("cost_updates", C.c_int64),
                ("arcs_unchanged", C.c_int64), ("running_kept", C.c_int64), ("arcs_removed", C.c_int64),
                ("unsched_updates", C.c_int64), ("unsched_added", C.c_int64), ("records", C.c_int64),
                ("reserved", C.c_int64 * 3)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


TASK_ARC_DT = np.dtype({"names": ["dst", "cost"], "formats": ["<u8", "<i8"], "offsets": [0, 8], "itemsize": 16})


class KsNodeStats(C.Structure):
    """ks_node_stats: what one ks_update_nodes found and generated on device."""
    _fields_ = [("nodes", C.c_int64), ("arcs_added", C.c_int64), ("arcs_updated", C.c_int64),
                ("arcs_unchanged", C.c_int64), ("arcs_skipped", C.c_int64), ("arcs_zeroed", C.c_int64),
                ("arcs_removed", C.c_int64), ("records", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


NODE_ARC_DT = np.dtype({"names": ["dst", "cost", "cap"], "formats": ["<u8", "<i8", "<u8"], "offsets": [0, 8, 16],
                        "itemsize": 24})


class KsBatchNodeList(C.Structure):
    """ks_batch_node_list (32 B): one graph's part of ks_batch_update_nodes, in the graph's own ids."""
    _fields_ = [("nodes", C.c_void_p), ("k", C.c_size_t), ("arc_off", C.c_void_p), ("arcs", C.c_void_p)]


def pack_node_lists(ngraphs: int, lists):
    """One ks_batch_node_list per graph. lists[g]: None (graph g untouched) or (nodes, arc_off,
    dst, cost, cap) as Context.update_nodes takes them. → (the ctypes array, the numpy arrays it
    points into: per graph a dict with nodes, arc_off, arcs (NODE_ARC_DT), or None)."""
    if lists is None:
        lists = [None] * ngraphs
    if len(lists) != ngraphs:
        raise ValueError("one entry (or None) per loaded graph")
    out = (KsBatchNodeList * max(1, ngraphs))()
    keep = []
    for g in range(ngraphs):
        if lists[g] is None:
            keep.append(None)
            continue
        nodes, off, dst, cost, cap = lists[g]
        a = {"nodes": np.ascontiguousarray(nodes, np.uint64).reshape(-1),
             "arc_off": np.ascontiguousarray(off, np.uint64).reshape(-1)}
        if a["arc_off"].shape[0] != a["nodes"].shape[0] + 1:
            raise ValueError("arc_off has one entry more than nodes")
        n = np.asarray(dst).size
        if np.asarray(cost).size != n or np.asarray(cap).size != n:
            raise ValueError("dst, cost and cap have one entry per listed arc")
        a["arcs"] = np.zeros(max(n, 1), NODE_ARC_DT)
        a["arcs"]["dst"][:n] = np.asarray(dst, np.uint64).reshape(-1)
        a["arcs"]["cost"][:n] = np.asarray(cost, np.int64).reshape(-1)
        a["arcs"]["cap"][:n] = np.asarray(cap, np.uint64).reshape(-1)
        out[g].nodes = a["nodes"].ctypes.data
        out[g].k = a["nodes"].shape[0]
        out[g].arc_off = a["arc_off"].ctypes.data
        out[g].arcs = a["arcs"].ctypes.data
        keep.append(a)
    return out, keep


class KsGrowStats(C.Structure):
    """ks_grow_stats: what one ks_add_resources generated on device."""
    _fields_ = [("nodes", C.c_int64), ("pus", C.c_int64), ("slots", C.c_int64), ("sink_arcs", C.c_int64),
                ("arcs_added", C.c_int64), ("cap_updates", C.c_int64), ("arcs_skipped", C.c_int64),
                ("records", C.c_int64), ("reserved", C.c_int64 * 4)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KsBatchTaskList(C.Structure):
    """ks_batch_task_list (48 B): one graph's part of a batch task call, in the graph's own ids."""
    _fields_ = [("tasks", C.c_void_p), ("k", C.c_size_t), ("arc_off", C.c_void_p), ("arcs", C.c_void_p),
                ("unsched_ids", C.c_void_p), ("nu", C.c_size_t)]


def pack_task_lists(ngraphs: int, lists, unsched_ids=None, with_arcs: bool = True):
    """One ks_batch_task_list per graph. lists[g]: None (graph g untouched), or with_arcs
    (tasks, arc_off, dst, cost) as Context.add_tasks takes them, else the task ids alone.
    unsched_ids: None (the NULL rule) or one id array (or None) per graph. → (the ctypes
    array, the numpy arrays it points into: per graph a dict with tasks, arc_off, arcs
    (TASK_ARC_DT), unsched_ids, or None)."""
    if lists is None:
        lists = [None] * ngraphs
    if len(lists) != ngraphs or (unsched_ids is not None and len(unsched_ids) != ngraphs):
        raise ValueError("one entry (or None) per loaded graph")
    out = (KsBatchTaskList * max(1, ngraphs))()
    keep = []
    for g in range(ngraphs):
        e = lists[g]
        agg = None if unsched_ids is None or unsched_ids[g] is None else \
            np.ascontiguousarray(unsched_ids[g], np.uint64).reshape(-1)
        if e is None and agg is None:
            keep.append(None)
            continue
        a = {"tasks": None, "arc_off": None, "arcs": None, "unsched_ids": agg}
        if e is not None:
            a["tasks"] = np.ascontiguousarray(e[0] if with_arcs else e, np.uint64).reshape(-1)
            if with_arcs:
                _, off, dst, cost = e
                a["arc_off"] = np.ascontiguousarray(off, np.uint64).reshape(-1)
                if a["arc_off"].shape[0] != a["tasks"].shape[0] + 1:
                    raise ValueError("arc_off has one entry more than tasks")
                dst, cost = np.asarray(dst, np.uint64).reshape(-1), np.asarray(cost, np.int64).reshape(-1)
                a["arcs"] = np.zeros(max(dst.size, 1), TASK_ARC_DT)
                a["arcs"]["dst"][:dst.size] = dst
                a["arcs"]["cost"][:cost.size] = cost
            out[g].tasks = a["tasks"].ctypes.data
            out[g].k = a["tasks"].shape[0]
            if with_arcs:
                out[g].arc_off = a["arc_off"].ctypes.data
                out[g].arcs = a["arcs"].ctypes.data
        if agg is not None:
            if agg.shape[0] == 0:   # an empty list names no aggregator: not NULL, which is the NULL rule
                a["unsched_ids"] = np.zeros(1, np.uint64)
            out[g].unsched_ids = a["unsched_ids"].ctypes.data
            out[g].nu = agg.shape[0]
        keep.append(a)
    return out, keep


RES_NODE_DT = np.dtype({"names": ["id", "type", "slots", "sink_cost"], "formats": ["<u8", "<i4", "<u8", "<i8"],
                        "offsets": [0, 8, 16, 24], "itemsize": 32})
RES_ARC_DT = np.dtype({"names": ["parent", "child", "cost", "kind"], "formats": ["<u8", "<u8", "<i8", "<i4"],
                       "offsets": [0, 8, 16, 24], "itemsize": 32})
KS_RES_TREE, KS_RES_EXTRA, KS_RES_MAX_DEPTH = 0, 1, 32


class KsBatchResList(C.Structure):
    """ks_batch_res_list (48 B): one graph's part of a batch resource call, in the graph's own ids."""
    _fields_ = [("roots", C.c_void_p), ("k", C.c_size_t), ("nodes", C.c_void_p), ("n", C.c_size_t),
                ("arcs", C.c_void_p), ("m", C.c_size_t)]


def res_rows(x, dt):
    """RES_NODE_DT / RES_ARC_DT rows from an array of that dtype or from tuples in field order."""
    if isinstance(x, np.ndarray) and x.dtype == dt:
        return np.ascontiguousarray(x).reshape(-1)
    out = np.zeros(len(x), dt)
    for name, col in zip(dt.names, zip(*x)):
        out[name] = np.asarray(col, dtype=dt[name])
    return out


class KsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ksmcmf error {code}: {msg}")
        self.code = code


_LIB = None


def lib_path() -> str:
    """The in-tree library; KS_LIB_VARIANT=<tag> selects libksmcmf_<tag>.so built
    by _build.build_variant (compile-time tuning experiments)."""
    tag = os.environ.get("KS_LIB_VARIANT")
    return _build.variant_path(tag) if tag else _build.LIB


_VARIANTS: dict = {}


def load(build_if_missing: bool = True, variant: str | None = None):
    """Load the in-tree library (building it with hipcc if absent and allowed).
    variant: an in-tree build of it, ksched_amd/libksmcmf_<variant>.so (tests use
    the fake-communicator build "fakecomm", _build.build_fake_comm)."""
    global _LIB
    if variant is not None:
        if variant not in _VARIANTS:
            path = _build.variant_path(variant)
            if not os.path.exists(path):
                raise RuntimeError(f"{path} missing: run __graft_entry__.build()")
            _VARIANTS[variant] = _bind(path)
        return _VARIANTS[variant]
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError(f"{path} missing: run __graft_entry__.build()")
        _build.build()
    _LIB = _bind(path)
    return _LIB


def _bind(path: str):
    if os.environ.get("KS_PRELOAD_TORCH", "1") != "0":
        # One HIP runtime per process: torch ships its own libamdhip64 (SONAME
        # libamdhip64.so.7) and links it by file name, so if the library loaded
        # /opt/rocm's copy first, a later torch.cuda init would bring up a second
        # HIP/HSA runtime and fail ("No HIP GPUs are available"). Importing torch
        # first makes libksmcmf bind to the runtime already loaded (same SONAME),
        # so the RCCL gather and the solver share device pointers and streams.
        import torch  # noqa: F401
    L = C.CDLL(path)
    P, V = C.POINTER, C.c_void_p
    L.ks_abi_version.restype = C.c_int
    L.ks_default_opts.argtypes = [P(KsOpts)]
    L.ks_create.argtypes = [C.c_int, P(KsOpts)]
    L.ks_create.restype = V
    L.ks_destroy.argtypes = [V]
    L.ks_last_error.argtypes = [V]
    L.ks_last_error.restype = C.c_char_p
    L.ks_load_graph.argtypes = [V, V, C.c_size_t, V, C.c_size_t]
    L.ks_apply_deltas.argtypes = [V, V, C.c_size_t]
    L.ks_solve.argtypes = [V, P(KsResult)]
    L.ks_get_flows.argtypes = [V, V, C.c_size_t, P(C.c_size_t)]
    L.ks_get_task_mapping.argtypes = [V, V, V, C.c_size_t, P(C.c_size_t)]
    L.ks_get_task_pu_device.argtypes = [V, V, C.c_size_t, P(C.c_size_t)]
    L.ks_solve_many.argtypes = [P(V), C.c_size_t, C.c_int, P(KsResult)]
    L.ks_coalesce_deltas.argtypes = [V, C.c_size_t, V, C.c_size_t, P(C.c_size_t)]
    L.ks_get_store_stats.argtypes = [V, P(KsStoreStats)]
    L.ks_get_graph.argtypes = [V, V, C.c_size_t, P(C.c_size_t), V, C.c_size_t, P(C.c_size_t)]
    L.ks_batch_create.argtypes = [P(C.c_int), C.c_int, P(KsOpts)]
    L.ks_batch_create.restype = V
    L.ks_batch_create_rank.argtypes = [C.c_int, C.c_int, C.c_int, V, P(KsOpts)]
    L.ks_batch_create_rank.restype = V
    L.ks_batch_unique_id.argtypes = [V]
    L.ks_batch_destroy.argtypes = [V]
    L.ks_batch_last_error.argtypes = [V]
    L.ks_batch_last_error.restype = C.c_char_p
    L.ks_batch_load.argtypes = [V, C.c_size_t, P(V), P(C.c_size_t), P(V), P(C.c_size_t)]
    L.ks_batch_solve.argtypes = [V, P(KsResult)]
    L.ks_batch_gather.argtypes = [V, C.c_size_t, V, V, V]
    L.ks_batch_slots.argtypes = [C.c_size_t, C.c_int]
    L.ks_batch_slots.restype = C.c_size_t
    L.ks_batch_owner.argtypes = [C.c_size_t, C.c_int, P(C.c_int), P(C.c_size_t)]
    L.ks_batch_block_len.argtypes = [C.c_size_t, C.c_int, C.c_size_t]
    L.ks_batch_block_len.restype = C.c_size_t
    L.ks_batch_unpack.argtypes = [V, C.c_size_t, C.c_int, C.c_size_t, V, V, V]
    L.ks_batch_node_offsets.argtypes = [V, C.c_size_t, C.c_size_t, V]
    L.ks_batch_translate_deltas.argtypes = [C.c_int64, C.c_int64, V, C.c_size_t, V]
    L.ks_batch_reserve.argtypes = [V, C.c_size_t]
    L.ks_batch_apply_deltas.argtypes = [V, C.c_size_t, P(V), P(C.c_size_t)]
    L.ks_batch_get_graph.argtypes = [V, C.c_size_t, V, C.c_size_t, P(C.c_size_t), V, C.c_size_t, P(C.c_size_t)]
    L.ks_batch_set_bindings.argtypes = [V, C.c_size_t, V, V, C.c_size_t]
    L.ks_batch_commit_schedule.argtypes = [V, C.c_int32, C.c_int64, V, C.c_size_t, P(C.c_size_t), P(KsCommitStats)]
    L.ks_batch_commit_preemptive.argtypes = [V, C.c_int32, C.c_int64, C.c_int64, V, C.c_size_t, P(C.c_size_t),
                                             P(KsPreemptStats)]
    L.ks_batch_add_tasks.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchTaskList), C.c_int64, P(KsAddStats)]
    L.ks_batch_complete_tasks.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchTaskList), P(V), P(KsCompleteStats)]
    L.ks_batch_update_tasks.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchTaskList), C.c_int64, P(KsUpdateStats)]
    L.ks_batch_get_bindings.argtypes = [V, C.c_size_t, V, V, C.c_size_t]
    L.ks_batch_update_unsched_costs.argtypes = [V, C.c_size_t, P(KsBatchTaskList), C.c_int32, C.c_int64, C.c_int64,
                                                P(C.c_size_t)]
    L.ks_batch_remove_resources.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchResList), V, C.c_size_t, P(C.c_size_t),
                                            V, V, C.c_size_t, P(C.c_size_t), P(KsRemoveStats)]
    L.ks_batch_add_resources.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchResList), P(KsGrowStats)]
    L.ks_batch_update_nodes.argtypes = [V, C.c_int32, C.c_size_t, P(KsBatchNodeList), P(KsNodeStats)]
    L.ks_set_bindings.argtypes = [V, V, V, C.c_size_t]
    L.ks_scheduling_deltas.argtypes = [V, C.c_int, V, C.c_size_t, P(C.c_size_t)]
    L.ks_update_unsched_costs.argtypes = [V, V, C.c_size_t, C.c_int32, C.c_int64, C.c_int64, P(C.c_size_t)]
    L.ks_topology_stats.argtypes = [V, C.c_uint64, V, V, C.c_size_t, V, V, C.c_size_t, P(C.c_size_t)]
    L.ks_commit_schedule.argtypes = [V, C.c_int32, C.c_int64, V, C.c_size_t, V, C.c_size_t, P(C.c_size_t),
                                     P(KsCommitStats)]
    L.ks_commit_preemptive.argtypes = [V, C.c_int32, C.c_int64, C.c_int64, V, C.c_size_t, V, C.c_size_t,
                                       P(C.c_size_t), P(KsPreemptStats)]
    L.ks_remove_resources.argtypes = [V, C.c_int32, V, C.c_size_t, V, C.c_size_t, P(C.c_size_t), V, C.c_size_t,
                                      P(C.c_size_t), P(KsRemoveStats)]
    L.ks_complete_tasks.argtypes = [V, C.c_int32, V, C.c_size_t, V, C.c_size_t, V, P(KsCompleteStats)]
    L.ks_add_tasks.argtypes = [V, C.c_int32, V, C.c_size_t, V, V, V, C.c_size_t, C.c_int64, P(KsAddStats)]
    L.ks_add_resources.argtypes = [V, C.c_int32, V, C.c_size_t, V, C.c_size_t, P(KsGrowStats)]
    L.ks_update_tasks.argtypes = [V, C.c_int32, V, C.c_size_t, V, V, V, C.c_size_t, C.c_int64, P(KsUpdateStats)]
    L.ks_update_nodes.argtypes = [V, C.c_int32, V, C.c_size_t, V, V, P(KsNodeStats)]
    L.ks_get_bindings.argtypes = [V, V, V, C.c_size_t]
    return L


def default_opts(**kw) -> KsOpts:
    o = KsOpts()
    load().ks_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@dataclass
class SolveResult:
    cost: int
    flow: int
    raw: dict


class Context:
    """One solver context on one HIP device (ks_create … ks_destroy)."""

    def __init__(self, device: int = 0, **opts):
        self._L = load()
        self.opts = default_opts(**opts)
        h = self._L.ks_create(device, C.byref(self.opts))
        if not h:
            raise KsError(KS_E_DEVICE, f"ks_create failed: no usable HIP device {device}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.ks_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != KS_OK:
            raise KsError(rc, self._L.ks_last_error(self._h).decode(errors="replace"))

    # -- graph upload -------------------------------------------------------
    def load_arrays(self, nodes: np.ndarray, arcs: np.ndarray):
        nodes = np.ascontiguousarray(nodes, NODE_DT)
        arcs = np.ascontiguousarray(arcs, ARC_DT)
        self._check(self._L.ks_load_graph(self._h, nodes.ctypes.data, nodes.shape[0],
                                          arcs.ctypes.data, arcs.shape[0]))

    def load_graph(self, g):
        """Upload a ksched_amd.gen.Graph (1-based ids, all nodes alive)."""
        nodes = np.zeros(g.n, NODE_DT)
        nodes["id"] = np.arange(1, g.n + 1, dtype=np.uint64)
        nodes["excess"] = g.supply
        nodes["type"] = g.ntype
        arcs = np.zeros(g.m, ARC_DT)
        arcs["src"], arcs["dst"] = g.src, g.dst
        arcs["low"], arcs["cap"], arcs["cost"] = g.low, g.cap, g.cost
        arcs["type"] = g.arc_types()
        self.load_arrays(nodes, arcs)

    def apply_deltas(self, deltas: np.ndarray):
        deltas = np.ascontiguousarray(deltas, DELTA_DT)
        self._check(self._L.ks_apply_deltas(self._h, deltas.ctypes.data, deltas.shape[0]))

    # -- solve & results ----------------------------------------------------
    def solve(self) -> SolveResult:
        r = KsResult()
        rc = self._L.ks_solve(self._h, C.byref(r))
        self._check(rc)
        return SolveResult(r.total_cost, r.flow_value, r.as_dict())

    def flows(self) -> np.ndarray:
        cnt = C.c_size_t()
        self._check(self._L.ks_get_flows(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, FLOW_DT)
        self._check(self._L.ks_get_flows(self._h, out.ctypes.data, cnt.value, C.byref(cnt)))
        return out

    def task_mapping_arrays(self) -> tuple[np.ndarray, np.ndarray]:
        """ks_get_task_mapping as the C-ABI returns it: parallel (task id, PU id) arrays."""
        cnt = C.c_size_t()
        self._check(self._L.ks_get_task_mapping(self._h, None, None, 0, C.byref(cnt)))
        t = np.zeros(cnt.value, np.uint64)
        p = np.zeros(cnt.value, np.uint64)
        self._check(self._L.ks_get_task_mapping(self._h, t.ctypes.data, p.ctypes.data, cnt.value, C.byref(cnt)))
        return t[:cnt.value], p[:cnt.value]

    def task_mapping(self) -> dict[int, int]:
        t, p = self.task_mapping_arrays()
        return dict(zip(t.tolist(), p.tolist()))

    def store_stats(self) -> dict:
        st = KsStoreStats()
        self._check(self._L.ks_get_store_stats(self._h, C.byref(st)))
        return st.as_dict()

    def graph(self):
        """The device-resident graph: (nodes NODE_DT, arcs ARC_DT)."""
        n, m = C.c_size_t(), C.c_size_t()
        self._check(self._L.ks_get_graph(self._h, None, 0, C.byref(n), None, 0, C.byref(m)))
        nodes = np.zeros(n.value, NODE_DT)
        arcs = np.zeros(m.value, ARC_DT)
        self._check(self._L.ks_get_graph(self._h, nodes.ctypes.data, n.value, C.byref(n), arcs.ctypes.data, m.value,
                                         C.byref(m)))
        return nodes, arcs

    # -- scheduler-side sweeps on device (ks_sched.hip) ----------------------
    def set_bindings(self, bindings: dict[int, int]):
        t = np.fromiter(bindings.keys(), np.uint64, len(bindings))
        p = np.fromiter(bindings.values(), np.uint64, len(bindings))
        self._check(self._L.ks_set_bindings(self._h, t.ctypes.data, p.ctypes.data, t.shape[0]))

    def scheduling_deltas(self, commit: bool = True) -> np.ndarray:
        """PREEMPT / PLACE / MIGRATE records (SCHED_DELTA_DT) of the last solve."""
        cnt = C.c_size_t()
        self._check(self._L.ks_scheduling_deltas(self._h, 0, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, SCHED_DELTA_DT)
        self._check(self._L.ks_scheduling_deltas(self._h, int(commit), out.ctypes.data, cnt.value, C.byref(cnt)))
        return out[:cnt.value]

    def update_unsched_costs(self, cost: int, mode: int = KS_COST_SET, continuation: int = 0,
                             unsched_ids=None) -> int:
        ch = C.c_size_t()
        ids = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64)
        self._check(self._L.ks_update_unsched_costs(self._h, None if ids is None else ids.ctypes.data,
                                                    0 if ids is None else ids.shape[0], mode, cost, continuation,
                                                    C.byref(ch)))
        return ch.value

    def topology_stats(self, max_tasks_per_pu: int, pu_running: dict[int, int] | None = None):
        """(slots_below, running_below) per node id − 1."""
        cnt = C.c_size_t()
        self._check(self._L.ks_topology_stats(self._h, max_tasks_per_pu, None, None, 0, None, None, 0,
                                              C.byref(cnt)))
        sl = np.zeros(cnt.value, np.uint64)
        rn = np.zeros(cnt.value, np.uint64)
        ids = vals = None
        k = 0
        if pu_running is not None:
            ids = np.fromiter(pu_running.keys(), np.uint64, len(pu_running))
            vals = np.fromiter(pu_running.values(), np.uint64, len(pu_running))
            k = ids.shape[0]
        self._check(self._L.ks_topology_stats(self._h, max_tasks_per_pu, None if ids is None else ids.ctypes.data,
                                              None if vals is None else vals.ctypes.data, k, sl.ctypes.data,
                                              rn.ctypes.data, cnt.value, C.byref(cnt)))
        return sl, rn

    def commit_schedule(self, continuation: int = 0, resource_caps: bool = True, unsched_ids=None):
        """ks_commit_schedule: pin every task the last solve placed, on device (the
        running arcs, the unscheduled aggregators' capacities and, with
        resource_caps, the resource arcs'). → (deltas SCHED_DELTA_DT, stats dict).
        Invalidates the solution: fetch the mapping first."""
        ids = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64)
        pid = None if ids is None else ids.ctypes.data
        k = 0 if ids is None else ids.shape[0]
        flags = KS_COMMIT_RESOURCE_CAPS if resource_caps else 0
        cnt = C.c_size_t()
        self._check(self._L.ks_commit_schedule(self._h, flags, continuation, pid, k, None, 0, C.byref(cnt), None))
        out = np.zeros(max(cnt.value, 1), SCHED_DELTA_DT)
        st = KsCommitStats()
        self._check(self._L.ks_commit_schedule(self._h, flags, continuation, pid, k, out.ctypes.data, cnt.value,
                                               C.byref(cnt), C.byref(st)))
        return out[:cnt.value], st.as_dict()

    def commit_preemptive(self, continuation: int = 0, preemption: int = 0, resource_caps: bool = True,
                          unsched_ids=None):
        """ks_commit_preemptive: commit every PLACE, PREEMPT and MIGRATE of the last solve
        on device (running arcs with low 0, the preemption cost on the arcs into the
        unscheduled aggregators and, with resource_caps, the resource arcs' capacities).
        → (deltas SCHED_DELTA_DT, stats dict). Invalidates the solution: fetch the
        mapping first."""
        ids = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64)
        pid = None if ids is None else ids.ctypes.data
        k = 0 if ids is None else ids.shape[0]
        flags = KS_COMMIT_RESOURCE_CAPS if resource_caps else 0
        cnt = C.c_size_t()
        self._check(self._L.ks_commit_preemptive(self._h, flags, continuation, preemption, pid, k, None, 0,
                                                 C.byref(cnt), None))
        out = np.zeros(max(cnt.value, 1), SCHED_DELTA_DT)
        st = KsPreemptStats()
        self._check(self._L.ks_commit_preemptive(self._h, flags, continuation, preemption, pid, k, out.ctypes.data,
                                                 cnt.value, C.byref(cnt), C.byref(st)))
        return out[:cnt.value], st.as_dict()

    def remove_resources(self, roots, resource_caps: bool = True, preemptive: bool = False):
        """ks_remove_resources: the subtrees of the root ids (machines, racks, PUs, or an
        unscheduled aggregator, which goes alone) leave the device-resident graph; every
        task bound in them is evicted and unbound and, with resource_caps, the surviving
        resource arcs get their capacities (preemptive: the rule of commit_preemptive).
        → (removed ids ascending uint64, evicted SCHED_DELTA_DT PREEMPTs in task order,
        stats dict). Needs no solve; invalidates the solution."""
        ids = np.ascontiguousarray(roots, np.uint64).reshape(-1)
        flags = (KS_REMOVE_RESOURCE_CAPS if resource_caps else 0) | (KS_REMOVE_PREEMPTIVE if preemptive else 0)
        nr, ne = C.c_size_t(), C.c_size_t()
        self._check(self._L.ks_remove_resources(self._h, flags, ids.ctypes.data, ids.shape[0], None, 0, C.byref(nr),
                                                None, 0, C.byref(ne), None))
        removed = np.zeros(max(nr.value, 1), np.uint64)
        evicted = np.zeros(max(ne.value, 1), SCHED_DELTA_DT)
        st = KsRemoveStats()
        self._check(self._L.ks_remove_resources(self._h, flags, ids.ctypes.data, ids.shape[0], removed.ctypes.data,
                                                nr.value, C.byref(nr), evicted.ctypes.data, ne.value, C.byref(ne),
                                                C.byref(st)))
        return removed[:nr.value], evicted[:ne.value], st.as_dict()

    def complete_tasks(self, tasks, resource_caps: bool = True, preemptive: bool = False, unsched_ids=None):
        """ks_complete_tasks: the finished (failed, killed) task ids leave the device-resident
        graph; each unscheduled aggregator loses one unit on its arc into the sink per
        completed task that still had an arc into it and, with resource_caps, the resource
        arcs get their capacities (preemptive: the rule of commit_preemptive, under which a
        completion changes none: such callers pass resource_caps=False).
        → (left: the PU each input id was bound to, 0 = unbound, uint64 aligned with tasks;
        stats dict). Needs no solve; invalidates the solution."""
        ids = np.ascontiguousarray(tasks, np.uint64).reshape(-1)
        agg = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64).reshape(-1)
        nu = 0 if agg is None else agg.shape[0]
        if agg is not None and nu == 0:
            agg = np.zeros(1, np.uint64)   # an empty list names no aggregator: not NULL, which is the auto rule
        flags = (KS_COMPLETE_RESOURCE_CAPS if resource_caps else 0) | (KS_COMPLETE_PREEMPTIVE if preemptive else 0)
        left = np.zeros(max(ids.shape[0], 1), np.uint64)
        st = KsCompleteStats()
        self._check(self._L.ks_complete_tasks(self._h, flags, ids.ctypes.data, ids.shape[0],
                                              None if agg is None else agg.ctypes.data,
                                              nu, left.ctypes.data, C.byref(st)))
        return left[:ids.shape[0]], st.as_dict()

    def add_tasks(self, tasks, arc_off, dst, cost, unsched_ids=None, unsched_sink_cost: int = 0) -> dict:
        """ks_add_tasks: the arriving task ids enter the device-resident graph as task nodes with
        supply 1; task i gets the arcs (dst[j], cost[j]) for arc_off[i] <= j < arc_off[i + 1]
        (low 0, cap 1, type 0), and each unscheduled aggregator gains one unit on its arc into
        the sink per arriving task with an arc into it (the arc is re-created with
        unsched_sink_cost when the store no longer holds it). unsched_ids=None: every type-0
        node with an arc into the sink; a task without an arc into one of those is then
        refused. → stats dict. Needs no solve; invalidates the solution when a task arrives."""
        ids = np.ascontiguousarray(tasks, np.uint64).reshape(-1)
        off = np.ascontiguousarray(arc_off, np.uint64).reshape(-1)
        if off.shape[0] != ids.shape[0] + 1:
            raise ValueError("arc_off has one entry more than tasks")
        arcs = np.zeros(max(np.asarray(dst).size, 1), TASK_ARC_DT)
        arcs["dst"][:np.asarray(dst).size] = np.asarray(dst, np.uint64).reshape(-1)
        arcs["cost"][:np.asarray(cost).size] = np.asarray(cost, np.int64).reshape(-1)
        agg = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64).reshape(-1)
        nu = 0 if agg is None else agg.shape[0]
        if agg is not None and nu == 0:
            agg = np.zeros(1, np.uint64)   # an empty list names no aggregator: not NULL, which is the auto rule
        st = KsAddStats()
        self._check(self._L.ks_add_tasks(self._h, 0, ids.ctypes.data, ids.shape[0], off.ctypes.data, arcs.ctypes.data,
                                         None if agg is None else agg.ctypes.data, nu, int(unsched_sink_cost),
                                         C.byref(st)))
        return st.as_dict()

    def add_resources(self, nodes, arcs) -> dict:
        """ks_add_resources: new resource nodes (RES_NODE_DT rows, or (id, type, slots, sink_cost)
        tuples) join the device-resident graph with supply 0; each PU gets its arc into the sink.
        arcs (RES_ARC_DT rows, or (parent, child, cost, kind) tuples): the KS_RES_TREE edges of the
        new subtree and of the chain from each attach point up to the root, and KS_RES_EXTRA arcs
        into nodes of the call. An edge whose head has S new slots beneath it is created with
        capacity S or, where the store still holds it, has its capacity raised by S. -> stats
        dict. Needs no solve; invalidates the solution when a record is applied."""
        nd, ar = res_rows(nodes, RES_NODE_DT), res_rows(arcs, RES_ARC_DT)
        st = KsGrowStats()
        self._check(self._L.ks_add_resources(self._h, 0, nd.ctypes.data if nd.shape[0] else None, nd.shape[0],
                                             ar.ctypes.data if ar.shape[0] else None, ar.shape[0], C.byref(st)))
        return st.as_dict()

    def update_tasks(self, tasks, arc_off, dst, cost, unsched_ids=None, unsched_sink_cost: int = 0,
                     keep_unlisted: bool = False) -> dict:
        """ks_update_tasks: the live task ids get the arcs their lists name. Task i's list is
        (dst[j], cost[j]) for arc_off[i] <= j < arc_off[i + 1]: an arc the store does not hold is
        added (low 0, cap 1, type 0), a held one whose cost differs is re-costed, a held running
        arc keeps its cost; a held arc the list does not name is deleted unless it is a running
        arc or an arc into an unscheduled aggregator (keep_unlisted: nothing is deleted, and no
        residual CSR is needed). An aggregator gains one unit on its arc into the sink per task
        whose listed arc into it the store did not hold (the arc is re-created with
        unsched_sink_cost when the store no longer holds it). unsched_ids=None: every type-0
        node with an arc into the sink; an unbound task that would end without an arc into one
        of those is then refused. → stats dict. Needs no solve; invalidates the solution when a
        record is applied."""
        ids = np.ascontiguousarray(tasks, np.uint64).reshape(-1)
        off = np.ascontiguousarray(arc_off, np.uint64).reshape(-1)
        if off.shape[0] != ids.shape[0] + 1:
            raise ValueError("arc_off has one entry more than tasks")
        arcs = np.zeros(max(np.asarray(dst).size, 1), TASK_ARC_DT)
        arcs["dst"][:np.asarray(dst).size] = np.asarray(dst, np.uint64).reshape(-1)
        arcs["cost"][:np.asarray(cost).size] = np.asarray(cost, np.int64).reshape(-1)
        agg = None if unsched_ids is None else np.ascontiguousarray(unsched_ids, np.uint64).reshape(-1)
        nu = 0 if agg is None else agg.shape[0]
        if agg is not None and nu == 0:
            agg = np.zeros(1, np.uint64)   # an empty list names no aggregator: not NULL, which is the auto rule
        st = KsUpdateStats()
        self._check(self._L.ks_update_tasks(self._h, KS_UPDATE_KEEP_UNLISTED if keep_unlisted else 0, ids.ctypes.data,
                                            ids.shape[0], off.ctypes.data, arcs.ctypes.data,
                                            None if agg is None else agg.ctypes.data, nu, int(unsched_sink_cost),
                                            C.byref(st)))
        return st.as_dict()

    def update_nodes(self, nodes, arc_off, dst, cost, cap, keep_unlisted: bool = False) -> dict:
        """ks_update_nodes: the live class, machine, intermediate and PU ids get the out-arcs
        their lists name. Tail i's list is (dst[j], cost[j], cap[j]) for arc_off[i] <= j <
        arc_off[i + 1]: an arc the store does not hold is added (low 0, type 0) unless its cap is
        0, a held one whose cost or capacity differs is updated with its lower bound and type
        kept, a held one listed with cap 0 is deleted; cap KS_CAP_KEEP keeps the held capacity. A
        type-0 tail's held arcs that its list does not name are deleted, except an arc into a
        sink; every other tail keeps them (keep_unlisted: nothing is deleted, and no residual
        CSR is needed). → stats dict. Needs no solve; invalidates the solution when a record is
        applied."""
        ids = np.ascontiguousarray(nodes, np.uint64).reshape(-1)
        off = np.ascontiguousarray(arc_off, np.uint64).reshape(-1)
        if off.shape[0] != ids.shape[0] + 1:
            raise ValueError("arc_off has one entry more than nodes")
        n = np.asarray(dst).size
        if np.asarray(cost).size != n or np.asarray(cap).size != n:
            raise ValueError("dst, cost and cap have one entry per listed arc")
        arcs = np.zeros(max(n, 1), NODE_ARC_DT)
        arcs["dst"][:n] = np.asarray(dst, np.uint64).reshape(-1)
        arcs["cost"][:n] = np.asarray(cost, np.int64).reshape(-1)
        arcs["cap"][:n] = np.asarray(cap, np.uint64).reshape(-1)
        st = KsNodeStats()
        self._check(self._L.ks_update_nodes(self._h, KS_NODES_KEEP_UNLISTED if keep_unlisted else 0, ids.ctypes.data,
                                            ids.shape[0], off.ctypes.data, arcs.ctypes.data, C.byref(st)))
        return st.as_dict()

    def bindings(self, tasks) -> np.ndarray:
        """ks_get_bindings: the PU each task id is bound to on the device, 0 = unbound."""
        ids = np.ascontiguousarray(tasks, np.uint64).reshape(-1)
        pu = np.zeros(max(ids.shape[0], 1), np.uint64)
        self._check(self._L.ks_get_bindings(self._h, ids.ctypes.data, pu.ctypes.data, ids.shape[0]))
        return pu[:ids.shape[0]]

    def task_pu_device(self, dev_ptr: int, cap: int) -> int:
        cnt = C.c_size_t()
        self._check(self._L.ks_get_task_pu_device(self._h, C.c_void_p(dev_ptr), cap, C.byref(cnt)))
        return cnt.value


def graph_arrays(g):
    """gen.Graph → (NODE_DT, ARC_DT) arrays with 1-based ids."""
    nodes = np.zeros(g.n, NODE_DT)
    nodes["id"] = np.arange(1, g.n + 1, dtype=np.uint64)
    nodes["excess"] = g.supply
    nodes["type"] = g.ntype
    arcs = np.zeros(g.m, ARC_DT)
    arcs["src"], arcs["dst"] = g.src, g.dst
    arcs["low"], arcs["cap"], arcs["cost"] = g.low, g.cap, g.cost
    arcs["type"] = g.arc_types()
    return nodes, arcs


class Batch:
    """Config 5 through the C-ABI (ks_batch_*): independent graphs, graph g on
    global rank g mod world, each device solving the union of its graphs; the
    per-graph rows gathered to rank 0 over RCCL inside libksmcmf.

    Batch(devices=[0, 1, ...]) drives several devices from one process;
    Batch(device=d, world=W, rank=r, uid=bytes) is one rank of a
    process-per-GPU job (uid from Batch.unique_id() on rank 0)."""

    def __init__(self, devices=None, device: int = 0, world: int = 1, rank: int = 0, uid: bytes | None = None,
                 variant: str | None = None, **opts):
        self._L = load(variant=variant)   # variant: an in-tree test build (tests: "fakecomm")
        self.opts = default_opts(**opts)
        if uid is None:
            devs = list(devices if devices is not None else [device])
            arr = (C.c_int * len(devs))(*devs)
            h = self._L.ks_batch_create(arr, len(devs), C.byref(self.opts))
            self.local = len(devs)
        else:
            buf = C.create_string_buffer(bytes(uid), 128)
            h = self._L.ks_batch_create_rank(device, world, rank, buf, C.byref(self.opts))
            self.local = 1
        if not h:
            raise KsError(KS_E_DEVICE, "ks_batch_create failed (device or RCCL unavailable)")
        self._h = h
        self.ngraphs = 0

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load().ks_batch_unique_id(buf)
        if rc != KS_OK:
            raise KsError(rc, "ks_batch_unique_id failed")
        return buf.raw

    def _check(self, rc):
        if rc != KS_OK:
            raise KsError(rc, self._L.ks_batch_last_error(self._h).decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._L.ks_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, graphs):
        self.load_arrays([graph_arrays(g) for g in graphs])

    def load_arrays(self, arrs):
        """ks_batch_load of prebuilt (nodes NODE_DT, arcs ARC_DT) pairs, one per graph."""
        k = len(arrs)
        self._keep = arrs
        npt = (C.c_void_p * max(1, k))(*[a[0].ctypes.data for a in arrs])
        apt = (C.c_void_p * max(1, k))(*[a[1].ctypes.data for a in arrs])
        ns = (C.c_size_t * max(1, k))(*[a[0].shape[0] for a in arrs])
        ms = (C.c_size_t * max(1, k))(*[a[1].shape[0] for a in arrs])
        self._check(self._L.ks_batch_load(self._h, k, npt, ns, apt, ms))
        self.ngraphs = k

    # -- rounds: deltas, the graph as it stands, bindings, commits ------------
    def reserve(self, spare_ids: int):
        """ks_batch_reserve: node ids every graph may grow by; takes effect at the next load."""
        self._check(self._L.ks_batch_reserve(self._h, spare_ids))

    def apply_deltas(self, streams):
        """ks_batch_apply_deltas: one DELTA_DT array (graph-local ids) or None per graph."""
        if len(streams) != self.ngraphs:
            raise ValueError("one stream (or None) per loaded graph")
        arrs = [None if d is None else np.ascontiguousarray(d, DELTA_DT) for d in streams]
        k = max(1, len(arrs))
        ptr = (C.c_void_p * k)(*[None if a is None or a.shape[0] == 0 else a.ctypes.data for a in arrs])
        cnt = (C.c_size_t * k)(*[0 if a is None else a.shape[0] for a in arrs])
        self._check(self._L.ks_batch_apply_deltas(self._h, len(arrs), ptr, cnt))

    def get_graph(self, g: int):
        """ks_batch_get_graph: graph g as it stands, graph-local ids → (nodes NODE_DT, arcs ARC_DT)."""
        n, m = C.c_size_t(), C.c_size_t()
        self._check(self._L.ks_batch_get_graph(self._h, g, None, 0, C.byref(n), None, 0, C.byref(m)))
        nodes = np.zeros(n.value, NODE_DT)
        arcs = np.zeros(m.value, ARC_DT)
        self._check(self._L.ks_batch_get_graph(self._h, g, nodes.ctypes.data, n.value, C.byref(n), arcs.ctypes.data,
                                               m.value, C.byref(m)))
        return nodes, arcs

    def set_bindings(self, g: int, bindings: dict[int, int]):
        t = np.fromiter(bindings.keys(), np.uint64, len(bindings))
        p = np.fromiter(bindings.values(), np.uint64, len(bindings))
        self._check(self._L.ks_batch_set_bindings(self._h, g, t.ctypes.data, p.ctypes.data, t.shape[0]))

    def commit_schedule(self, continuation: int = 0, resource_caps: bool = True):
        """ks_batch_commit_schedule → (deltas BATCH_DELTA_DT grouped by graph, stats summed
        over the local devices). Invalidates the solution: gather first."""
        flags = KS_COMMIT_RESOURCE_CAPS if resource_caps else 0
        cnt = C.c_size_t()
        self._check(self._L.ks_batch_commit_schedule(self._h, flags, continuation, None, 0, C.byref(cnt), None))
        out = np.zeros(max(cnt.value, 1), BATCH_DELTA_DT)
        st = KsCommitStats()
        self._check(self._L.ks_batch_commit_schedule(self._h, flags, continuation, out.ctypes.data, cnt.value,
                                                     C.byref(cnt), C.byref(st)))
        return out[:cnt.value], st.as_dict()

    def commit_preemptive(self, continuation: int = 0, preemption: int = 0, resource_caps: bool = True):
        """ks_batch_commit_preemptive → (deltas BATCH_DELTA_DT grouped by graph, stats)."""
        flags = KS_COMMIT_RESOURCE_CAPS if resource_caps else 0
        cnt = C.c_size_t()
        self._check(self._L.ks_batch_commit_preemptive(self._h, flags, continuation, preemption, None, 0,
                                                       C.byref(cnt), None))
        out = np.zeros(max(cnt.value, 1), BATCH_DELTA_DT)
        st = KsPreemptStats()
        self._check(self._L.ks_batch_commit_preemptive(self._h, flags, continuation, preemption, out.ctypes.data,
                                                       cnt.value, C.byref(cnt), C.byref(st)))
        return out[:cnt.value], st.as_dict()

    # -- rounds, the task side: one entry per graph, None = untouched, graph-local ids --------
    def add_tasks(self, lists, unsched_ids=None, unsched_sink_cost: int = 0) -> dict:
        """ks_batch_add_tasks: lists[g] = None or (tasks, arc_off, dst, cost) as Context.add_tasks
        takes them, in graph g's own ids; unsched_ids: None (the NULL rule) or one id array per
        graph (every listed graph then passes one). → stats summed over the local devices."""
        ls, keep = pack_task_lists(self.ngraphs, lists, unsched_ids, True)
        st = KsAddStats()
        self._check(self._L.ks_batch_add_tasks(self._h, 0, self.ngraphs, ls, int(unsched_sink_cost), C.byref(st)))
        del keep
        return st.as_dict()

    def complete_tasks(self, tasks, resource_caps: bool = True, preemptive: bool = False, unsched_ids=None):
        """ks_batch_complete_tasks: tasks[g] = None or the finished ids of graph g. → (left: per
        graph None or the PU each id was bound to, graph-local, 0 = unbound; stats)."""
        ls, keep = pack_task_lists(self.ngraphs, tasks, unsched_ids, False)
        flags = (KS_COMPLETE_RESOURCE_CAPS if resource_caps else 0) | (KS_COMPLETE_PREEMPTIVE if preemptive else 0)
        left = [None if a is None or a["tasks"] is None else np.zeros(max(a["tasks"].shape[0], 1), np.uint64)
                for a in keep]
        ptr = (C.c_void_p * max(1, self.ngraphs))(*[None if x is None else x.ctypes.data for x in left])
        st = KsCompleteStats()
        self._check(self._L.ks_batch_complete_tasks(self._h, flags, self.ngraphs, ls, ptr, C.byref(st)))
        return [None if x is None else x[:a["tasks"].shape[0]] for x, a in zip(left, keep)], st.as_dict()

    def update_tasks(self, lists, unsched_ids=None, unsched_sink_cost: int = 0, keep_unlisted: bool = False) -> dict:
        """ks_batch_update_tasks: lists[g] = None or (tasks, arc_off, dst, cost) as
        Context.update_tasks takes them, in graph g's own ids. → stats summed."""
        ls, keep = pack_task_lists(self.ngraphs, lists, unsched_ids, True)
        st = KsUpdateStats()
        self._check(self._L.ks_batch_update_tasks(self._h, KS_UPDATE_KEEP_UNLISTED if keep_unlisted else 0,
                                                  self.ngraphs, ls, int(unsched_sink_cost), C.byref(st)))
        del keep
        return st.as_dict()

    # -- rounds, the resource side: one entry per graph, None = untouched, graph-local ids ----
    def remove_resources(self, roots_per_graph, resource_caps: bool = True, preemptive: bool = False, flags=None):
        """ks_batch_remove_resources: roots_per_graph[g] = None or the root ids of graph g, as
        Context.remove_resources takes them. → (removed: per graph the removed ids ascending
        uint64, empty for an untouched graph; evicted BATCH_DELTA_DT PREEMPTs grouped by graph
        in task order; stats summed over the local devices). flags: the raw KS_REMOVE_* word
        instead of the two switches."""
        if len(roots_per_graph) != self.ngraphs:
            raise ValueError("one root list (or None) per loaded graph")
        if flags is None:
            flags = (KS_REMOVE_RESOURCE_CAPS if resource_caps else 0) | (KS_REMOVE_PREEMPTIVE if preemptive else 0)
        ls = (KsBatchResList * max(1, self.ngraphs))()
        keep = [None if r is None else np.ascontiguousarray(r, np.uint64).reshape(-1) for r in roots_per_graph]
        for g, r in enumerate(keep):
            if r is not None and r.shape[0]:
                ls[g].roots, ls[g].k = r.ctypes.data, r.shape[0]
        nr, ne = C.c_size_t(), C.c_size_t()
        self._check(self._L.ks_batch_remove_resources(self._h, flags, self.ngraphs, ls, None, 0, C.byref(nr), None,
                                                      None, 0, C.byref(ne), None))
        removed = np.zeros(max(nr.value, 1), np.uint64)
        evicted = np.zeros(max(ne.value, 1), BATCH_DELTA_DT)
        off = np.zeros(self.ngraphs + 1, np.uintp)
        st = KsRemoveStats()
        self._check(self._L.ks_batch_remove_resources(self._h, flags, self.ngraphs, ls, removed.ctypes.data, nr.value,
                                                      C.byref(nr), off.ctypes.data, evicted.ctypes.data, ne.value,
                                                      C.byref(ne), C.byref(st)))
        del keep
        per = [removed[int(off[g]):int(off[g + 1])].copy() for g in range(self.ngraphs)]
        return per, evicted[:ne.value], st.as_dict()

    def add_resources(self, per_graph) -> dict:
        """ks_batch_add_resources: per_graph[g] = None or (nodes, arcs) as Context.add_resources
        takes them, in graph g's own ids. → stats summed over the local devices."""
        if len(per_graph) != self.ngraphs:
            raise ValueError("one (nodes, arcs) pair (or None) per loaded graph")
        ls = (KsBatchResList * max(1, self.ngraphs))()
        keep = []
        for g, e in enumerate(per_graph):
            if e is None:
                continue
            nd, ar = res_rows(e[0], RES_NODE_DT), res_rows(e[1], RES_ARC_DT)
            keep.append((nd, ar))
            if nd.shape[0]:
                ls[g].nodes, ls[g].n = nd.ctypes.data, nd.shape[0]
            if ar.shape[0]:
                ls[g].arcs, ls[g].m = ar.ctypes.data, ar.shape[0]
        st = KsGrowStats()
        self._check(self._L.ks_batch_add_resources(self._h, 0, self.ngraphs, ls, C.byref(st)))
        del keep
        return st.as_dict()

    def update_nodes(self, lists, keep_unlisted: bool = False, flags=None) -> dict:
        """ks_batch_update_nodes: lists[g] = None or (nodes, arc_off, dst, cost, cap) as
        Context.update_nodes takes them, in graph g's own ids. → stats summed over the local
        devices. flags: the raw KS_NODES_* word instead of the switch."""
        ls, keep = pack_node_lists(self.ngraphs, lists)
        if flags is None:
            flags = KS_NODES_KEEP_UNLISTED if keep_unlisted else 0
        st = KsNodeStats()
        self._check(self._L.ks_batch_update_nodes(self._h, flags, self.ngraphs, ls, C.byref(st)))
        del keep
        return st.as_dict()

    def bindings(self, g: int, tasks) -> np.ndarray:
        """ks_batch_get_bindings: the PU each task of graph g is bound to, graph-local, 0 = unbound."""
        ids = np.ascontiguousarray(tasks, np.uint64).reshape(-1)
        pu = np.zeros(max(ids.shape[0], 1), np.uint64)
        self._check(self._L.ks_batch_get_bindings(self._h, g, ids.ctypes.data, pu.ctypes.data, ids.shape[0]))
        return pu[:ids.shape[0]]

    def update_unsched_costs(self, cost: int, mode: int = KS_COST_SET, continuation: int = 0, unsched_ids=None) -> int:
        """ks_batch_update_unsched_costs: unsched_ids None = every aggregator of every graph, else
        one id array (or None: untouched) per graph. → arcs whose cost changed."""
        ls = None
        if unsched_ids is not None:
            ls, keep = pack_task_lists(self.ngraphs, None, unsched_ids, False)
        ch = C.c_size_t()
        self._check(self._L.ks_batch_update_unsched_costs(self._h, self.ngraphs, ls, mode, int(cost), int(continuation),
                                                          C.byref(ch)))
        return ch.value

    def solve(self) -> list[SolveResult]:
        rs = (KsResult * self.local)()
        self._check(self._L.ks_batch_solve(self._h, rs))
        return [SolveResult(r.total_cost, r.flow_value, r.as_dict()) for r in rs]

    def gather(self, max_tasks: int, root: bool = True):
        """→ (pu [ngraphs, max_tasks] uint64, cost [ngraphs], flow [ngraphs]) on rank 0."""
        pu = np.zeros((self.ngraphs, max_tasks), np.uint64) if root else None
        cost = np.zeros(self.ngraphs, np.int64) if root else None
        flow = np.zeros(self.ngraphs, np.int64) if root else None
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self._L.ks_batch_gather(self._h, max_tasks, p(pu), p(cost), p(flow)))
        return pu, cost, flow


def batch_owner(g: int, world: int) -> tuple[int, int]:
    """ks_batch_owner: (global rank, slot on that rank) of graph g."""
    r, sl = C.c_int(), C.c_size_t()
    if load().ks_batch_owner(g, world, C.byref(r), C.byref(sl)) != KS_OK:
        raise KsError(KS_E_INVALID, "ks_batch_owner")
    return r.value, sl.value


def batch_node_offsets(maxids, spare: int = 0) -> np.ndarray:
    """ks_batch_node_offsets: the k + 1 node-id offsets of k graphs in a device's union."""
    mx = np.ascontiguousarray(maxids, np.uint64)
    off = np.zeros(mx.shape[0] + 1, np.int64)
    rc = load().ks_batch_node_offsets(mx.ctypes.data, mx.shape[0], spare, off.ctypes.data)
    if rc != KS_OK:
        raise KsError(rc, "ks_batch_node_offsets")
    return off


def batch_translate_deltas(lo: int, hi: int, deltas: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
    """ks_batch_translate_deltas: a graph-local stream into the id range (lo, hi] of a union
    (out may be the input array itself). KsError(KS_E_RANGE) when an id leaves the range."""
    d = np.ascontiguousarray(deltas, DELTA_DT)
    if out is None:
        out = np.zeros(d.shape[0], DELTA_DT)
    rc = load().ks_batch_translate_deltas(lo, hi, d.ctypes.data, d.shape[0], out.ctypes.data)
    if rc != KS_OK:
        raise KsError(rc, "ks_batch_translate_deltas: an id outside the graph's range")
    return out


def batch_block_len(ngraphs: int, world: int, max_tasks: int) -> int:
    return int(load().ks_batch_block_len(ngraphs, world, max_tasks))


def batch_unpack(gathered: np.ndarray, ngraphs: int, world: int, max_tasks: int):
    """ks_batch_unpack over the world blocks rank 0 received → (pu, cost, flow) in graph order."""
    gathered = np.ascontiguousarray(gathered, np.int64)
    pu = np.zeros((ngraphs, max_tasks), np.uint64)
    cost = np.zeros(ngraphs, np.int64)
    flow = np.zeros(ngraphs, np.int64)
    rc = load().ks_batch_unpack(gathered.ctypes.data, ngraphs, world, max_tasks, pu.ctypes.data, cost.ctypes.data,
                                flow.ctypes.data)
    if rc != KS_OK:
        raise KsError(rc, "ks_batch_unpack: a rank reported a failure")
    return pu, cost, flow


def solve_many(ctxs: list[Context], workers: int = 0) -> list[SolveResult]:
    """ks_solve_many: solve independent contexts concurrently (native worker
    threads, one stream per context). Raises KsError on the first failure."""
    L = load()
    k = len(ctxs)
    hs = (C.c_void_p * max(1, k))(*[c._h for c in ctxs])
    rs = (KsResult * max(1, k))()
    rc = L.ks_solve_many(hs, k, workers, rs)
    if rc != KS_OK:
        bad = next((c for c, r in zip(ctxs, rs) if r.status != KS_OK), None)
        if bad is None:   # rejected before any solve ran (e.g. a null context)
            raise KsError(rc, "ks_solve_many failed")
        bad._check(rc)
    return [SolveResult(r.total_cost, r.flow_value, r.as_dict()) for r in rs[:k]]


def coalesce_deltas(deltas: np.ndarray) -> np.ndarray:
    """ks_coalesce_deltas: the change optimisers of graph_change_manager.go:220-279
    (merge per arc, drop duplicates, purge before node removal). Host-only."""
    d = np.ascontiguousarray(deltas, DELTA_DT)
    out = np.zeros(d.shape[0], DELTA_DT)
    cnt = C.c_size_t()
    rc = load().ks_coalesce_deltas(d.ctypes.data, d.shape[0], out.ctypes.data, d.shape[0], C.byref(cnt))
    if rc != KS_OK:
        raise KsError(rc, "ks_coalesce_deltas: invalid node id in delta stream")
    return out[:cnt.value]
