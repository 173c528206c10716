"""CPU suite: the host-only layout helpers of the batch rounds.

ks_batch_node_offsets places every graph of a device's union — its highest id plus the
reserved ids — and ks_batch_translate_deltas moves a graph-local delta stream into its
range. ks_batch_load and ks_batch_apply_deltas call exactly these, so a wrong offset or
an id that leaks into the next cell shows here without a device. The same edge cases run
under AddressSanitizer and UBSan in a stand-alone C++ program
(tests/sanitize/batch_layout_main.cpp)."""
import ctypes as C

import numpy as np
import pytest

from ksched_amd import native

K = native


def test_cells_run_in_the_reserved_word():
    lib = native.load()
    assert lib.ks_abi_version() == native.ABI_VERSION     # additions only: the version did not move
    # the struct did not grow: cells_run took half of the first reserved word after gu_leaf_scans
    assert native.KsResult.cells_run.offset == native.KsResult.gu_leaf_scans.offset + 8
    assert C.sizeof(native.KsResult) == native.KsResult.gu_leaf_scans.offset + 8 + 16
    assert "cells_run" in native.KsResult().as_dict()
    assert native.BATCH_DELTA_DT.itemsize == 24


@pytest.mark.parametrize("maxids", [[7], [5, 9, 1, 12_127], [3, 0, 4]])
def test_node_offsets_spare_0_is_the_running_sum(maxids):
    off = native.batch_node_offsets(maxids, 0)
    assert off.tolist() == [0] + np.cumsum(maxids).tolist()


@pytest.mark.parametrize("spare", [1, 16, 256])
def test_node_offsets_spare_adds_i_times_s(spare):
    maxids = [2432, 1217, 612, 2432, 368, 1217]
    base = native.batch_node_offsets(maxids, 0)
    off = native.batch_node_offsets(maxids, spare)
    assert off.tolist() == [int(b) + i * spare for i, b in enumerate(base)]
    assert native.batch_node_offsets([], spare).tolist() == [0]


def _stream():
    d = np.zeros(5, native.DELTA_DT)
    d["kind"] = [K.KS_ADD_NODE, K.KS_REMOVE_NODE, K.KS_SET_EXCESS, K.KS_ADD_ARC, K.KS_UPDATE_ARC]
    d["id"] = [10, 3, 1, 0, 0]                 # arc kinds do not use id: it stays 0
    d["src"] = [0, 0, 0, 10, 4]                # node kinds do not use src / dst
    d["dst"] = [0, 0, 0, 2, 10]
    d["cap"], d["cost"], d["excess"] = 1, 7, -5
    return d


def test_translate_moves_every_kinds_ids():
    d = _stream()
    out = native.batch_translate_deltas(100, 110, d)
    assert out["id"].tolist() == [110, 103, 101, 0, 0]
    assert out["src"].tolist() == [0, 0, 0, 110, 104]
    assert out["dst"].tolist() == [0, 0, 0, 102, 110]
    for f in ("kind", "type", "low", "cap", "cost", "old_cost", "excess"):
        assert out[f].tolist() == d[f].tolist(), f
    # lo = 0 is the identity
    assert native.batch_translate_deltas(0, 10, d).tobytes() == d.tobytes()


@pytest.mark.parametrize("field,rec", [("id", 0), ("id", 1), ("id", 2), ("src", 3), ("dst", 3), ("src", 4), ("dst", 4)])
@pytest.mark.parametrize("bad", ["zero", "past"])
def test_translate_refuses_ids_outside_the_range_and_writes_nothing(field, rec, bad):
    lo, hi = 100, 110
    d = _stream()
    d[field][rec] = 0 if bad == "zero" else hi - lo + 1
    out = np.full(d.shape[0], 0, native.DELTA_DT)
    out["cost"] = 12345                          # a sentinel: the call must not write
    before = out.tobytes()
    with pytest.raises(native.KsError) as e:
        native.batch_translate_deltas(lo, hi, d, out)
    assert e.value.code == native.KS_E_RANGE
    assert out.tobytes() == before
    # the largest id of the range itself is fine
    d[field][rec] = hi - lo
    native.batch_translate_deltas(lo, hi, d, out)


def test_translate_in_place():
    d = _stream()
    want = native.batch_translate_deltas(40, 50, d)
    same = native.batch_translate_deltas(40, 50, d, d)
    assert same is d and d.tobytes() == want.tobytes()
    # a refused in-place call leaves the stream as it was
    d2 = _stream()
    d2["dst"][3] = 11
    keep = d2.tobytes()
    with pytest.raises(native.KsError):
        native.batch_translate_deltas(40, 50, d2, d2)
    assert d2.tobytes() == keep


def test_translate_empty_and_bad_arguments():
    lib = native.load()
    assert lib.ks_batch_translate_deltas(5, 9, None, 0, None) == native.KS_OK
    d = _stream()
    assert lib.ks_batch_translate_deltas(9, 5, d.ctypes.data, d.shape[0], d.ctypes.data) == native.KS_E_INVALID
    assert lib.ks_batch_translate_deltas(0, 20, d.ctypes.data, d.shape[0], None) == native.KS_E_INVALID
    assert lib.ks_batch_node_offsets(None, 2, 0, None) == native.KS_E_INVALID
