"""CPU: the batch task calls' C-ABI surface (no device): the ABI version, the size of
ks_batch_task_list, the bound symbols, KS_E_INVALID on a null handle, and the Python packing of the
per-graph lists (offsets, None entries, the dtype of the arcs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ksched_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ks_batch_add_tasks", "ks_batch_complete_tasks", "ks_batch_update_tasks", "ks_batch_get_bindings",
       "ks_batch_update_unsched_costs")


@pytest.fixture(scope="module")
def lib():
    return native.load(build_if_missing=False)


def test_abi_version_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "ksmcmf.h")).read()
    assert re.search(r"#define KSMCMF_ABI_VERSION (\d+)", header).group(1) == "5"
    assert lib.ks_abi_version() == native.ABI_VERSION == 5
    assert C.sizeof(native.KsBatchTaskList) == 48
    fields = re.search(r"typedef struct ks_batch_task_list \{(.*?)\} ks_batch_task_list;", header, re.S).group(1)
    assert [f for f, _ in native.KsBatchTaskList._fields_] == re.findall(r"(\w+);", fields)


def test_symbols_are_bound(lib):
    for sym in NEW:
        assert sym in native.EXPORTED_SYMBOLS
        assert getattr(lib, sym).argtypes is not None


def test_null_handle_is_invalid(lib):
    one = (native.KsBatchTaskList * 1)()
    ch = C.c_size_t(7)
    assert lib.ks_batch_add_tasks(None, 0, 1, one, 0, None) == native.KS_E_INVALID
    assert lib.ks_batch_complete_tasks(None, 0, 1, one, None, None) == native.KS_E_INVALID
    assert lib.ks_batch_update_tasks(None, 0, 1, one, 0, None) == native.KS_E_INVALID
    assert lib.ks_batch_get_bindings(None, 0, None, None, 0) == native.KS_E_INVALID
    assert lib.ks_batch_update_unsched_costs(None, 1, one, 0, 0, 0, C.byref(ch)) == native.KS_E_INVALID
    assert ch.value == 7                                   # nothing is written on a null handle


def u64(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), (n,)).tolist()


def test_packing_of_per_graph_lists():
    lists = [([11, 12], [0, 2, 3], [5, 6, 7], [-1, 2, 3]), None, ([9], [0, 0], [], [])]
    ls, keep = native.pack_task_lists(3, lists, [[4, 5], None, []], True)
    assert (ls[0].k, ls[1].k, ls[2].k) == (2, 0, 1)
    assert ls[1].tasks is None and ls[1].arc_off is None and ls[1].arcs is None and ls[1].unsched_ids is None
    assert keep[1] is None
    assert u64(ls[0].tasks, 2) == [11, 12] and u64(ls[0].arc_off, 3) == [0, 2, 3]
    arcs = keep[0]["arcs"]
    assert arcs.dtype == native.TASK_ARC_DT and arcs.dtype.itemsize == 16
    assert arcs["dst"].tolist() == [5, 6, 7] and arcs["cost"].tolist() == [-1, 2, 3]
    assert ls[0].arcs == arcs.ctypes.data
    assert (ls[0].nu, u64(ls[0].unsched_ids, 2)) == (2, [4, 5])
    # a task without arcs: offsets 0, 0 and a non-null arc pointer; an empty id list is not NULL
    assert u64(ls[2].arc_off, 2) == [0, 0] and ls[2].arcs and ls[2].nu == 0 and ls[2].unsched_ids
    # the NULL rule: no aggregator pointer anywhere
    ls, keep = native.pack_task_lists(3, lists, None, True)
    assert all(ls[g].unsched_ids is None and ls[g].nu == 0 for g in range(3))
    # ids alone (completions), and aggregators alone (costs)
    ls, keep = native.pack_task_lists(2, [[3, 3, 4], None], None, False)
    assert ls[0].k == 3 and u64(ls[0].tasks, 3) == [3, 3, 4] and ls[0].arc_off is None and ls[1].k == 0
    ls, keep = native.pack_task_lists(2, None, [None, [8]], False)
    assert ls[0].nu == 0 and ls[0].unsched_ids is None and (ls[1].k, ls[1].nu, u64(ls[1].unsched_ids, 1)) == (0, 1, [8])


def test_packing_refuses_a_wrong_shape():
    with pytest.raises(ValueError):
        native.pack_task_lists(2, [None], None, True)
    with pytest.raises(ValueError):
        native.pack_task_lists(1, [([1, 2], [0, 1], [5], [5])], None, True)
    with pytest.raises(ValueError):
        native.pack_task_lists(2, [None, None], [None], False)
