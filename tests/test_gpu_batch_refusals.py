"""GPU: the whole text of the refusals that every batch round call shares — the list checks, the
"outside the graph's ids" range refusal of the host and of the device's head translation, and the
one aggregator rule of a call. The suites of the calls themselves check a code and a few words of
a message; here every message is pinned as a literal, so a noun, a graph index or a span that a
shared helper gets wrong shows.

Two cells (cells 0 and 3 of the batch suites) on one device with 16 reserved ids each, cold: nothing
is solved. The offender is always in graph 1, whose span is 248 + 16 = 264, so a message that names
graph 0 or a union id (graph 0 spans 384 ids) is wrong. After every refusal both graphs are
byte-identical to the snapshot taken at the start."""
import ctypes as C

import numpy as np
import pytest

from commit_ref import MACHINE, PU
from grow_ref import TREE
from ksched_amd import churn, native
from test_gpu_batch_tasks import CELLS, snapshot

pytestmark = pytest.mark.gpu

RANGE, INVALID = native.KS_E_RANGE, native.KS_E_INVALID
SPAN = 264                       # graph 1: its 248 nodes at the load plus the 16 reserved ids
X, RACK, AGG, LIVE, NEW = 2, 3, 45, 49, 249   # graph 1: the class node, a rack, an aggregator, a live task, a free id
SUFFIX = " is outside the graph's ids 1..264 (its highest id at the load plus the reserved ids)"


@pytest.fixture(scope="module")
def batch():
    cells = [churn.Cell(*CELLS[0]), churn.Cell(*CELLS[3])]
    assert cells[1].graph().n + 16 == SPAN and cells[0].graph().n + 16 == 384
    assert (cells[1].X, cells[1].RACK0, cells[1].U0, cells[1].TASK0) == (X, RACK, AGG, LIVE)
    b = native.Batch(devices=[0])
    b.reserve(16)
    b.load([c.graph() for c in cells])
    yield b, snapshot(b, 2)
    b.close()


def refused(batch, call, code, text):
    b, before = batch
    with pytest.raises(native.KsError) as e:
        call()
    assert e.value.code == code, e.value
    assert str(e.value) == f"ksmcmf error {code}: {text}"
    assert snapshot(b, 2) == before


def task_list(tasks, off, heads):
    return (tasks, np.asarray(off, np.uint64), np.asarray(heads, np.uint64), np.full(len(heads), 5, np.int64))


def node_list(tails, off, heads):
    return (tails, np.asarray(off, np.uint64), np.asarray(heads, np.uint64), np.full(len(heads), 3, np.int64),
            np.full(len(heads), 2, np.uint64))


# ------------------------------------------------------------- the offsets of a list ---
def test_arc_off_must_start_at_zero(batch):
    b = batch[0]
    refused(batch, lambda: b.add_tasks([None, task_list([NEW, NEW + 1], [1, 1, 2], [AGG, AGG])]), INVALID,
            "graph 1: arc_off[0] must be 0")
    refused(batch, lambda: b.update_tasks([None, task_list([LIVE, LIVE + 1], [1, 1, 2], [AGG, AGG])]), INVALID,
            "graph 1: arc_off[0] must be 0")
    refused(batch, lambda: b.update_nodes([None, node_list([RACK, X], [1, 1, 2], [5, RACK])]), INVALID,
            "graph 1: arc_off[0] must be 0")


def test_arc_off_decreases(batch):
    b = batch[0]
    refused(batch, lambda: b.add_tasks([None, task_list([NEW, NEW + 1], [0, 2, 1], [AGG, AGG])]), INVALID,
            "graph 1: arc_off decreases at task 250")
    refused(batch, lambda: b.update_tasks([None, task_list([LIVE, LIVE + 1], [0, 2, 1], [AGG, AGG])]), INVALID,
            "graph 1: arc_off decreases at task 50")
    refused(batch, lambda: b.update_nodes([None, node_list([RACK, X], [0, 2, 1], [5, RACK])]), INVALID,
            "graph 1: arc_off decreases at node 2")


# ------------------------------------------- ids the host checks: 0 and span + 1 ---
@pytest.mark.parametrize("bad", [0, SPAN + 1])
def test_ids_outside_the_graph(batch, bad):
    b = batch[0]
    refused(batch, lambda: b.add_tasks([None, task_list([NEW, bad], [0, 1, 2], [AGG, AGG])]), RANGE,
            f"graph 1: task {bad}" + SUFFIX)
    refused(batch, lambda: b.complete_tasks([None, [LIVE, bad]], resource_caps=False), RANGE,
            f"graph 1: task {bad}" + SUFFIX)
    refused(batch, lambda: b.add_tasks([None, task_list([NEW], [0, 1], [AGG])], unsched_ids=[None, [AGG, bad]]), RANGE,
            f"graph 1: unscheduled aggregator {bad}" + SUFFIX)
    refused(batch, lambda: b.remove_resources([None, [RACK, bad]]), RANGE, f"graph 1: root {bad}" + SUFFIX)
    refused(batch, lambda: b.add_resources([None, ([(SPAN, MACHINE, 0, 0), (bad, PU, 2, 0)], [])]), RANGE,
            f"graph 1: resource node id {bad}" + SUFFIX)
    refused(batch, lambda: b.update_nodes([None, node_list([X, bad], [0, 0, 0], [])]), RANGE,
            f"graph 1: node {bad}" + SUFFIX)


# ------------------------------- heads the device checks while it translates them ---
@pytest.mark.parametrize("bad", [0, SPAN + 1])
def test_heads_outside_the_graph(batch, bad):
    b = batch[0]
    good0 = task_list([369], [0, 1], [66])   # a good list of graph 0 in the same call: arc 0 of the union is its
    refused(batch, lambda: b.add_tasks([good0, task_list([NEW], [0, 2], [AGG, bad])]), RANGE,
            f"rank 0: graph 1: task 249: head {bad}" + SUFFIX)
    refused(batch, lambda: b.update_tasks([None, task_list([LIVE, LIVE + 1], [0, 1, 3], [AGG, AGG, bad])]), RANGE,
            f"rank 0: graph 1: task 50: head {bad}" + SUFFIX)
    refused(batch, lambda: b.update_nodes([None, node_list([RACK, X], [0, 0, 1], [bad])], keep_unlisted=True), RANGE,
            f"rank 0: graph 1: node 2: head {bad}" + SUFFIX)
    mach = [(SPAN, MACHINE, 0, 0)]
    refused(batch, lambda: b.add_resources([None, (mach, [(bad, SPAN, 2, TREE)])]), RANGE,
            f"rank 0: graph 1: edge {bad} -> 264: parent {bad}" + SUFFIX)
    refused(batch, lambda: b.add_resources([None, (mach, [(RACK, SPAN, 2, TREE), (SPAN, bad, 1, TREE)])]), RANGE,
            f"rank 0: graph 1: edge 264 -> {bad}: child {bad}" + SUFFIX)


# ---------------------------------------------------------- the rules of a call ---
def test_one_aggregator_rule_per_call(batch):
    b = batch[0]
    lists = [task_list([369], [0, 1], [66]), task_list([NEW], [0, 1], [AGG])]
    refused(batch, lambda: b.add_tasks(lists, unsched_ids=[[66], None]), INVALID,
            "graph 1: either every listed graph passes unsched_ids or none does (one rule per call)")
    refused(batch, lambda: b.complete_tasks([[69], [LIVE]], resource_caps=False, unsched_ids=[[66], None]), INVALID,
            "graph 1: either every listed graph passes unsched_ids or none does (one rule per call)")


@pytest.mark.parametrize("n", [1, 3])
def test_list_count_differs(batch, n):
    """Through the C entry points: the wrappers always pass one list per loaded graph."""
    b = batch[0]
    L, h = b._L, b._h
    tl, _ = native.pack_task_lists(n, None)
    nl, _ = native.pack_node_lists(n, None)
    rl = (native.KsBatchResList * n)()
    nr, ne = C.c_size_t(), C.c_size_t()
    calls = [lambda: L.ks_batch_add_tasks(h, 0, n, tl, 0, None),
             lambda: L.ks_batch_complete_tasks(h, 0, n, tl, None, None),
             lambda: L.ks_batch_update_tasks(h, 0, n, tl, 0, None),
             lambda: L.ks_batch_add_resources(h, 0, n, rl, None),
             lambda: L.ks_batch_remove_resources(h, 0, n, rl, None, 0, C.byref(nr), None, None, 0, C.byref(ne), None),
             lambda: L.ks_batch_update_nodes(h, 0, n, nl, None)]
    for call in calls:
        refused(batch, lambda: b._check(call()), INVALID, "the list count differs from the loaded graphs")
