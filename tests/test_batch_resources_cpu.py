"""CPU: the resource side of a batch round without a device. The C-ABI surface of
ks_batch_remove_resources and ks_batch_add_resources (the ABI version, the size and the fields of
ks_batch_res_list, the bound symbols, KS_E_INVALID on a null handle), and the host model of
tests/test_gpu_batch_resources.py (batch_resources_ref.ResCellModel) against the oracle on the six
cells of the GPU suite: after every removal, re-listing, growth and refresh no arc dangles, the
capacity refresh has nothing left to write, the next solve is feasible and ko.cost_scaling equals
ko.verify. That is what lets the GPU cases solve after every call of the refresh sequence."""
import ctypes as C
import os
import re

import pytest

from batch_resources_ref import ResCellModel
from ksched_amd import churn, native
from oracle import ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(300, 30, 3, 3, 1600), (300, 30, 3, 3, 1601), (500, 50, 5, 5, 1602), (200, 20, 2, 4, 1603),
         (1000, 100, 5, 10, 1604), (120, 12, 2, 2, 1605)]
STATES = ["cold", "pinned", "preemptive"]
NEW = ("ks_batch_remove_resources", "ks_batch_add_resources")


@pytest.fixture(scope="module")
def lib():
    return native.load(build_if_missing=False)


# ------------------------------------------------------------------- the surface ---
def test_abi_version_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "ksmcmf.h")).read()
    assert re.search(r"#define KSMCMF_ABI_VERSION (\d+)", header).group(1) == "5"
    assert lib.ks_abi_version() == native.ABI_VERSION == 5
    # three pointers and three size_t, no padding: sizeof(ks_batch_res_list) on an LP64 target
    assert C.sizeof(native.KsBatchResList) == 3 * C.sizeof(C.c_void_p) + 3 * C.sizeof(C.c_size_t) == 48
    fields = re.search(r"typedef struct ks_batch_res_list \{(.*?)\} ks_batch_res_list;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert [f for f, _ in native.KsBatchResList._fields_] == re.findall(r"(\w+);", fields)
    assert re.findall(r"(\w+)\s*\*?\s*\w+;", fields) == ["uint64_t", "size_t", "ks_res_node", "size_t", "ks_res_arc",
                                                        "size_t"]


def test_symbols_are_exported_and_bound(lib):
    for sym in NEW:
        assert sym in native.EXPORTED_SYMBOLS
        assert getattr(lib, sym).argtypes is not None


def test_null_handle_is_invalid(lib):
    one = (native.KsBatchResList * 1)()
    nr, ne = C.c_size_t(7), C.c_size_t(7)
    assert lib.ks_batch_remove_resources(None, 1, 1, one, None, 0, C.byref(nr), None, None, 0, C.byref(ne),
                                         None) == native.KS_E_INVALID
    assert (nr.value, ne.value) == (7, 7)                  # nothing is written on a null handle
    assert lib.ks_batch_add_resources(None, 0, 1, one, None) == native.KS_E_INVALID


def test_documents_name_the_batch_twins():
    for name in ("include/ksmcmf.h", "README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "ks_batch_remove_resources" in text and "ks_batch_add_resources" in text, name


# --------------------------------------------------------- the model and the oracle ---
def check(m, preemptive, feasible=True):
    assert m.dangling() == []
    assert m.one_sink()
    assert m.stale_caps(preemptive) == 0, "the capacity refresh has records left to write"
    if not feasible:
        return
    g = m.graph()
    st, cost, flow, fl = ko.cost_scaling(g)
    assert st == 0 and flow == len(m.tasks()), "the next solve is infeasible"
    vst, vcost, _ = ko.verify(g, fl)
    assert (vst, vcost) == (0, cost)


def models_in(state):
    models = [ResCellModel(churn.Cell(*p)) for p in CELLS]
    for m in models:
        if state == "cold":
            continue
        g = m.graph()
        st, _, _, vec, _ = ko.ssp(g)
        assert st == 0
        placed = ko.bfs_mapping(g, vec)
        if state == "pinned":
            m.commit_pinned(placed, 3)
        else:
            m.commit_preemptive([(native.KS_DELTA_PLACE, t, p) for t, p in sorted(placed.items())], 0, 150)
    return models


@pytest.mark.parametrize("state", STATES)
def test_model_against_the_oracle(state):
    pre = state == "preemptive"
    models = models_in(state)
    for m in models:
        check(m, pre)
    # a machine leaves cells 0, 3 and 5, every machine of one rack cell 2 (the rack stays, emptied),
    # a whole rack cell 4
    evicted = {}
    for g in (0, 2, 3, 4, 5):
        m, c = models[g], models[g].cell
        top = {2: [c.MACH0 + k for k in range(c.M) if k % c.R == 0], 4: [c.RACK0 + 1]}.get(g, [c.MACH0 + 1])
        removed, ev, st = m.remove(m.named_roots(top), True, pre)
        assert removed == sorted(removed) and st["nodes_removed"] == len(removed) and st["tasks_evicted"] == len(ev)
        assert st["pus_removed"] == len(removed) // 2 and st["roots"] >= len(top)
        assert (c.RACK0 in m.alive) and (g != 4 or c.RACK0 + 1 not in m.alive)
        evicted[g] = [t for t, _ in ev]
        # pinned: an evicted task has no arc until it is re-listed
        assert bool(m.waiting_without_arc()) == (state == "pinned" and bool(ev))
        check(m, pre, feasible=not m.waiting_without_arc())
    if state != "cold":
        assert any(evicted.values())
    # the evicted tasks get their arcs back, their aggregator's among them
    for g, tasks in evicted.items():
        m = models[g]
        if state == "pinned" and tasks:
            m.refresh(tasks, m.relist(tasks), m.aggs, 0)
            assert not m.waiting_without_arc()
        check(m, pre)
    # a machine joins: with the removal's ids in cells 0 and 5, with fresh ones in cell 1, beneath the
    # emptied rack in cell 2; then the refresh
    for g, fresh in ((0, False), (1, True), (2, False), (5, False)):
        m, c = models[g], models[g].cell
        ids = m.new_res_ids(2, fresh)
        assert fresh == (ids[0] > m.n0)
        nodes, edges = m.machine(c.RACK0 if g == 2 else c.RACK0 + 1, ids)
        st = m.grow(nodes, edges)
        assert st["pus"] == 1 and st["sink_arcs"] == 1 and st["records"] >= 4
        m.refresh_caps(pre)
        check(m, pre)
