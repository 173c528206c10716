"""CPU: ks_batch_update_nodes without a device. The C-ABI surface (the ABI version, the size and
the fields of ks_batch_node_list, the bound symbol, KS_E_INVALID on a null handle), and the claim
the batch call rests on: ks_update_nodes' rule run on a union of cells, the tails and heads moved
into the union's ids, gives per cell exactly what the rule gives on the cell alone, and the summed
statistics. The six cells of the GPU suite are laid out with ks_batch_node_offsets, 256 reserved
ids each, cold, pinned and preemptive, under seeded lists of a caller without a shadow
(batch_nodes_ref.NodeCellModel). The last case states why the range check of the translate kernel
is needed: a head of span + 1 in cell 0 is a live node of cell 1 in the union, and the lone rule
accepts it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from batch_nodes_ref import NodeCellModel
from batch_tasks_ref import sum_stats
from commit_ref import OTHER
from ksched_amd import churn, native
from nodes_ref import CAP_KEEP, KEEP_UNLISTED, nodes_reference
from oracle import ko
from test_batch_resources_cpu import CELLS, STATES, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARE = 256


@pytest.fixture(scope="module")
def lib():
    return native.load(build_if_missing=False)


# ------------------------------------------------------------------- the surface ---
def test_abi_version_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "ksmcmf.h")).read()
    assert re.search(r"#define KSMCMF_ABI_VERSION (\d+)", header).group(1) == "5"
    assert lib.ks_abi_version() == native.ABI_VERSION == 5
    # three pointers and one size_t, no padding: sizeof(ks_batch_node_list) on an LP64 target
    assert C.sizeof(native.KsBatchNodeList) == 3 * C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t) == 32
    fields = re.search(r"typedef struct ks_batch_node_list \{(.*?)\} ks_batch_node_list;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert [f for f, _ in native.KsBatchNodeList._fields_] == re.findall(r"(\w+);", fields)
    assert re.findall(r"(\w+)\s*\*?\s*\w+;", fields) == ["uint64_t", "size_t", "uint64_t", "ks_node_arc"]
    assert native.NODE_ARC_DT.itemsize == 24


def test_symbol_is_exported_and_bound(lib):
    assert "ks_batch_update_nodes" in native.EXPORTED_SYMBOLS
    assert lib.ks_batch_update_nodes.argtypes is not None


def test_null_handle_is_invalid(lib):
    one = (native.KsBatchNodeList * 1)()
    st = native.KsNodeStats()
    st.nodes = 7
    assert lib.ks_batch_update_nodes(None, 0, 1, one, C.byref(st)) == native.KS_E_INVALID
    assert st.nodes == 7                                    # nothing is written on a null handle


def test_the_packer():
    ls, keep = native.pack_node_lists(3, [None, ([4, 5], [0, 1, 3], [7, 8, 9], [1, -2, 3], [1, CAP_KEEP, 0]), None])
    assert ls[0].k == ls[2].k == 0 and not ls[0].nodes and not ls[2].arcs and keep[0] is None
    assert ls[1].k == 2 and keep[1]["arcs"].dtype == native.NODE_ARC_DT
    assert keep[1]["arcs"]["cap"].tolist() == [1, CAP_KEEP, 0] and keep[1]["arcs"]["cost"].tolist() == [1, -2, 3]
    assert ls[1].arcs == keep[1]["arcs"].ctypes.data and ls[1].arc_off == keep[1]["arc_off"].ctypes.data
    with pytest.raises(ValueError):
        native.pack_node_lists(2, [None])
    with pytest.raises(ValueError):
        native.pack_node_lists(1, [([4], [0, 1, 2], [7], [1], [1])])
    with pytest.raises(ValueError):
        native.pack_node_lists(1, [([4], [0, 1], [7], [1, 2], [1])])


def test_documents_name_the_batch_twin():
    for name in ("include/ksmcmf.h", "README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "ks_batch_update_nodes" in text, name
    for name in ("include/ksmcmf.h", "INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, name)).read().lower()
        assert "no batch twin" not in text, name


# ------------------------------------------------------------ the union and the cells ---
def models_in(state):
    models = [NodeCellModel(churn.Cell(*p)) for p in CELLS]
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


def union_of(models):
    """The cells as one graph in a device's ids: (offsets, node types with the reserved ids dead,
    the live ids, the arc table cell after cell)."""
    off = native.batch_node_offsets([m.n0 for m in models], SPARE).tolist()
    assert [b - a for a, b in zip(off, off[1:])] == [m.n0 + SPARE for m in models]
    ntype, alive, table = [0] * off[-1], set(), {}
    for m, lo in zip(models, off):
        ntype[lo:lo + len(m.ntype)] = m.ntype
        alive |= {i + lo for i in m.alive}
        table.update({(s + lo, d + lo): a for (s, d), a in m.arcs.items()})
    return off, ntype, alive, table


def seeded_lists(m, rng, preemptive):
    """A seeded part of the lists of a caller without a shadow: X and some racks with their costs from
    the load, one rack with a machine dropped from its list (the unlisted arc is deleted) and a
    machine of another rack in it (added), some machines and PUs with KS_CAP_KEEP, one PU resized."""
    tails, lists = m.cost_lists(preemptive)
    pick = sorted(rng.choice(len(tails), max(2, len(tails) // 2), replace=False).tolist())
    tails, lists = [tails[i] for i in pick], [list(lists[i]) for i in pick]
    racks = [i for i, u in enumerate(tails) if u != m.cell.X]
    if racks and len(lists[racks[0]]) > 1:
        i = racks[0]
        other = next(x for x in m.machines() if m.parent[x] != tails[i])
        lists[i] = lists[i][1:] + m.class_list([other], 11, preemptive, was_blocked=[other])     # (capacity ≥ 1: added)
    pus = sorted(m.slots)
    grown = int(rng.choice([p for p in pus if not m.blocked(p, preemptive)] or pus))
    rt, rl = m.pu_lists(preemptive, resized={grown: m.slots[grown] + 2})
    pick = sorted(rng.choice(len(rt), max(3, len(rt) // 3), replace=False).tolist() + [rt.index(grown)])
    pick = sorted(set(pick))
    return tails + [rt[i] for i in pick], lists + [rl[i] for i in pick]


@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
@pytest.mark.parametrize("state", STATES)
def test_the_rule_on_the_union_is_the_rule_per_cell(state, keep):
    pre = state == "preemptive"
    models = models_in(state)
    rng = np.random.default_rng(91 + STATES.index(state))
    off, ntype, alive, table = union_of(models)
    per = {g: seeded_lists(models[g], rng, pre) for g in (0, 1, 3, 5)}        # cells 2 and 4 are unlisted
    nodes = [u + off[g] for g, (tails, _) in per.items() for u in tails]
    lists = [[(d + off[g], c, cap) for d, c, cap in lst] for g, (_, ls) in per.items() for lst in ls]
    r = nodes_reference(ntype, table, nodes, lists, KEEP_UNLISTED if keep else 0, alive=alive)
    want = [models[g].update_nodes(tails, ls, keep) for g, (tails, ls) in per.items()]
    assert r.stats == sum_stats(want)
    assert r.stats["arcs_added"] and r.stats["arcs_updated"]
    # (pinned: every machine is full after the commit, so the dropped rack → machine arc was gone already)
    assert keep or state == "pinned" or r.stats["arcs_removed"]
    for g, m in enumerate(models):
        lo, hi = off[g], off[g + 1]
        mine = {(s - lo, d - lo): a for (s, d), a in r.arcs.items() if lo < s <= hi}
        assert all(lo < d <= hi for (s, d) in r.arcs if lo < s <= hi), f"cell {g}: an arc leaves the cell"
        assert mine == m.arcs, f"cell {g}"
    assert len(r.arcs) == sum(len(m.arcs) for m in models)


@pytest.mark.parametrize("state", ["pinned", "preemptive"])
def test_the_no_shadow_lists_leave_a_solvable_cell(state):
    """Every cost of X, the racks, the machines and the PUs re-listed from the caller's own knowledge:
    nothing dangles, the capacity refresh has nothing left to write and the next solve is feasible."""
    pre = state == "preemptive"
    for m in models_in(state):
        tails, lists = m.cost_lists(pre)
        rt, rl = m.pu_lists(pre)
        st = m.update_nodes(tails + rt, lists + rl)
        assert st["arcs_updated"] > 0 and st["arcs_added"] == st["arcs_removed"] == 0
        check(m, pre)


def test_a_head_of_span_plus_one_is_a_live_node_of_the_next_cell():
    """What only the range check can refuse: cell 0's cluster node listed with the head span + 1 is,
    in the union's ids, an arc into cell 1's sink, which the lone rule accepts from a type-0 tail."""
    models = models_in("cold")
    off, ntype, alive, table = union_of(models)
    m = models[0]
    span = m.n0 + SPARE
    assert off[1] == span and span + 1 in alive and models[1].sink == 1
    x = m.cell.X
    assert m.ntype[x - 1] == OTHER
    r = nodes_reference(ntype, table, [x], [[(span + 1, 3, 2)]], KEEP_UNLISTED, alive=alive)
    assert r.stats["arcs_added"] == 1 and (x, span + 1) in r.arcs             # accepted: an arc between two cells
    # the reserved ids of cell 0 itself are dead: span is the lone rule's to refuse
    with pytest.raises(ValueError):
        nodes_reference(ntype, table, [x], [[(span, 3, 2)]], KEEP_UNLISTED, alive=alive)
