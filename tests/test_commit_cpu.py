"""CPU suite: ks_commit_schedule's host-visible pieces. The ks_commit_stats layout
equals the ctypes struct, and the rule the GPU tests hold the device to
(tests/commit_ref.py) equals the churn model's own pin and capacity steps
(ksched_amd/churn.py steps 1 and 5), arc for arc including the arc types."""
import ctypes as C
import os
import subprocess

import pytest

from commit_ref import arc_table, commit_reference
from ksched_amd import churn, native
from oracle import ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ksmcmf.h"
#define P(T, F) printf(#T "." #F " %zu\n", offsetof(T, F))
int main(void) {
  printf("ks_commit_stats %zu\n", sizeof(ks_commit_stats));
  P(ks_commit_stats, placed); P(ks_commit_stats, arcs_removed); P(ks_commit_stats, running_added);
  P(ks_commit_stats, running_converted); P(ks_commit_stats, unsched_updates); P(ks_commit_stats, cap_updates);
  P(ks_commit_stats, records); P(ks_commit_stats, reserved);
  printf("KS_COMMIT_RESOURCE_CAPS %d\n", KS_COMMIT_RESOURCE_CAPS);
  return 0;
}
"""


def test_commit_stats_layout_matches_binding(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["ks_commit_stats"] == C.sizeof(native.KsCommitStats) == 96
    for f, _ in native.KsCommitStats._fields_:
        assert getattr(native.KsCommitStats, f).offset == out[f"ks_commit_stats.{f}"], f
    assert out["KS_COMMIT_RESOURCE_CAPS"] == native.KS_COMMIT_RESOURCE_CAPS
    assert "ks_commit_schedule" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "ks_commit_schedule")
    assert native.load().ks_abi_version() == 5       # no struct changed layout


@pytest.mark.parametrize("shape", [(200, 20, 4, 5, 3), (1000, 100, 5, 10, 7)])
def test_commit_reference_equals_the_churn_model(shape):
    """Three rounds, 5 % churn in between: the rule applied to the cell's graph and
    the oracle's placements gives the cell's graph after its own pin step."""
    cell = churn.Cell(*shape)
    T = shape[0]
    pins = 0
    for rnd in range(3):
        g = cell.graph()
        st, _, _, fl = ko.cost_scaling(g)
        assert st == 0
        mp = ko.bfs_mapping(g, fl)
        waiting = set(cell.task_ids(cell.WAIT).tolist())
        placed = {t: p for t, p in mp.items() if t in waiting}
        pins += len(placed)
        want = commit_reference(g, placed, 0, True)
        host = cell.step(mp, 0, 0, age_cost=0, seed=100 + rnd)
        got = {k: a for k, a in arc_table(cell.graph()).items() if a[1] > 0}
        assert got == want, rnd
        if rnd == 0 and shape[0] == 200:
            assert (len(placed), host.shape[0]) == (193, 1207)
        # without the capacity refresh the resource arcs keep their values
        part = commit_reference(g, placed, 0, False)
        was = arc_table(g)
        assert all(part[k] == was[k] for k in part if k[0] < cell.U0 and k[1] != cell.SINK)
        cell.step({}, T // 20, T // 20, seed=200 + rnd)
    assert pins > 0
