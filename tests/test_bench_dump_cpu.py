"""CPU: bench.py's --dump-outputs helpers (no device: the arrays are given)."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_pu_load_counts_tasks_per_pu():
    M, R = 4, 2
    pu0 = 3 + R + M                                   # gen.quincy's first PU node id
    pus = np.array([pu0, pu0 + 3, 0, pu0, pu0 + 3, pu0 + 3, 0], np.uint64)
    assert bench.pu_load(pus, M, R).tolist() == [2, 0, 0, 3]
    assert bench.pu_load(np.zeros(5, np.int64), M, R).tolist() == [0, 0, 0, 0]


def test_dump_outputs_writes_float64_npy(tmp_path):
    d = tmp_path / "out"
    args = argparse.Namespace(dump_outputs=str(d))
    bench.dump_outputs(args, types.SimpleNamespace(rank=0), cost=[3257656], flow=[100000],
                       pu_load=np.arange(7, dtype=np.int64))
    assert sorted(os.listdir(d)) == ["cost.npy", "flow.npy", "pu_load.npy"]
    for name, want in (("cost", [3257656.0]), ("flow", [100000.0]), ("pu_load", list(range(7)))):
        a = np.load(d / f"{name}.npy")
        assert a.dtype == np.float64 and a.tolist() == want
    bench.dump_outputs(args, types.SimpleNamespace(rank=1), cost=[1])
    assert os.path.exists(d / "cost.rank1.npy")
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), types.SimpleNamespace(rank=0), cost=[1])
