"""GPU: the log_cycles line of each device delta call. tools/*_measure.py read their
timings out of these lines, so each call must write exactly one line that the tool's own
pattern matches, and the record count in it is the call's stats' `records`. The graph is the
smallest on which every call emits a record: one sink, one machine with one PU of 2 slots,
one unscheduled aggregator, two tasks."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

from ksched_amd import gen, native

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


@functools.lru_cache(maxsize=None)
def tool(name):
    """tools/<name>.py as a module, loaded by its path (tools/ is no package of the suite)."""
    spec = importlib.util.spec_from_file_location("delta_log_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Stderr = tool("commit_measure").Stderr

SINK, MACHINE, PU, U, T1, T2 = 1, 2, 3, 4, 5, 6


def tiny() -> gen.Graph:
    ntype = np.asarray([3, 4, 2, 0, 1, 1], np.int32)
    supply = np.asarray([-2, 0, 0, 0, 1, 1], np.int64)
    rows = [(U, SINK, 0, 2, 0), (MACHINE, PU, 0, 2, 0), (PU, SINK, 0, 2, 0)]
    for t in (T1, T2):
        rows += [(t, U, 0, 1, 100), (t, MACHINE, 0, 1, 1)]
    a = np.asarray(rows, np.int64)
    return gen.Graph(ntype, supply, a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), a[:, 4].copy())


def logged(call, solve=False):
    """The call on a fresh log_cycles context holding the tiny graph; → (what it returned, the
    text the library wrote to fd 2 during it)."""
    with native.Context(0, log_cycles=1) as ctx:
        with Stderr():
            ctx.load_graph(tiny())
            if solve:
                ctx.solve()
        with Stderr() as log:
            out = call(ctx)
    return out, log.text


def check(text, pattern, group, stats):
    lines = list(re.finditer(pattern, text))
    assert len(lines) == 1, text
    assert stats["records"] > 0
    assert int(lines[0].group(group)) == stats["records"], (lines[0].group(0), stats)


def test_commit_schedule_line():
    (_, stats), text = logged(lambda c: c.commit_schedule(), solve=True)
    check(text, tool("commit_measure").COMMIT_RE, 1, stats)


def test_commit_preemptive_line():
    (_, stats), text = logged(lambda c: c.commit_preemptive(preemption=150), solve=True)
    check(text, tool("commit_measure").COMMIT_RE, 1, stats)


def test_remove_resources_line():
    (removed, _, stats), text = logged(lambda c: c.remove_resources([MACHINE]))
    assert removed.tolist() == [MACHINE, PU]
    check(text, tool("remove_measure").REMOVE_RE, 3, stats)


def test_complete_tasks_line():
    (_, stats), text = logged(lambda c: c.complete_tasks([T1]))
    check(text, tool("complete_measure").COMPLETE_RE, 2, stats)


def test_add_tasks_line():
    stats, text = logged(lambda c: c.add_tasks([7], [0, 2], [U, MACHINE], [100, 1]))
    check(text, tool("add_measure").ADD_RE, 3, stats)


def test_add_resources_line():
    nodes = [(7, 4, 0, 0), (8, 2, 2, 0)]   # (id, type, slots, sink cost): a second machine and its PU
    stats, text = logged(lambda c: c.add_resources(nodes, [(7, 8, 0, 0)]))
    check(text, tool("grow_measure").GROW_RE, 3, stats)


def test_update_tasks_line():
    stats, text = logged(lambda c: c.update_tasks([T1], [0, 2], [U, MACHINE], [100, 5]))
    check(text, tool("update_measure").UPD_RE, 3, stats)
