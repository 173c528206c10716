"""The host side of tests/test_gpu_batch_tasks.py: one CellModel per graph of a batch, moved only
by the host restatements of the lone calls (arrive_ref, complete_ref, refresh_ref, commit_ref,
preempt_ref) run on the cell's OWN graph in its own ids. Nothing read from the device goes into a
model except a commit's scheduling deltas, which are the solver's answer and checked on their
own. Test infrastructure: no product code uses it."""
from __future__ import annotations

import numpy as np

from arrive_ref import arrive_reference
from commit_ref import TASK, arc_table, commit_reference
from complete_ref import complete_reference
from preempt_ref import preempt_reference, table_graph
from refresh_ref import refresh_reference

KS_COST_SET, KS_COST_ADD = 0, 1


class CellModel:
    def __init__(self, cell):
        g = cell.graph()
        self.cell = cell
        self.ntype = [int(t) for t in g.ntype]
        self.supply = [int(s) for s in g.supply]
        self.arcs = {k: v for k, v in arc_table(g).items() if v[1] > 0}
        self.alive = set(range(1, g.n + 1))
        self.bind: dict = {}
        self.sink = cell.SINK
        self.aggs = [cell.U0 + j for j in range(cell.J)]
        self.n0 = g.n                      # the highest id at the load: span = n0 + the reserved ids
        self.free: list = []               # completed ids, reused first

    # ------------------------------------------------------------------ views
    def graph(self):
        return table_graph(self.ntype, self.supply, self.arcs)

    def nodes(self) -> dict:
        return {i: (self.ntype[i - 1], self.supply[i - 1]) for i in sorted(self.alive)}

    def tasks(self, bound=None) -> list:
        out = [i for i in sorted(self.alive) if self.ntype[i - 1] == TASK]
        if bound is None:
            return out
        return [t for t in out if bool(self.bind.get(t, 0)) == bound]

    def new_ids(self, k: int) -> list:
        """k ids for arriving tasks: freed ones first (in the order they were freed), then fresh ones."""
        out = self.free[:k]
        self.free = self.free[k:]
        top = len(self.ntype)
        return out + list(range(top + 1, top + 1 + k - len(out)))

    def lists(self, tasks, narcs: int, base_cost: int = 40) -> list:
        """narcs (head, cost) pairs per task: its job's aggregator first, then the cluster node, a rack
        and machines, as the Quincy shape has them."""
        c = self.cell
        out = []
        for i, t in enumerate(tasks):
            j = (t + i) % c.J
            heads = [c.U0 + j, c.X, c.RACK0 + (t % c.R), c.MACH0 + (t % c.M), c.MACH0 + ((t + 7) % c.M)]
            if heads[3] == heads[4]:
                heads[4] = c.MACH0 + ((t + 1) % c.M)
            out.append([(h, base_cost * (q + 1) + (t % 13)) for q, h in enumerate(heads[:narcs])])
        return out

    def _fix_sink(self):
        self.supply[self.sink - 1] = -sum(self.supply[i - 1] for i in self.alive if i != self.sink)

    # ------------------------------------------------------------------ calls
    def arrive(self, tasks, lists, unsched_ids=None, sink_cost: int = 0) -> dict:
        r = arrive_reference(self.graph(), tasks, lists, unsched_ids, sink_cost, alive=self.alive)
        self.arcs, self.ntype, self.supply, self.alive = dict(r.arcs), list(r.ntype), list(r.supply), set(r.alive)
        self._fix_sink()
        return r.stats

    def complete(self, tasks, caps: bool, preemptive: bool, unsched_ids=None):
        r = complete_reference(self.graph(), tasks, self.bind, caps, preemptive, unsched_ids, alive=self.alive)
        self.arcs, self.bind = dict(r.arcs), dict(r.bindings)
        for t in r.removed:
            self.alive.discard(t)
            self.ntype[t - 1] = self.supply[t - 1] = 0
            self.free.append(t)
        self._fix_sink()
        return r.left, r.stats

    def refresh(self, tasks, lists, unsched_ids=None, sink_cost: int = 0, flags: int = 0) -> dict:
        r = refresh_reference(self.ntype, self.arcs, tasks, lists, self.bind, unsched_ids, sink_cost, flags,
                              alive=self.alive)
        self.arcs = dict(r.arcs)
        return r.stats

    def commit_pinned(self, placed: dict, continuation: int):
        self.arcs = dict(commit_reference(self.graph(), placed, continuation, True))
        self.bind.update(placed)

    def commit_preemptive(self, deltas, continuation: int, preemption: int) -> dict:
        want, self.bind, st = preempt_reference(self.graph(), deltas, self.bind, continuation, preemption, True)
        self.arcs = dict(want)
        return st

    def age(self, cost: int, mode: int, continuation: int, aggs=None) -> int:
        """UpdateAllCostsToUnscheduledAggs: a running task with an arc into an aggregator gets its running
        arc set to the continuation cost, any other its arc into the aggregator set to / raised by cost."""
        aggs = set(self.aggs if aggs is None else aggs)
        running = {s: (s, d) for (s, d), a in self.arcs.items() if a[3] == 1 and self.ntype[s - 1] == TASK}
        changed = 0
        for (s, d), (lo, cap, co, ty) in list(self.arcs.items()):
            if self.ntype[s - 1] != TASK or d not in aggs:
                continue
            if s in running:
                k = running[s]
                a = self.arcs[k]
                if a[2] != continuation:
                    self.arcs[k] = (a[0], a[1], continuation, a[3])
                    changed += 1
            else:
                new = co + cost if mode == KS_COST_ADD else cost
                if new != co:
                    self.arcs[(s, d)] = (lo, cap, new, ty)
                    changed += 1
        return changed


def offsets(lists):
    off, dst, cost = [0], [], []
    for lst in lists:
        dst += [d for d, _ in lst]
        cost += [c for _, c in lst]
        off.append(len(dst))
    return (np.asarray(off, np.uint64), np.asarray(dst, np.uint64), np.asarray(cost, np.int64))


def sum_stats(stats) -> dict:
    out: dict = {}
    for st in stats:
        for k, v in st.items():
            out[k] = out.get(k, 0) + v
    return out
