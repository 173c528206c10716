"""The host side of tests/test_gpu_batch_resources.py: a CellModel (batch_tasks_ref.py) that also
knows what a caller knows of its resources — the tree (child → parent), the PUs' slots and an id
allocator — and moves through the host restatements of the two resource calls (remove_ref,
grow_ref) run on the cell's OWN graph in its own ids. Nothing read from the device goes into a
model except a commit's scheduling deltas. Test infrastructure: no product code uses it."""
from __future__ import annotations

from batch_tasks_ref import CellModel
from commit_ref import MACHINE, PU, SINK, TASK, arc_table
from complete_ref import complete_reference
from grow_ref import TREE, chain, grow_reference, tree_parents
from remove_ref import remove_reference

TREE_COST = {MACHINE: 2, PU: 1}      # the cost an edge carries when the device creates its arc


class ResCellModel(CellModel):
    def __init__(self, cell):
        super().__init__(cell)
        full = arc_table(cell.graph())                                  # (also arcs whose capacity is 0)
        self.parent = tree_parents(self.ntype, full)
        self.slots = {s: a[1] for (s, d), a in full.items() if d == self.sink and self.ntype[s - 1] == PU}
        self.res_free: list = []                                        # removed resource ids, reused first

    # ------------------------------------------------------------------ views
    def subtree(self, v) -> list:
        out = [v]
        for c in sorted(c for c, p in self.parent.items() if p == v):
            out += self.subtree(c)
        return out

    def named_roots(self, roots) -> list:
        """The roots plus every node beneath them that no arc reaches any more (pinned: a full PU has
        lost the arc from its machine, a full machine the arc from its rack): the walk cannot find
        those, so the caller names them, from its own tree and the model's own arcs."""
        tree = sorted({v for r in roots for v in self.subtree(r)})
        return list(roots) + [v for v in tree if v not in roots and (self.parent[v], v) not in self.arcs]

    def new_res_ids(self, k: int, fresh: bool = False) -> list:
        """k ids for new resources: freed resource ids first (unless fresh), then ids past the highest."""
        out = [] if fresh else self.res_free[:k]
        self.res_free = self.res_free[len(out):]
        top = len(self.ntype)
        return out + list(range(top + 1, top + 1 + k - len(out)))

    def machine(self, rack: int, ids, slots: int = 3, sink_cost: int = 0):
        """A machine and its one PU beneath rack, the chain listed up to the cluster node:
        → (nodes, edges) as ks_add_resources takes them. ids: (machine id, PU id)."""
        mid, pid = ids
        nodes = [(mid, MACHINE, 0, 0), (pid, PU, slots, sink_cost)]
        edges = [(rack, mid, TREE_COST[MACHINE], TREE), (mid, pid, TREE_COST[PU], TREE)] + chain(self.parent, rack)
        return nodes, edges

    def relist(self, tasks, base_cost: int = 40) -> list:
        """The arcs an evicted task gets back through ks_update_tasks: its job's aggregator first,
        then the heads of CellModel.lists that are still alive."""
        out = []
        for lst in self.lists(tasks, 5, base_cost):
            out.append([lst[0]] + [(h, c) for h, c in lst[1:] if h in self.alive])
        return out

    # ------------------------------------------------------------------ calls
    def remove(self, roots, caps: bool, preemptive: bool):
        r = remove_reference(self.graph(), roots, self.bind, caps, preemptive, alive=self.alive)
        self.arcs, self.bind = dict(r.arcs), dict(r.bindings)
        for v in r.removed:
            self.alive.discard(v)
            self.ntype[v - 1] = self.supply[v - 1] = 0
            self.parent.pop(v, None)
            self.slots.pop(v, None)
            self.res_free.append(v)
        return r.removed, r.evicted, r.stats

    def grow(self, nodes, edges) -> dict:
        r = grow_reference(self.graph(), nodes, edges, alive=self.alive)
        self.arcs, self.ntype, self.supply, self.alive = dict(r.arcs), list(r.ntype), list(r.supply), set(r.alive)
        new = {n[0] for n in nodes}
        for i, ty, s, _ in nodes:
            if ty == PU:
                self.slots[i] = s
        for p, c, _, kind in edges:
            if kind == TREE and c in new:
                self.parent[c] = p
        return r.stats

    def refresh_caps(self, preemptive: bool) -> dict:
        """ks_complete_tasks with k == 0 and the caps flag: the plain capacity refresh."""
        _, st = self.complete([], True, preemptive)
        return st

    # ------------------------------------------------------------- invariants
    def stale_caps(self, preemptive: bool) -> int:
        """The records a capacity refresh would still write."""
        r = complete_reference(self.graph(), [], self.bind, True, preemptive, None, alive=self.alive)
        return r.stats["records"]

    def dangling(self) -> list:
        return [(s, d) for (s, d) in self.arcs if s not in self.alive or d not in self.alive]

    def one_sink(self) -> bool:
        return [i for i in self.alive if self.ntype[i - 1] == SINK] == [self.sink]

    def waiting_without_arc(self) -> list:
        has = {s for (s, d) in self.arcs}
        return [t for t in self.alive if self.ntype[t - 1] == TASK and t not in has]
