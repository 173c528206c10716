"""The host side of tests/test_gpu_batch_nodes.py: a ResCellModel (batch_resources_ref.py) that
also moves through the host restatement of ks_update_nodes (nodes_ref.nodes_reference) run on the
cell's OWN graph in its own ids, and the lists a caller WITHOUT a shadow of the cell's arcs would
write, from what it knows itself: its resource tree, the PUs' slots, the bindings the commits told
it and its cost model. In a Quincy cell the cluster node X and the racks are type-0 nodes, so
X → rack and rack → machine are class arcs (an unlisted one is deleted, and they are listed with an
explicit capacity: the head's room under the mode's capacity rule); machine → PU and PU → sink are
resource arcs (KS_CAP_KEEP where the caller knows the store to hold the arc). Nothing read from the
device goes into a model. Test infrastructure: no product code uses it."""
from __future__ import annotations

from batch_resources_ref import ResCellModel
from commit_ref import MACHINE, PU
from nodes_ref import CAP_KEEP, KEEP_UNLISTED, nodes_reference

SPREAD = 7          # what one bound task beneath a head adds to the cost of an arc into it
RACK_COST, MACH_COST, SINK_COST = 5, 2, 0


class NodeCellModel(ResCellModel):
    # ------------------------------------------------------------------ the call
    def update_nodes(self, nodes, lists, keep: bool = False) -> dict:
        r = nodes_reference(self.ntype, self.arcs, nodes, lists, KEEP_UNLISTED if keep else 0, alive=self.alive)
        self.arcs = dict(r.arcs)
        for u, lst in zip(nodes, lists):                    # a PU → sink arc with a capacity is a new slot count
            for d, _, cap in lst:
                if self.ntype[u - 1] == PU and d == self.sink and cap != CAP_KEEP:
                    self.slots[u] = int(cap)
        return r.stats

    # ------------------------------------------------ what the caller knows itself
    def children(self, v) -> list:
        return sorted(c for c, p in self.parent.items() if p == v)

    def pus_beneath(self, v) -> list:
        return [p for p in self.subtree(v) if p in self.slots]

    def load(self) -> dict:
        n: dict = {}
        for p in self.bind.values():
            if p:
                n[p] = n.get(p, 0) + 1
        return n

    def bound_beneath(self, v, load=None) -> int:
        load = self.load() if load is None else load
        return sum(load.get(p, 0) for p in self.pus_beneath(v))

    def room(self, v, preemptive: bool, load=None) -> int:
        """What the capacity rule gives an arc into v: the slots beneath it, minus the bound tasks
        under the pinned rule."""
        load = self.load() if load is None else load
        return sum(self.slots[p] - (0 if preemptive else load.get(p, 0)) for p in self.pus_beneath(v))

    def blocked(self, v, preemptive: bool, load=None) -> bool:
        """No arc leads into v under the pinned rule: a full PU, a node whose children are all blocked."""
        load = self.load() if load is None else load
        if v in self.slots:
            return not preemptive and load.get(v, 0) >= self.slots[v]
        return all(self.blocked(c, preemptive, load) for c in self.children(v))

    def blocked_nodes(self, preemptive: bool) -> set:
        """The resource nodes no arc leads into, as the caller knows them right after a commit. The
        pinned rule deleted those arcs, and a completion that frees a slot beneath one does not bring
        them back: while such a node has room again its in-arc is listed with an explicit capacity."""
        load = self.load()
        return {v for v in self.parent if self.blocked(v, preemptive, load)}

    def freed(self, marked, preemptive: bool) -> set:
        """Of the nodes blocked at the last commit, those that are still there and have room now."""
        load = self.load()
        return {v for v in marked if v in self.parent and not self.blocked(v, preemptive, load)}

    def racks(self) -> list:
        return [r for r in self.children(self.cell.X)]

    def machines(self) -> list:
        return sorted(i for i in self.alive if self.ntype[i - 1] == MACHINE)

    # -------------------------------------------- the lists of a caller without a shadow
    def class_list(self, heads, base: int, preemptive: bool, load=None, was_blocked=()) -> list:
        """(head, cost, cap) of a type-0 tail's arcs into resource heads, the capacity explicit: the
        head's room (0 while it is full: skipped or zeroed), at least 1 for a head that was blocked
        until this call gave a PU beneath it a slot; the cost follows the load beneath the head."""
        load = self.load() if load is None else load
        return [(h, base + SPREAD * self.bound_beneath(h, load),
                 max(self.room(h, preemptive, load), 1 if h in was_blocked else 0)) for h in heads]

    def cost_lists(self, preemptive: bool, was_blocked=()) -> tuple:
        """→ (tails, lists): X → rack and rack → machine costs from the load, the capacities explicit."""
        load = self.load()
        tails = [self.cell.X] + self.racks()
        lists = [self.class_list(self.racks(), RACK_COST, preemptive, load, was_blocked)]
        lists += [self.class_list(self.children(r), MACH_COST, preemptive, load, was_blocked) for r in self.racks()]
        return tails, lists

    def pu_lists(self, preemptive: bool, resized=None, was_blocked=()) -> tuple:
        """→ (tails, lists): machine → PU re-costed with KS_CAP_KEEP where the arc is known to be held
        (an explicit capacity into a PU of was_blocked, nothing into a PU that stays full), every PU → sink
        re-costed with KS_CAP_KEEP, the PUs of resized {pu: slots} with their new slot count."""
        load = self.load()
        resized = resized or {}
        tails, lists = [], []
        for u in self.machines():
            lst = []
            for p in self.children(u):
                if p in was_blocked:
                    lst.append((p, 1 + load.get(p, 0) // 2, max(self.room(p, preemptive, load), 1)))
                elif not self.blocked(p, preemptive, load):
                    lst.append((p, 1 + load.get(p, 0) // 2, CAP_KEEP))
            tails.append(u)
            lists.append(lst)
        for p in sorted(self.slots):
            tails.append(p)
            lists.append([(self.sink, SINK_COST + load.get(p, 0) // 2, resized.get(p, CAP_KEEP))])
        return tails, lists

    def blocked_chain(self, p, preemptive: bool) -> set:
        """A PU about to gain a slot and its ancestors that are blocked with it: the arcs into these
        went with the pinned rule, so they are listed with an explicit capacity."""
        out, v, load = set(), p, self.load()
        while v in self.parent and self.blocked(v, preemptive, load):
            out.add(v)
            v = self.parent[v]
        return out
