"""A caller that keeps no shadow, and the graph it expects: whole scheduling rounds (INTEGRATION
§2.1: commit → ks_remove_resources → ks_complete_tasks → ks_add_resources → the capacity refresh →
ks_add_tasks → ks_update_tasks → ks_update_nodes → ks_update_unsched_costs → solve, and the mapping
read after it: the ten-call round) on the host only.

RoundModel plays ksched's side of the C-ABI and holds the expected graph. The graph evolves only
through the rules the single-call suites already restate (commit_reference, preempt_reference,
remove_reference, complete_reference, grow_reference, arrive_reference, refresh_reference,
nodes_reference, sched_ref.scheduling_deltas / apply_deltas) and one new one, unsched_costs_reference. What the
model knows beside the graph is what a real caller knows: the resource tree, the slots of every
PU, each live task's job and preference list, the bindings and an id allocator. The recipes of
include/ksmcmf.h are issued from that knowledge.

With classes = True (off by default: without it no case draws or adds anything more) every job has
an equivalence class between its tasks and a few preferred machines, and a cost model that moves:
class → machine costs and capacities follow the bindings and the slots, the resource tree's arcs
are re-costed with KS_CAP_KEEP, two rounds change a PU's slot count, and ks_update_nodes carries
all of it each round. The arcs it lists are those the caller KNOWS the store to hold or to lack:
  - class → machine: always with an explicit capacity (the room the capacity rule gives the arc,
    capped at 1 for the classes with an odd index). The pinned rule deletes the arc into a full
    machine, so KS_CAP_KEEP on a class arc is not the caller's to use: an explicit capacity adds
    the arc back once a completion freed a slot, and 0 drops or skips it while the machine is full.
  - a resource arc with KS_CAP_KEEP only into a head that is not blocked(): the rule holds exactly
    those. The arc into a rack with NO slot beneath it is the one whose presence the caller cannot
    know (the rule leaves it as it was: absent if the rack had filled up before it emptied, stale
    otherwise), so it is listed with capacity 0: zeroed when held, skipped when not. No flow could
    use it, and ks_add_resources re-creates it with the right capacity when a machine joins.
  - pinned, a FULL PU that gains a slot: the rule had deleted the arcs into it and into every
    ancestor that was blocked with it, and the capacity refresh that follows the slot change only
    writes arcs that exist. So the caller lists those chain arcs with an explicit positive capacity
    in the same call (ADD_ARC), as the completion recipe does with its upserts; the refresh then
    sets them.

THE RULE: nothing read from ctx.graph() ever becomes an input of the model or of a later call.
A backend (the oracle here, the device in test_gpu_rounds.py) answers the solve; its cost, flow,
flows and mapping are checked against the model's own graph before the mapping is used, and every
other answer of a call (removed, evicted, left, the statistics, the bindings) is compared with the
rule's and the rule's value is the one the model keeps.

Test infrastructure: no product code uses it."""
from __future__ import annotations

import bisect
import json

import numpy as np

from arrive_ref import arrive_reference
from commit_ref import MACHINE, OTHER, PU, SINK, TASK, commit_reference
from complete_ref import chain_upserts, complete_reference, parent_chains
from grow_ref import TREE, chain, grow_reference
from nodes_ref import CAP_KEEP, nodes_reference
from oracle import ko, sched_ref
from preempt_ref import preempt_reference, table_graph
from refresh_ref import refresh_reference
from remove_ref import remove_reference
from store_ref import StoreRef

PLACE, PREEMPT, MIGRATE = sched_ref.PLACE, sched_ref.PREEMPT, sched_ref.MIGRATE
COST_SET, COST_ADD = 0, 1
# the toy cost model: strict gaps, so that the scripted MIGRATE and PREEMPT are unique optima
UNSCHED, WILDCARD, PREEMPTION, AGE, SINK_COST = 1000, 500, 300, 3, 0
CONTINUATION, RAISED_CONTINUATION, LURE = 0, 40, -5000
# ResourceNodeToResourceNodeCost by the child's type: an arc the device re-creates must carry its edge's cost
TREE_COST = {OTHER: 3, MACHINE: 2, PU: 1}
# with classes: task → class at a fixed cost, class → machine at a base drawn once + SPREAD × the tasks bound there
CLASS_COST, SPREAD = 200, 7
COUNTERS = ("evictions", "bound_id_reused", "pu_id_reused", "aggregator_recreated", "ancestor_recreated",
            "migrations", "preemptions", "new_jobs", "superseded", "running_kept", "recipe_upserts", "stale_caps_repaired",
            "class_arcs_added", "class_arcs_removed", "class_arcs_zeroed", "class_arc_recreated", "cap_overwritten",
            "resource_recosted", "resource_unchanged", "slots_raised", "slots_lowered", "chain_relisted", "class_tail_over_64")


def unsched_costs_reference(ntype, arcs: dict, aggs, mode: int, unsched_cost: int, continuation: int):
    """ks_update_unsched_costs (include/ksmcmf.h; UpdateAllCostsToUnscheduledAggs,
    flowmanager/graph_manager.go:462-475): for every task with an arc into a marked aggregator, a
    running task (it has a type-1 arc) gets its running arc set to the continuation cost, any
    other task its arc into the aggregator SET to or raised by unsched_cost. → (arcs, changed)."""
    marked = {int(a) for a in aggs}
    waiting_on = {s for (s, d) in arcs if ntype[s - 1] == TASK and d in marked}
    running = {s for (s, d), a in arcs.items() if ntype[s - 1] == TASK and a[3] == 1}
    out, changed = dict(arcs), 0
    for (s, d), (lo, cap, co, ty) in arcs.items():
        if s not in waiting_on:
            continue
        if d in marked:
            if s in running:
                continue
            new = co + unsched_cost if mode == COST_ADD else unsched_cost
        elif ty == 1:
            new = continuation
        else:
            continue
        if new != co:
            out[(s, d)] = (lo, cap, new, ty)
            changed += 1
    return out, changed


class RoundFailure(AssertionError):
    pass


class RoundModel:
    def __init__(self, preemptive: bool, ntype, supply, arcs: dict, parent: dict, slots: dict, job: dict, prefs: dict,
                 wildcard=None, seed=None):
        self.preemptive, self.seed, self.round = bool(preemptive), seed, 0
        self.ntype, self.supply, self.arcs = [int(t) for t in ntype], [int(s) for s in supply], dict(arcs)
        self.alive = set(range(1, len(self.ntype) + 1))
        self.sink = self.ntype.index(SINK) + 1
        self.bindings: dict = {}
        self.parent, self.slots, self.job, self.prefs = dict(parent), dict(slots), dict(job), {t: list(p) for t, p in prefs.items()}
        self.tree_cost = {c: self.arcs[(p, c)][2] for c, p in self.parent.items() if (p, c) in self.arcs}
        self.wildcard = wildcard                       # X: the cluster aggregator every task may go through
        self.aggs = sorted(set(job.values()))
        self.free: list = []
        self.top = len(self.ntype)
        self.cont = CONTINUATION
        self.returning: list = []                      # evicted or preempted: they come back through ks_update_tasks
        self.count = dict.fromkeys(COUNTERS, 0)
        self.freed_bound: set = set()
        self.freed_pus: set = set()
        self.had_sink_arc = {a for a in self.aggs if (a, self.sink) in self.arcs}   # to tell "re-created" from "new"
        self._held_before: set = set()
        self.log: list = []
        # the classes (empty without the option): what the caller knows of them
        self.cls: dict = {}                            # job (its aggregator) → the job's class node
        self.classes: list = []                        # in the order they were made: the index decides the cap-1 limit
        self.pref: dict = {}                           # class → its preferred machines
        self.base: dict = {}                           # (class, machine) → the base cost, drawn once
        self.caps_from = "rule"                        # who wrote the class arcs' capacities last: "rule" or "model"
        self.commit_dropped: set = set()               # class arcs a commit deleted (into a full machine)
        self.held_down: set = set()                    # cap-1 arcs the last ks_update_nodes wrote below the rule's value

    # ---------------------------------------------------------------- the cluster ---
    @classmethod
    def cluster(cls, preemptive, seed, racks=2, mpr=3, pus=1, slots=2, job_sizes=(8, 8, 8), classes=False):
        """SINK 1, X 2, the racks, the machines (machine k in rack k // mpr), their PUs, one
        unscheduled aggregator per job, [one class per job,] the tasks."""
        rng = np.random.default_rng(seed)
        ntype, supply = [SINK, OTHER], [0, 0]

        def node(ty, s=0):
            ntype.append(ty)
            supply.append(s)
            return len(ntype)
        X = 2
        rk = [node(OTHER) for _ in range(racks)]
        ms = [node(MACHINE) for _ in range(racks * mpr)]
        ps = [node(PU) for _ in range(racks * mpr * pus)]
        ag = [node(OTHER) for _ in job_sizes]
        cl = [node(OTHER) for _ in job_sizes] if classes else []
        arcs, parent, slot = {}, {}, {}
        for r in rk:
            arcs[(X, r)], parent[r] = (0, mpr * pus * slots, TREE_COST[OTHER], 0), X
        for k, m in enumerate(ms):
            arcs[(rk[k // mpr], m)], parent[m] = (0, pus * slots, TREE_COST[MACHINE], 0), rk[k // mpr]
        for k, p in enumerate(ps):
            arcs[(ms[k // pus], p)], parent[p], slot[p] = (0, slots, TREE_COST[PU], 0), ms[k // pus], slots
            arcs[(p, 1)] = (0, slots, SINK_COST, 0)
        job, prefs = {}, {}
        for k, (a, size) in enumerate(zip(ag, job_sizes)):
            arcs[(a, 1)] = (0, size, SINK_COST, 0)
            for _ in range(size):
                t = node(TASK, 1)
                job[t] = a
                prefs[t] = [(int(m), int(c)) for m, c in zip(rng.choice(ms, 2, replace=False), rng.integers(1, 100, 2))]
                for d, c in prefs[t] + ([(cl[k], CLASS_COST)] if cl else []) + [(X, WILDCARD), (a, UNSCHED)]:
                    arcs[(t, d)] = (0, 1, c, 0)
        supply[0] = -len(job)
        m = cls(preemptive, ntype, supply, arcs, parent, slot, job, prefs, wildcard=X, seed=seed)
        m.rng = rng
        for a, c in zip(ag, cl):                         # the graph is loaded with the cost model's arcs of an idle cluster
            m.add_class(a, c)
            for x, co, cap in m.class_list(c, m.draw_class_set(c)):
                m.arcs[(c, x)] = (0, cap, co, 0)
        if cl:
            m.caps_from = "model"
        return m

    # -------------------------------------------------------------------- views ---
    def graph(self):
        return table_graph(self.ntype, self.supply, self.arcs)

    def balanced(self):
        """The graph as auto_sink solves it: the sink's demand is −Σ of the other supplies."""
        supply = list(self.supply)
        supply[self.sink - 1] = 0
        supply[self.sink - 1] = -sum(supply)
        return table_graph(self.ntype, supply, self.arcs)

    def store(self) -> StoreRef:
        nodes = {i: [self.supply[i - 1], self.ntype[i - 1]] for i in sorted(self.alive)}
        return StoreRef(nodes, {k: a[:3] for k, a in self.arcs.items()}, {k: a[3] for k, a in self.arcs.items()})

    def live_tasks(self) -> list:
        return sorted(self.job)

    def of_type(self, ty) -> list:
        return sorted(i for i in self.alive if self.ntype[i - 1] == ty and (ty != OTHER or i in self.parent))

    def children(self, v) -> list:
        return sorted(c for c, p in self.parent.items() if p == v)

    def subtree(self, v) -> list:
        out = [v]
        for c in self.children(v):
            out += self.subtree(c)
        return out

    def load(self) -> dict:
        n: dict = {}
        for p in self.bindings.values():
            n[p] = n.get(p, 0) + 1
        return n

    def blocked(self, v, load=None) -> bool:
        """No arc leads into v under the mode's capacity rule: a PU as full as the caller knows it
        to be (pinned: slots − running), a node above whose children are all blocked."""
        load = self.load() if load is None else load
        if v in self.slots:
            return not self.preemptive and load.get(v, 0) >= self.slots[v]
        return all(self.blocked(c, load) for c in self.children(v))

    def topology(self) -> dict:
        """The caller's own resource tree as an arc table (any positive capacity)."""
        return {(p, c): (0, 1, self.tree_cost.get(c, 0), 0) for c, p in self.parent.items()}

    # ------------------------------------------------- the cost model that moves ---
    def add_class(self, job, c):
        self.cls[job] = c
        self.classes.append(c)
        self.pref[c] = []

    def limited(self, c) -> bool:
        """A per-job, per-machine limit of one task: the classes with an odd index."""
        return self.classes.index(c) % 2 == 1

    def draw_class_set(self, c) -> list:
        ms = self.of_type(MACHINE)
        self.pref[c] = sorted(int(x) for x in self.rng.choice(ms, min(3, len(ms)), replace=False)) if ms else []
        return self.pref[c]

    def bound_beneath(self, v, load=None) -> int:
        load = self.load() if load is None else load
        return sum(load.get(p, 0) for p in self.subtree(v) if p in self.slots)

    def room(self, v, load=None) -> int:
        """What the capacity rule gives an arc into v: the slots beneath it, minus the bound tasks in pinned mode."""
        load = self.load() if load is None else load
        return sum(self.slots[p] - (0 if self.preemptive else load.get(p, 0)) for p in self.subtree(v) if p in self.slots)

    def class_list(self, c, machines, load=None) -> list:
        """(machine, cost, cap) of the class's arcs; a base cost is drawn when a pair is first priced."""
        load = self.load() if load is None else load
        out = []
        for x in machines:
            if (c, x) not in self.base:
                self.base[(c, x)] = int(self.rng.integers(1, 50))
            room = self.room(x, load)
            out.append((x, self.base[(c, x)] + SPREAD * self.bound_beneath(x, load), min(room, 1) if self.limited(c) else room))
        return out

    def resource_lists(self, was_blocked=(), resized=None) -> tuple:
        """→ (tails, lists) of X, the racks, the machines and the PUs: every arc the caller knows
        the store to hold, re-costed with KS_CAP_KEEP (the edge's cost + the tasks bound beneath
        the head; machine → PU and PU → sink move at every second task only); X → a rack with no
        slot beneath it with capacity 0; the arcs into was_blocked (a full PU that gained a slot,
        and its ancestors that were blocked with it) with an explicit capacity; the resized PU's
        arc into the sink with its new slot count."""
        load = self.load()
        tails, lists = [], []
        for u in [self.wildcard] + self.of_type(OTHER) + self.of_type(MACHINE):
            lst = []
            for v in self.children(u):
                n = self.bound_beneath(v, load)
                cost = self.tree_cost.get(v, 0) + (n // 2 if v in self.slots else n)
                if not any(p in self.slots for p in self.subtree(v)):
                    lst.append((v, cost, 0))
                elif v in was_blocked:
                    lst.append((v, cost, 1))
                elif not self.blocked(v, load):
                    lst.append((v, cost, CAP_KEEP))
            tails.append(u)
            lists.append(lst)
        for p in sorted(self.slots):
            tails.append(p)
            lists.append([(self.sink, SINK_COST + load.get(p, 0) // 2, self.slots[p] if p == resized else CAP_KEEP)])
        return tails, lists

    def set_slots(self, p, n):
        self.count["slots_raised" if n > self.slots[p] else "slots_lowered"] += 1
        self.slots[p] = n

    def full_list(self, t, with_agg: bool) -> list:
        out = list(self.prefs[t])
        if self.cls:
            out.append((self.cls[self.job[t]], CLASS_COST))
        if self.wildcard:
            out.append((self.wildcard, WILDCARD))
        if with_agg:
            out.append((self.job[t], UNSCHED))
        return out

    # ---------------------------------------------------------------- bookkeeping ---
    def record(self, call: str, **args):
        self.log.append(dict(round=self.round, call=call, **args))

    def dump(self, path) -> str:
        with open(path, "w") as f:
            json.dump(dict(seed=self.seed, preemptive=self.preemptive, calls=self.log), f, default=_plain)
        return str(path)

    def alloc(self) -> int:
        """The caller owns id reuse (flowgraph/graph.go:169-182): a freed id first, the lowest; else the next."""
        if self.free:
            return self.free.pop(0)
        self.top += 1
        return self.top

    def _kill(self, ids):
        for i in ids:
            self.alive.discard(i)
            self.ntype[i - 1], self.supply[i - 1] = 0, 0
            bisect.insort(self.free, i)

    def _adopt(self, ref):
        self.arcs, self.ntype, self.supply, self.alive = dict(ref.arcs), list(ref.ntype), list(ref.supply), set(ref.alive)
        self.top = max(self.top, len(self.ntype))

    # ------------------------------------------------------------------ the solve ---
    def check_solution(self, cost, flow, flows: dict, mapping: dict) -> list:
        """Checks (a) and (b) of a backend's solve against the MODEL's graph; → the deltas the
        commit must write (c)."""
        g = self.balanced()
        self.record("solve", cost=cost, flow=flow, mapping=sorted(mapping.items()), flows=sorted(flows.items()))
        st, ocost, oflow, _ = ko.cost_scaling(g)
        assert st == 0 and (cost, flow) == (ocost, oflow), ("cost/flow", (cost, flow), (st, ocost, oflow))
        assert flow == len(self.job), "every live task routes its unit"
        got = dict(flows)
        vec = np.asarray([got.pop((int(s), int(d)), 0) for s, d in zip(g.src, g.dst)], np.int64)
        assert not got, ("flow on arcs the model does not hold", got)
        vst, vcost, _ = ko.verify(g, vec)
        assert (vst, vcost) == (0, ocost), ("the oracle's verifier on the model's graph", vst, vcost, ocost)
        on: dict = {}
        for t, p in mapping.items():                       # check_mapping, on the model's types
            assert t in self.job and p in self.slots, ("mapping of a non-task or to a non-PU", t, p)
            on[p] = on.get(p, 0) + 1
        for p in self.slots:                               # (b)
            assert on.get(p, 0) == flows.get((p, self.sink), 0), ("tasks mapped to PU vs its flow into the sink", p)
            assert on.get(p, 0) <= self.slots[p]
        return sched_ref.scheduling_deltas(self.bindings, mapping, self.live_tasks())

    # ------------------------------------------------------------------ the calls ---
    def commit(self, deltas):
        deltas = [tuple(int(v) for v in d) for d in deltas]
        g, before = self.graph(), self.arcs
        args = dict(continuation=self.cont, preemption=PREEMPTION, aggs=list(self.aggs), deltas=deltas)
        if self.preemptive:
            arcs, bind, st = preempt_reference(g, deltas, self.bindings, self.cont, PREEMPTION, True, self.aggs)
        else:
            assert all(k == PLACE for k, _, _ in deltas), "a pinned task moved"
            placed = {t: p for _, t, p in deltas}
            arcs = commit_reference(g, placed, self.cont, True, self.aggs)
            bind = sched_ref.apply_deltas(self.bindings, deltas)
            changed = lambda k: arcs.get(k) != before[k]
            st = dict(placed=len(placed),
                      arcs_removed=sum(1 for (s, d) in before if s in placed and d != placed[s]),
                      running_added=sum(1 for t, p in placed.items() if (t, p) not in before),
                      running_converted=sum(1 for t, p in placed.items() if (t, p) in before),
                      unsched_updates=sum(1 for k in before if k[0] in self.aggs and k[1] == self.sink and changed(k)),
                      cap_updates=sum(1 for k in before if self.ntype[k[0] - 1] != TASK and k[1] != self.sink and changed(k)))
            st["records"] = sum(v for k, v in st.items() if k != "placed")
        self.commit_dropped |= {k for k in before if k[0] in self.pref and k not in arcs}
        self.caps_from = "rule"
        self.arcs, self.bindings = arcs, {t: p for t, p in bind.items() if p}
        self.count["migrations"] += sum(1 for k, _, _ in deltas if k == MIGRATE)
        self.count["preemptions"] += sum(1 for k, _, _ in deltas if k == PREEMPT)
        self.returning += [t for k, t, _ in deltas if k == PREEMPT]
        self.record("commit", **args)
        return args, dict(deltas=deltas, stats=st)

    def remove(self, roots):
        """In pinned mode a full PU has no arc from its machine and a full machine none from its
        rack: such nodes of the subtree are named as roots too, from the caller's own knowledge."""
        load = self.load()
        tree = sorted({v for r in roots for v in self.subtree(r)})
        named = list(roots) + [v for v in tree if v not in roots and self.blocked(v, load)]
        ref = remove_reference(self.graph(), named, self.bindings, True, self.preemptive, alive=self.alive)
        assert ref.removed == tree, ("the rule's subtree is the caller's", ref.removed, tree)
        self.arcs, self.bindings = dict(ref.arcs), dict(ref.bindings)
        self.caps_from = "rule"
        self.pref = {c: [x for x in ms if x not in tree] for c, ms in self.pref.items()}   # the caller's own knowledge
        self.freed_pus |= {v for v in tree if v in self.slots}
        for v in tree:
            self.parent.pop(v, None)
            self.slots.pop(v, None)
            self.tree_cost.pop(v, None)
        self._kill(tree)
        gone = set(tree)
        self.prefs = {t: [(d, c) for d, c in p if d not in gone] for t, p in self.prefs.items()}
        self.returning += [t for t, _ in ref.evicted]
        self.count["evictions"] += len(ref.evicted)
        self.record("remove", roots=named)
        return dict(roots=named), dict(removed=ref.removed, evicted=[(PREEMPT, t, p) for t, p in ref.evicted], stats=ref.stats)

    def complete_recipe(self, tasks):
        """Pinned mode, tasks that ran on full PUs: the bindings to ask for and the ADD_ARC upserts
        of those PUs' parent chains; → (bindings args and expectation, the upserts) or None."""
        if self.preemptive:
            return None
        load = self.load()
        pus = sorted({self.bindings[t] for t in tasks if t in self.bindings and self.blocked(self.bindings[t], load)})
        if not pus:
            return None
        want = [self.bindings.get(t, 0) for t in tasks]
        topo = self.topology()
        ups = chain_upserts(topo, parent_chains(self.ntype, topo, pus))
        for x in ups:
            self.arcs[(int(x["src"]), int(x["dst"]))] = (int(x["low"]), int(x["cap"]), int(x["cost"]), int(x["type"]))
        self.record("get_bindings", tasks=list(tasks))
        self.count["recipe_upserts"] += len(ups)
        self.record("apply_deltas", upserts=[(int(x["src"]), int(x["dst"]), int(x["cap"])) for x in ups])
        return dict(tasks=list(tasks), pu=want), ups

    def complete(self, tasks):
        caps = not self.preemptive        # under the preemptive rule a completion moves no capacity: the flag stays off
        ref = complete_reference(self.graph(), tasks, self.bindings, caps, False, self.aggs, alive=self.alive)
        self.freed_bound |= {t for t in ref.removed if t in self.bindings}
        self.arcs, self.bindings = dict(ref.arcs), dict(ref.bindings)
        self.caps_from = "rule" if caps else self.caps_from
        for t in ref.removed:
            del self.job[t], self.prefs[t]
        self.returning = [t for t in self.returning if t in self.job]
        self._kill(ref.removed)
        self.record("complete", tasks=list(tasks), caps=caps)
        return dict(tasks=list(tasks), caps=caps, aggs=list(self.aggs)), dict(left=ref.left, stats=ref.stats)

    def grow(self, nodes, edges):
        """nodes (id, type, slots, sink_cost); edges (parent, child, cost, kind) of the new subtree.
        The chains from the attach points up to the root come from the caller's tree."""
        new = {n[0] for n in nodes}
        edges = list(edges)
        for p in sorted({e[0] for e in edges if e[0] not in new}):
            costs = {(q, c): self.tree_cost.get(c, 0) for c, q in self.parent.items()}
            edges += [e for e in chain(self.parent, p, costs) if e not in edges]
        ref = grow_reference(self.graph(), nodes, edges, alive=self.alive)
        held = sum(1 for p, c, _, _ in edges if c not in new and ref.S.get(c, 0) and (p, c) not in self.arcs)
        self.count["ancestor_recreated"] += held
        self.count["pu_id_reused"] += sum(1 for i, ty, _, _ in nodes if ty == PU and i in self.freed_pus)
        self._adopt(ref)
        for i, ty, s, _ in nodes:
            if ty == PU:
                self.slots[i] = s
        for p, c, co, kind in edges:
            if kind == TREE and c in new:
                self.parent[c], self.tree_cost[c] = p, co
        self.record("grow", nodes=list(nodes), edges=edges)
        return dict(nodes=list(nodes), edges=edges), dict(stats=ref.stats)

    def refresh_caps(self):
        """ks_complete_tasks(k = 0, KS_COMPLETE_RESOURCE_CAPS[ | _PREEMPTIVE]): the plain refresh."""
        ref = complete_reference(self.graph(), [], self.bindings, True, self.preemptive, self.aggs, alive=self.alive)
        self.arcs = dict(ref.arcs)
        self.caps_from = "rule"
        self.count["stale_caps_repaired"] += ref.stats["cap_updates"]
        self.record("refresh_caps")
        return dict(preemptive=self.preemptive, aggs=list(self.aggs)), dict(left=[], stats=ref.stats)

    def arrive(self, tasks, jobs, prefs, lists=None):
        for t, a, p in zip(tasks, jobs, prefs):
            self.job[t], self.prefs[t] = a, list(p)
        lists = [self.full_list(t, True) for t in tasks] if lists is None else lists
        self._held_before = {a for a in self.aggs if (a, self.sink) in self.arcs}
        ref = arrive_reference(self.graph(), tasks, lists, self.aggs, SINK_COST, alive=self.alive)
        self.count["bound_id_reused"] += sum(1 for t in tasks if t in self.freed_bound)
        self.count["superseded"] += ref.superseded
        self.freed_bound -= set(tasks)
        self._adopt(ref)
        self._note_sink_arcs(ref.stats["unsched_added"])
        self.record("arrive", tasks=list(tasks), lists=lists)
        return dict(tasks=list(tasks), lists=lists, aggs=list(self.aggs)), dict(stats=ref.stats, superseded=ref.superseded)

    def _note_sink_arcs(self, added: int):
        """Of the aggregator → sink arcs a call added, those the graph held earlier in the run."""
        now = {a for a in self.aggs if (a, self.sink) in self.arcs}
        fresh = now - self._held_before
        assert len(fresh) == added
        self.count["aggregator_recreated"] += len(fresh & self.had_sink_arc)
        self.had_sink_arc |= now

    def refresh(self, tasks, lists):
        self._held_before = {a for a in self.aggs if (a, self.sink) in self.arcs}
        table = dict(sorted(self.arcs.items()))           # any fixed order: the record order is not compared
        ref = refresh_reference(self.ntype, table, tasks, lists, self.bindings, self.aggs, SINK_COST, 0, alive=self.alive)
        self.arcs = dict(ref.arcs)
        self._note_sink_arcs(ref.stats["unsched_added"])
        self.count["running_kept"] += ref.stats["running_kept"]
        self.returning = [t for t in self.returning if t not in tasks]
        self.record("refresh", tasks=list(tasks), lists=lists)
        return dict(tasks=list(tasks), lists=lists, aggs=list(self.aggs)), dict(stats=ref.stats)

    def nodes(self, tails, lists):
        """ks_update_nodes with the classes' and the resources' lists. A refusal of the rule
        (InvalidNodes, BelowLowerBound) leaves the model as it was."""
        table = dict(sorted(self.arcs.items()))           # any fixed order: the record order is not compared
        ref = nodes_reference(self.ntype, table, tails, lists, 0, alive=self.alive)
        n, before, down = self.count, self.arcs, set()
        for u, lst in zip(tails, lists):
            named = {d for d, _, _ in lst}
            if u not in self.pref:
                n["resource_recosted"] += sum(1 for d, c, _ in lst if (u, d) in before and before[(u, d)][2] != c)
                n["resource_unchanged"] += sum(1 for d, c, cap in lst if cap == CAP_KEEP and (u, d) in before and before[(u, d)][2] == c)
                n["chain_relisted"] += sum(1 for d, _, cap in lst if d != self.sink and cap not in (0, CAP_KEEP) and (u, d) not in before)
                continue
            if sum(1 for k in before if u in k) > 64:     # its residual segment holds its out-arcs and its in-arcs: more than one chunk
                n["class_tail_over_64"] += 1
            n["class_arcs_removed"] += sum(1 for (s, d) in before if s == u and d not in named and d != self.sink)
            for d, _, cap in lst:
                if (u, d) not in before:
                    n["class_arcs_added"] += cap > 0
                    n["class_arc_recreated"] += cap > 0 and (u, d) in self.commit_dropped
                else:
                    n["class_arcs_zeroed"] += cap == 0
                    n["cap_overwritten"] += 0 < cap < before[(u, d)][1] and (u, d) in self.held_down
                if self.limited(u) and 0 < cap < self.room(d):
                    down.add((u, d))
        self.commit_dropped -= {(u, d) for u, lst in zip(tails, lists) for d, _, cap in lst if cap}
        self.held_down = down
        self.arcs = dict(ref.arcs)
        self.caps_from = "model"
        self.record("nodes", tails=list(tails), lists=lists)
        return dict(tails=list(tails), lists=lists), dict(stats=ref.stats)

    def age(self, mode, cost, continuation=None):
        self.cont = self.cont if continuation is None else continuation
        self.arcs, changed = unsched_costs_reference(self.ntype, self.arcs, self.aggs, mode, cost, self.cont)
        self.record("age", mode=mode, cost=cost, continuation=self.cont)
        return dict(mode=mode, cost=cost, continuation=self.cont, aggs=list(self.aggs)), dict(changed=changed)

    # ----------------------------------------------------------------- invariants ---
    def check_invariants(self, caps=True, feasible=True):
        for (s, d) in self.arcs:
            assert s in self.alive and d in self.alive, ("a dangling arc", s, d)
        into: dict = {}
        for (s, d) in self.arcs:
            if s in self.job and d in self.aggs:
                into[d] = into.get(d, 0) + 1
        for a in self.aggs:
            arc = self.arcs.get((a, self.sink))
            assert (arc is None) == (into.get(a, 0) == 0) and (arc is None or arc[1] == into[a]), ("aggregator", a, arc, into.get(a))
        if caps:
            ref = complete_reference(self.graph(), [], self.bindings, True, self.preemptive, self.aggs, alive=self.alive)
            if not self.classes or self.caps_from == "rule":
                assert ref.stats["records"] == 0, ("resource capacities are not the rule's", ref.stream)
            else:                                          # ks_update_nodes wrote last: the cap-1 classes' arcs are the cost model's
                odd = {c for c in self.classes if self.limited(c)}
                assert all(int(x["src"]) in odd for x in ref.stream), ("resource capacities are not the rule's", ref.stream)
                load = self.load()
                for (s, d), a in self.arcs.items():
                    assert s not in odd or d == self.sink or a[1] == min(self.room(d, load), 1), ("a cap-1 arc", s, d, a)
        if caps:                                           # no free slot is cut off: the tree's arc leads into every head with room
            load = self.load()
            for v, p in self.parent.items():
                assert self.blocked(v, load) or (p, v) in self.arcs, ("no arc into a resource with room", p, v)
        for (s, d) in self.arcs:                           # (no class: nothing to look at)
            if s in self.pref:
                assert self.ntype[d - 1] == MACHINE and d in self.pref[s], ("a class arc outside the class's set", s, d)
        for t, p in self.bindings.items():
            assert t in self.job and p in self.slots and self.arcs[(t, p)][3] == 1, ("binding", t, p)
        for (s, d), a in self.arcs.items():
            assert a[3] != 1 or self.bindings.get(s) == d, ("a running arc without its binding", s, d)
        if feasible:
            st, _, flow, _ = ko.cost_scaling(self.balanced())
            assert st == 0 and flow == len(self.job), ("the next solve is infeasible", st, flow)


def _plain(x):
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, np.ndarray):
        return x.tolist()
    raise TypeError(type(x))


# ------------------------------------------------------------------------ backends ---
class OracleBackend:
    """No device: the oracle solves (successive shortest paths; the model checks it against
    cost scaling) and every other call is answered by the rule itself."""

    def solve(self, model):
        g = model.balanced()
        st, cost, flow, vec, _ = ko.ssp(g)
        assert st == 0
        flows = {(int(s), int(d)): int(f) for s, d, f in zip(g.src, g.dst, vec) if f}
        return cost, flow, flows, ko.bfs_mapping(g, vec)

    def idle(self, model, mapping):
        pass

    def between(self, model, rnd):
        pass

    def call(self, model, name, args, expect):
        pass


class ReplayBackend(OracleBackend):
    """The solves of a call log (RoundModel.dump), in order: a round that failed on a device is
    replayed on the host with the optimum the device chose."""

    def __init__(self, log: dict):
        self.solves = [x for x in log["calls"] if x["call"] == "solve"]

    def solve(self, model):
        x = self.solves.pop(0)
        return x["cost"], x["flow"], {(s, d): f for (s, d), f in x["flows"]}, {t: p for t, p in x["mapping"]}


# -------------------------------------------------------------------- the events ---
class Script:
    """The seeded event generator and the scripted events of a run. It draws from the model's
    rng over the model's sorted state only."""

    def __init__(self, model, rounds, arrivals=(2, 5), completions=(1, 3), burst=None, grow_rack=None, hub=None,
                 classes=False, wide=None):
        self.m, self.rounds, self.arrivals, self.completions = model, rounds, arrivals, completions
        self.burst, self.grow_rack, self.hub = burst, grow_rack, hub
        self.classes, self.wide = classes, wide   # wide: the class that prefers every machine of the growing rack ("round 4": that round's new job's)
        self.fresh: list = []                 # (job, class) of the jobs ks_add_resources brought in this round
        self.resized = False                  # a PU's slot count changed in this round's ks_update_nodes
        self.frozen: set = set()              # tasks a scripted event still needs
        self.guard: set = set()               # resources a scripted event still needs
        self.drain = None                     # the job drained for the re-created aggregator
        self.lone = self.occupant = self.migrant = self.emptied = None
        self.feasible = True                  # solve for feasibility after every call (the small shapes)

    # every step: → the arguments of the model's call, or None for no call this round
    def removal(self, rnd):
        m, rng = self.m, self.m.rng
        machines = [x for x in m.of_type(MACHINE) if x not in self.guard]
        if rnd == 1 and machines:             # the machine holding the most bound tasks: evictions
            load = m.load()
            held = lambda x: sum(load.get(p, 0) for p in m.children(x))
            return [max(machines, key=lambda x: (held(x), -x))]
        racks = [r for r in m.of_type(OTHER) if not (set(m.subtree(r)) & self.guard)]
        if rnd == 5 and len(racks) > 1:
            return [int(rng.choice(racks))]
        if rnd == 8:                          # every machine of one rack: the rack stays, with no slot beneath it
            left = {r: m.children(r) for r in racks}
            self.emptied = min(left, key=lambda r: (len(left[r]), r)) if left else None
            if self.emptied and left[self.emptied]:         # (a rack that earlier removals emptied serves as well)
                return left[self.emptied]
        if len(machines) > 3 and rng.random() < 0.3:
            return sorted(int(x) for x in rng.choice(machines, int(rng.integers(1, 3)), replace=False))
        return None

    def completion(self, rnd):
        m, rng = self.m, self.m.rng
        free = [t for t in m.live_tasks() if t not in self.frozen]
        if self.burst and rnd == self.burst[0]:
            return free[:self.burst[1]]
        if rnd == 3:                          # drain the smallest job of every task that holds its aggregator arc
            sizes = {a: sum(1 for t in free if m.job[t] == a) for a in m.aggs if not any(m.job[t] == a for t in self.frozen)}
            self.drain = min(sizes, key=lambda a: (sizes[a], a))
            out = [t for t in free if m.job[t] == self.drain and (m.preemptive or t not in m.bindings)]
            if out:
                return out
        bound = [t for t in free if t in m.bindings]
        waiting = [t for t in free if t not in m.bindings]
        lo, hi = self.completions
        kb, kw = min(len(bound), int(rng.integers(lo, hi + 1))), min(max(len(waiting) - 1, 0), int(rng.integers(lo, hi + 1)))
        out = ([] if not kb else rng.choice(bound, kb, replace=False).tolist()) + \
              ([] if not kw else rng.choice(waiting, kw, replace=False).tolist())
        return sorted(int(t) for t in out) or None

    def growth(self, rnd):
        """→ (nodes, edges, new jobs' aggregator ids)."""
        m, rng = self.m, self.m.rng
        nodes, edges, jobs = [], [], []

        def machine(rack, pus, slots, reuse=False):
            was_pu = [i for i in m.free if i in m.freed_pus] if reuse else []
            if was_pu:                        # scripted: a removed PU's id for the new PU, whatever else is free
                m.free.remove(was_pu[0])
            mid = m.alloc()
            nodes.append((mid, MACHINE, 0, 0))
            edges.append((rack, mid, TREE_COST[MACHINE], TREE))
            for k in range(pus):
                p = was_pu[0] if was_pu and k == 0 else m.alloc()
                nodes.append((p, PU, slots, SINK_COST))
                edges.append((mid, p, TREE_COST[PU], TREE))
            return mid
        racks = m.of_type(OTHER)
        if self.grow_rack and rnd in self.grow_rack[0]:    # one rack gains machines until its segment overflows
            for _ in range(self.grow_rack[1]):
                machine(racks[0], 1, 2)
        if rnd == 1:                        # right after the scripted removal: its ids come back, the PU's for a PU
            machine(racks[0], 1, 2, reuse=True)
        elif rnd == 2:                        # a PU beneath a machine that is full: the pinned rule dropped the arcs above it
            ms = m.of_type(MACHINE)
            full = [x for x in ms if m.blocked(x)] or ms
            p = m.alloc()
            nodes.append((p, PU, 1, SINK_COST))
            edges.append((full[0], p, TREE_COST[PU], TREE))
        elif rnd == 4:                        # a new rack with two machines
            r = m.alloc()
            nodes.append((r, OTHER, 0, 0))
            edges.append((m.wildcard, r, TREE_COST[OTHER], TREE))
            machine(r, 1, 2)
            machine(r, 2, 1)
        elif rnd == 9 and self.emptied in m.alive:         # … and gains a machine: the arc into it had kept its capacity
            machine(self.emptied, 1, 2)
        elif racks and rng.random() < 0.4:
            machine(int(rng.choice(racks)), int(rng.integers(1, 3)), int(rng.integers(1, 3)))
        if m.preemptive and rnd == 5 and not self.hub:     # the one-slot PU of the scripted PREEMPT
            self.lone = machine(racks[0], 1, 1)
            self.guard |= {self.lone, racks[0]}
        if rnd in (0, 4):                     # a new job: its aggregator has no arc into the sink yet
            a = m.alloc()
            nodes.append((a, OTHER, 0, 0))
            jobs.append(a)
            if self.classes:                  # … and its class no arc at all: ks_add_tasks and ks_update_nodes give it them
                c = m.alloc()
                nodes.append((c, OTHER, 0, 0))
                self.fresh.append((a, c))
                if self.wide == "round 4" and rnd == 4:
                    self.wide = c
        return nodes, edges, jobs

    def draw_prefs(self):
        m, rng = self.m, self.m.rng
        ms = m.of_type(MACHINE)
        k = min(2, len(ms))
        return [(int(x), int(c)) for x, c in zip(rng.choice(ms, k, replace=False), rng.integers(1, 100, k))] if k else []

    def arrival(self, rnd):
        """→ (tasks, jobs, prefs, lists or None)."""
        m, rng = self.m, self.m.rng
        lo, hi = self.arrivals
        k = self.burst[1] if self.burst and rnd == self.burst[0] else int(rng.integers(lo, hi + 1))
        tasks = [m.alloc() for _ in range(k)]
        jobs = [int(rng.choice(m.aggs)) for _ in tasks]
        if self.hub:
            jobs = [self.hub] * k
        prefs = [self.draw_prefs() for _ in tasks]
        for a in m.aggs:                      # a new or a drained job gets a task at once
            if (a, m.sink) not in m.arcs and a not in jobs:
                tasks.append(m.alloc())
                jobs.append(a)
                prefs.append(self.draw_prefs())
        lists = None
        if m.preemptive and rnd == 5 and self.lone:        # the occupant-to-be of the lone PU: nothing else is as cheap
            t = m.alloc()
            tasks.append(t)
            jobs.append(m.aggs[0])
            prefs.append([(self.lone, LURE)])
            self.occupant = t
            self.frozen.add(t)
        if m.preemptive and rnd == 6 and self.occupant:    # the task that takes the occupant's slot
            t = m.alloc()
            tasks.append(t)
            jobs.append(m.aggs[0])
            prefs.append([(self.lone, LURE)])
            self.frozen.add(t)
        if rnd == 2 and tasks and prefs[0]:   # a head listed twice for one task: the later record stands
            for t, a, p in zip(tasks, jobs, prefs):
                m.job[t], m.prefs[t] = a, list(p)
            lists = [m.full_list(t, True) for t in tasks]
            d, c = prefs[0][0]
            lists[0] = [(d, c + 7)] + lists[0]
        return tasks, jobs, prefs, lists

    def update(self, rnd):
        """→ (tasks, lists): the returning tasks with their aggregator arc, a share of the others
        with new preferences (pinned: waiting tasks only; a pinned task keeps its one arc)."""
        m, rng = self.m, self.m.rng
        tasks, lists = [], []
        for t in sorted(set(m.returning)):
            if t not in self.frozen or t == self.occupant:
                m.prefs[t] = self.draw_prefs() if t != self.occupant else [(self.lone, 1)]
            tasks.append(t)
            lists.append(m.full_list(t, True))
        if m.preemptive and rnd == 6 and self.occupant in m.bindings and self.occupant not in tasks:
            m.prefs[self.occupant] = [(self.lone, 1)]          # its lure goes: it stays only while nobody pays more
            tasks.append(self.occupant)
            lists.append(m.full_list(self.occupant, False))
        if m.preemptive and rnd == 7:         # a running task gets a much cheaper arc into another machine: MIGRATE
            here = lambda t: m.parent[m.bindings[t]]
            ms = [x for x in m.of_type(MACHINE) if x != self.lone]
            cand = [t for t in sorted(m.bindings) if t not in self.frozen and t not in tasks and any(x != here(t) for x in ms)]
            if cand:
                t = cand[0]
                m.prefs[t] = [(next(x for x in ms if x != here(t)), LURE)]
                tasks.append(t)
                lists.append(m.full_list(t, False))
                self.migrant = t
                self.frozen.add(t)
        elif self.migrant in m.job and rnd == 8:               # its lure goes again
            if self.migrant not in tasks:
                m.prefs[self.migrant] = self.draw_prefs()
                tasks.append(self.migrant)
                lists.append(m.full_list(self.migrant, False))
            self.frozen.discard(self.migrant)
        pool = [t for t in m.live_tasks() if t not in self.frozen and t not in tasks and (m.preemptive or t not in m.bindings)]
        if self.hub:
            pool = pool[:64]
        for t in pool:
            if rng.random() < 0.25:
                m.prefs[t] = self.draw_prefs()
                lst = m.full_list(t, False)
                if t in m.bindings and rng.random() < 0.5:
                    lst.append((m.bindings[t], 0))             # its own PU: the running arc is kept
                tasks.append(t)
                lists.append(lst)
        return (tasks, lists) if tasks else None

    def node_lists(self, rnd):
        """→ (tails, lists) of this round's ks_update_nodes, or None without the option: a slot
        change in rounds 2 and 6, every class's set with one machine gone and one other in it, the
        classes' and the resources' arcs as the cost model prices them now."""
        self.resized = False
        if not self.classes:
            return None
        m, rng = self.m, self.m.rng
        load = m.load()
        was_blocked, resized = set(), None
        free = [p for p in sorted(m.slots) if m.parent[p] not in self.guard]
        if rnd == 6:                          # a PU with a bound task gains a slot (pinned: a full one first)
            cand = sorted((p for p in free if load.get(p, 0)), key=lambda p: (load[p] < m.slots[p], p))
            if cand:
                v = resized = cand[0]
                while v in m.parent and m.blocked(v, load):    # the arcs into these went with the pinned rule
                    was_blocked.add(v)
                    v = m.parent[v]
                m.set_slots(resized, m.slots[resized] + 1)
        if rnd == 2:                          # a PU with room loses a slot, never below its bound tasks
            down = lambda p: load[p] if not m.preemptive and load.get(p, 0) else m.slots[p] - 1
            held = lambda p: any(m.parent[p] in s for s in m.pref.values())     # listed last round, with room: a class holds the arc
            cand = sorted((p for p in free if m.slots[p] - 1 >= max(load.get(p, 0), 1)),
                          key=lambda p: (down(p) != load.get(p, 0), len(m.children(m.parent[p])), not held(p), p))
            if cand:                          # pinned: down to exactly that count, the only PU of a machine a class prefers first:
                resized = cand[0]             # the PU is full, and the class arc into its machine is listed with capacity 0
                m.set_slots(resized, down(resized))
        self.resized = resized is not None
        ms = m.of_type(MACHINE)
        tails, lists = [], []
        for c in m.classes:
            mine = list(m.pref[c])
            if c == self.wide:                # every machine of the growing rack but one, another one each round
                mine = m.children(m.of_type(OTHER)[0]) if m.of_type(OTHER) else []
                mine = [x for k, x in enumerate(mine) if len(mine) <= 3 or k != rnd % len(mine)]
            elif not mine:                    # a new class (or one whose machines all left)
                mine = m.draw_class_set(c)
            else:                             # one leaves, one other joins; then up to three again after removals
                others = [x for x in ms if x not in mine]
                if others:                    # (the machine of a PU resized in this call stays: its arc is re-sized, not dropped)
                    mine.remove(int(rng.choice([x for x in mine if resized is None or x != m.parent[resized]] or mine)))
                    mine.append(int(rng.choice(others)))
                while len(mine) < 3 and len(mine) < len(ms):
                    mine.append(int(rng.choice([x for x in ms if x not in mine])))
            m.pref[c] = sorted(mine)
            tails.append(c)
            lists.append(m.class_list(c, m.pref[c], load))
        rt, rl = m.resource_lists(was_blocked, resized)
        return tails + rt, lists + rl

    def ageing(self, rnd):
        if rnd == 7:                          # once per run: a SET, with a raised continuation cost
            return COST_SET, UNSCHED + 50, RAISED_CONTINUATION
        return COST_ADD, AGE, None


def run_round(model, script, dev, rnd):
    """One round of INTEGRATION §2.1 against a backend; the invariants after every call."""
    m = model
    m.round = rnd

    def step(name, res, caps=True):
        args, expect = res
        dev.call(m, name, args, expect)
        # a task evicted after a pinned commit has no arc until ks_update_tasks brings it back in this round
        m.check_invariants(caps, script.feasible and (m.preemptive or not m.returning))

    cost, flow, flows, mapping = dev.solve(m)
    deltas = m.check_solution(cost, flow, flows, mapping)
    dev.idle(m, mapping)
    step("commit", m.commit(deltas))
    dev.between(m, rnd)
    roots = script.removal(rnd)
    if roots:
        step("remove", m.remove(roots))
    done = script.completion(rnd)
    if done:
        recipe = m.complete_recipe(done)
        if recipe:
            dev.call(m, "get_bindings", recipe[0], dict(pu=recipe[0]["pu"]))
            dev.call(m, "apply_deltas", dict(stream=recipe[1]), {})
            m.check_invariants(caps=False, feasible=False)
        step("complete", m.complete(done))
    nodes, edges, jobs = script.growth(rnd)
    if nodes:
        step("grow", m.grow(nodes, edges), caps=not edges)
        m.aggs = sorted(m.aggs + jobs)
        m.count["new_jobs"] += len(jobs)
        while script.fresh:
            m.add_class(*script.fresh.pop(0))
        if edges:                             # a stale capacity into a rack that had no free slot beneath it was raised, not set
            step("refresh_caps", m.refresh_caps())
    tasks, jobs, prefs, lists = script.arrival(rnd)
    if tasks:
        step("arrive", m.arrive(tasks, jobs, prefs, lists))
    upd = script.update(rnd)
    if upd:
        step("refresh", m.refresh(*upd))
    assert not m.returning, "an evicted task did not come back in its round"
    lists = script.node_lists(rnd)
    if lists:
        step("nodes", m.nodes(*lists), caps=not script.resized)
        if script.resized:                    # UpdateResourceTopology: the new slot count goes up the chain
            step("refresh_caps", m.refresh_caps())
    step("age", m.age(*script.ageing(rnd)))


def run(model, script, dev, rounds, tmp_path=None):
    """rounds rounds and a last solve; a failing assertion names the seed and the round and leaves
    the call log as JSON."""
    try:
        model.check_invariants()
        for rnd in range(rounds):
            run_round(model, script, dev, rnd)
        model.round = rounds
        model.check_solution(*dev.solve(model))
    except Exception as e:                    # (a rule that refuses the model's own call is a failure of the round too)
        where = model.dump(tmp_path / f"round_log_seed{model.seed}.json") if tmp_path is not None else "(no log)"
        raise RoundFailure(f"seed {model.seed}, {'preemptive' if model.preemptive else 'pinned'}, round {model.round}: "
                           f"{e!r}; the call log: {where}") from e
    return model.count


# ------------------------------------------------------- the cases of both suites ---
def small_case(preemptive, seed, rounds, classes=False):
    m = RoundModel.cluster(preemptive, seed, classes=classes, slots=6 if classes else 2)
    return m, Script(m, rounds, classes=classes), rounds


def wave_case(preemptive, classes=False):
    """One job of 150 tasks, 65 arrivals and 65 completions in round 2, one rack that gains 12
    machines in each of rounds 1 to 5. With classes: the 150-task job's class holds more than 64
    arcs (its tasks' and its machines': its segment is walked in chunks), and the class of the job
    that round 4 brings prefers every machine of the growing rack from its first call on: some
    fifty arcs (pinned: the dozen into machines with room) into the segment of a node the store
    has just sized for the one or two tasks pointing at it, whatever the solves chose before."""
    m = RoundModel.cluster(preemptive, 7, job_sizes=(150, 8, 8), classes=classes)
    return m, Script(m, 6, burst=(2, 65), grow_rack=((1, 2, 3, 4, 5), 12), classes=classes, wide="round 4" if classes else None), 6


def hub_case(preemptive):
    """4,200 tasks of one job on 60 slots: the job's aggregator holds more than 4,096 arcs."""
    m = RoundModel.cluster(preemptive, 9, racks=2, mpr=3, pus=2, slots=5, job_sizes=(4200, 8))
    s = Script(m, 4, arrivals=(20, 40), completions=(10, 20), hub=m.aggs[0])
    s.feasible = False                        # (a solve after every call of this size is the GPU suite's time)
    return m, s, 4
