// ks_sched.hip — the scheduler-side sweeps of a ksched round, on the
// device-resident graph (SURVEY §8 row f: the per-round O(T) CPU work that
// remains around Solve once the solve itself is fast):
//
//   scheduling deltas   NodeBindingToSchedulingDelta + SchedulingDeltasForPreemptedTasks
//                       (flowmanager/graph_manager.go:253-295, :297-339): the new
//                       task→PU mapping against the bindings kept per task slot →
//                       PREEMPT / PLACE / MIGRATE records; every destination must be
//                       a PU (:259-262)
//   topology statistics ComputeTopologyStatistics (graph_manager.go:480-511) with the
//                       trivial model's PrepareStats / GatherStats
//                       (costmodel/trivial_cost_modeler.go:147-176): BFS from the
//                       sink over in-arcs, level-synchronous
//   unscheduled costs   UpdateAllCostsToUnscheduledAggs (graph_manager.go:462-475):
//                       every task's arc into its unscheduled aggregator re-costed
//                       in place (residual pair included), running tasks' running
//                       arcs set to the continuation cost
//   commit              the records a host would export for the solve's deltas, generated
//                       in device memory for store_apply (ks_store.hip) by one kernel
//                       family with a mode. Pinned: TaskScheduled → pinTaskToNode
//                       (graph_manager.go:454-460, 675-720), updateUnscheduledAggNode(−1)
//                       (:706) and capacityFromResNodeToParent (:662-667). Preemptive
//                       (Preemption == true): updateArcsForScheduledTask (:855-888),
//                       updateRunningTaskToUnscheduledAggArc (:1164-1181), TaskEvicted
//                       (:412-433), TaskMigrated (:407-410) and
//                       capacityFromResNodeToParent returning NumSlotsBelow
//   remove resources    DeregisterResource (flowscheduler/scheduler.go:162-210): the subtree of
//                       a machine or a rack marked by a chunked level descent over the
//                       residual CSR (traverseAndRemoveTopology, graph_manager.go:829-844),
//                       the tasks bound in it evicted (dfsEvictTasks, scheduler.go:533-566),
//                       its REMOVE_NODE records and, through the commit's capacity pass, the
//                       ancestors' capacity records generated for store_apply
//   complete tasks      HandleTaskCompletion (flowscheduler/scheduler.go:106-132) → TaskCompleted
//                       (graph_manager.go:389-405) → removeTaskNode (:803-813): the ids checked and
//                       claimed in the flag bytes, their bindings read, the aggregators' losses
//                       (updateUnscheduledAggNode(−1), :1291-1305) counted from the tasks' own chunked
//                       segments, the REMOVE_NODE records and, through the commit's capacity pass in
//                       its completing mode, the capacity records generated for store_apply
//   add tasks           AddOrUpdateJobNodes (graph_manager.go:166-208): addTaskNode (:632-648) and the
//                       arcs of updateTaskNode (:1183-1285) as ADD_NODE and ADD_ARC records at fixed
//                       stream positions, every head checked against node liveness and types, and
//                       updateUnscheduledAggNode(+1) (:194, :1291-1305): the gains counted with one
//                       atomic per aggregator per wave, the store's (src, dst) index telling a capacity
//                       rise from an arc to re-create. No residual CSR is read and no BFS runs
//   add resources       AddResourceTopology (graph_manager.go:238-251): addResourceTopologyDFS (:557-630)
//                       as ADD_NODE, PU → sink and resource-arc records at fixed stream positions, every
//                       edge checked against node liveness and types; the new PUs' slots summed up the
//                       parent edges with one atomic per ancestor per wave and step, and
//                       updateResourceStatsUpToRoot (:1041-1061) for the arcs above the attach point, the
//                       store's index again telling a capacity rise from an arc to re-create
//   update tasks        UpdateTimeDependentCosts (graph_manager.go:211-213) → updateTaskNode (:1183-1192)
//                       for tasks that have their node: each task's list of arcs diffed against the
//                       store. A listed arc finds its slot through the (src, dst) index (AddArc, or
//                       ChangeArcCost when the cost differs); the held arcs nobody listed are found in the
//                       task's own chunked segment and deleted (removeInvalid*Arcs, :732-790) unless
//                       running or into an aggregator; an evicted task's unit returns to its aggregator
//                       with one atomic per aggregator per wave
#include "ks_sched.h"
#include "ks_store.h"

namespace ks {
namespace {

constexpr int SB = 256;

inline int grid(long long n) {
    long long b = (n + SB - 1) / SB;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---------------------------------------------------------- scheduling deltas ---
// kind per task slot: 0 none, 1 + pb.SchedulingDelta type (PLACE 0, PREEMPT 1, MIGRATE 2)
__global__ void k_delta_kinds(int ncap, const int* __restrict__ is_task, const int* __restrict__ rank,
                              const unsigned long long* __restrict__ newpu, const unsigned long long* __restrict__ bind,
                              const unsigned char* __restrict__ type, long long nstore, int* __restrict__ pre,
                              int* __restrict__ other, int* __restrict__ bad) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < ncap; v += (long long)gridDim.x * SB) {
        int p = 0, o = 0;
        if (is_task[v]) {
            const unsigned long long nw = newpu[rank[v]], old = bind[v];
            if (nw && ((long long)nw > nstore || type[nw - 1] != KS_NODE_PU)) atomicOr(bad, 1);   // :259-262
            if (nw == 0 && old != 0) p = 1;                // PREEMPT: running, absent from the mapping
            else if (nw != 0 && old == 0) o = 1;           // PLACE
            else if (nw != 0 && old != nw) o = 2;          // MIGRATE
        }
        pre[v] = p;
        other[v] = o;
    }
}

// Records at their scanned positions: preemptions first (the reference emits them
// before the mapping's deltas, flowscheduler/scheduler.go:356-365), then
// placements and migrations, each in task-slot order.
__global__ void k_delta_emit(int ncap, const int* __restrict__ rank, const unsigned long long* __restrict__ newpu,
                             const unsigned long long* __restrict__ bind, const int* __restrict__ pre,
                             const int* __restrict__ pre_pos, const int* __restrict__ other,
                             const int* __restrict__ other_pos, int npre, ks_sched_delta* __restrict__ out,
                             unsigned long long* __restrict__ bind_out, int commit) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < ncap; v += (long long)gridDim.x * SB) {
        if (pre[v]) {
            ks_sched_delta d{KS_DELTA_PREEMPT, 0, (uint64_t)v + 1, bind[v]};
            out[pre_pos[v]] = d;
            if (commit) bind_out[v] = 0;
        } else if (other[v]) {
            const unsigned long long nw = newpu[rank[v]];
            ks_sched_delta d{other[v] == 1 ? KS_DELTA_PLACE : KS_DELTA_MIGRATE, 0, (uint64_t)v + 1, nw};
            out[npre + other_pos[v]] = d;
            if (commit) bind_out[v] = nw;
        }
    }
}

// ------------------------------------------------------- topology statistics ---
// Level-synchronous BFS from the sink over in-arcs. Every node first reached at
// level L + 1 is zeroed (PrepareStats; the arrays start at 0) and pushed; then
// each in-arc source gathers from the node being expanded: a PU from the sink
// takes (len(CurrentRunningTasks), maxTasksPerPu), any other accumulating node
// adds the expanded node's sums (GatherStats). Accumulating nodes: PUs,
// machines, intermediate resources, and type-0 nodes (the coordinator; ECs and
// aggregators only ever see non-resource sources and stay 0).
__device__ __forceinline__ bool accum(unsigned char t) {
    return t == KS_NODE_PU || t == KS_NODE_MACHINE || t == KS_NODE_INTERMEDIATE || t == KS_NODE_OTHER;
}

__global__ void k_topo_level(SchedDev d, const int* __restrict__ front, int nfront, int level, int* __restrict__ lvl,
                             int* __restrict__ next, int* __restrict__ nnext, unsigned long long mtpp,
                             const unsigned long long* __restrict__ pu_slots,
                             const unsigned long long* __restrict__ pu_running, unsigned long long* __restrict__ slots,
                             unsigned long long* __restrict__ running) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    for (int i = wave; i < nfront; i += nwaves) {
        const int x = front[i];                 // internal id
        const int v = d.iperm[x];               // its slot
        const unsigned char tx = d.n_type[v];
        const bool cur_sink = tx == KS_NODE_SINK;
        const bool cur_res = accum(tx);
        for (int p = d.first[x] + lane; p < d.first[x + 1]; p += 64) {
            const int e = d.ent[p];
            if (e < 0 || !(e & 1)) continue;    // live in-arcs only (reverse positions)
            const int u = d.pos[p].head;
            const int us = d.iperm[u];
            if (atomicCAS(&lvl[u], -1, level + 1) == -1) next[atomicAdd(nnext, 1)] = u;
            const unsigned char tu = d.n_type[us];
            if (!accum(tu)) continue;
            if (cur_sink) {
                if (tu == KS_NODE_PU) {
                    running[us] = pu_running[us];
                    slots[us] = pu_slots ? pu_slots[us] : mtpp;
                }
            } else if (cur_res) {
                atomicAdd(&running[us], running[v]);
                atomicAdd(&slots[us], slots[v]);
            }
        }
    }
}

// running arcs (type 1) into each PU slot: len(CurrentRunningTasks) by default
__global__ void k_running_into(int hi, const unsigned char* __restrict__ alive, const unsigned char* __restrict__ atype,
                               const int* __restrict__ dst, unsigned long long* __restrict__ cnt) {
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < hi; s += (long long)gridDim.x * SB)
        if (alive[s] && atype[s] == 1) atomicAdd(&cnt[dst[s]], 1ULL);
}

__global__ void k_scatter_running(int k, const unsigned long long* __restrict__ ids,
                                  const unsigned long long* __restrict__ vals, unsigned long long* __restrict__ cnt) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < k; i += (long long)gridDim.x * SB)
        cnt[ids[i] - 1] = vals[i];
}

// ----------------------------------------------------- unscheduled-arc costs ---
// flag bits per node slot: 1 unscheduled aggregator, 2 task with a running arc
// (type 1), 4 task with an arc into an unscheduled aggregator
__global__ void k_mark_unsched_auto(int hi, const unsigned char* __restrict__ alive, const int* __restrict__ src,
                                    const int* __restrict__ dst, const unsigned char* __restrict__ type,
                                    unsigned char* __restrict__ fl) {
    // type-0 nodes with an arc into a sink (graph_manager.go:1291-1305)
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < hi; s += (long long)gridDim.x * SB)
        if (alive[s] && type[dst[s]] == KS_NODE_SINK && type[src[s]] == KS_NODE_OTHER) fl[src[s]] = 1;
}

__global__ void k_mark_ids(int k, const unsigned long long* __restrict__ ids, unsigned char* __restrict__ fl) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < k; i += (long long)gridDim.x * SB)
        fl[ids[i] - 1] = 1;
}

__global__ void k_mark_tasks(SchedDev d, int hi, unsigned char* __restrict__ fl) {
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < hi; s += (long long)gridDim.x * SB) {
        if (!d.a_alive[s]) continue;
        const int t = d.a_src[s];
        if (d.n_type[t] != KS_NODE_TASK) continue;
        if (d.a_type[s] == 1) atomicOr((unsigned*)&fl[t & ~3], 2u << (8 * (t & 3)));
        if (fl[d.a_dst[s]] & 1) atomicOr((unsigned*)&fl[t & ~3], 4u << (8 * (t & 3)));
    }
}

__device__ __forceinline__ void set_cost(const SchedDev& d, int s, long long c, int* changed) {
    if (d.a_cost[s] == c) return;           // ChangeArcCost emits nothing then (graph_change_manager.go:171-182)
    d.a_cost[s] = c;
    const int p = d.fwd[s];
    if (d.csr_valid && p >= 0) {
        d.pos[p].cost = c * d.mult;
        d.pos[d.pos[p].rev].cost = -c * d.mult;
    }
    atomicAdd(changed, 1);
}

// For each U_j and each task t with an arc t→U_j (U_j's IncomingArcMap): a
// running t gets its running arc set to the continuation cost
// (updateRunningTaskNode, :1140-1158), any other t its t→U_j arc set to (SET) or
// raised by (ADD) the unscheduled cost (updateTaskToUnscheduledAggArc, :1270-1285).
__global__ void k_unsched_costs(SchedDev d, int hi, const unsigned char* __restrict__ fl, int mode, long long ucost,
                                long long ccost, int* __restrict__ changed) {
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < hi; s += (long long)gridDim.x * SB) {
        if (!d.a_alive[s]) continue;
        const int t = d.a_src[s];
        const unsigned char ft = fl[t];
        if (d.n_type[t] != KS_NODE_TASK || !(ft & 4)) continue;
        if (fl[d.a_dst[s]] & 1) {
            if (!(ft & 2)) set_cost(d, (int)s, mode == KS_COST_ADD ? d.a_cost[s] + ucost : ucost, changed);
        } else if (d.a_type[s] == 1) {
            set_cost(d, (int)s, ccost, changed);
        }
    }
}

// --------------------------------------------------------------------- commit ---
// The graph edit of the last solve's deltas as ks_delta records written in device memory
// for store_apply. The items are the tasks with a delta, in delta order.
// Pinned (c.preempt == 0, every item a PLACE): pinTaskToNode (graph_manager.go:675-720)
// with updateUnscheduledAggNode(−1) (:706, :1291-1305) and capacityFromResNodeToParent
// (:662-667).
// Preemptive: updateArcsForScheduledTask with Preemption == true (:855-888): a placed
// task keeps every arc; the one into its PU becomes (or is added as) the running arc with
// low 0, and its arcs into unscheduled aggregators take the preemption cost
// (updateRunningTaskToUnscheduledAggArc, :1164-1181). TaskEvicted (:412-433) deletes the
// running arc and nothing else; TaskMigrated (:407-410) is both.
// Three record families, disjoint in (src, dst): an item's out-arcs (the tail is a task),
// aggregator → sink arcs (the head is the sink), resource arcs (neither).
//
// An item's out-arcs are found in its residual segment, one wave per 64-position chunk
// of it (the chunk items of k_bf_round, built here on device: nch → ch_off by a scan,
// the item's place by bisection): no lane walks a segment.

// One atomicAdd per distinct idx among the pred lanes of a wave (hundreds of tasks
// placed on one PU hit one word: same-word atomics serialise at ~10 ns each).
// Every lane of the wave calls it.
__device__ __forceinline__ void wave_add_distinct(unsigned long long* base, int idx, bool pred) {
    const int me = (int)__lane_id();
    unsigned long long rem = __ballot(pred);
    while (rem) {
        const int l = __ffsll((long long)rem) - 1;
        const int il = __shfl(idx, l);
        const unsigned long long same = __ballot(pred && idx == il) & rem;
        if (me == l) atomicAdd(&base[il], (unsigned long long)__popcll(same));
        rem &= ~same;
    }
}

__device__ __forceinline__ void wave_count(int* ctr, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(ctr, __popcll(m));
}

__global__ void k_commit_items(SchedDev d, CommitDev c, const int* __restrict__ rank,
                               const unsigned long long* __restrict__ newpu, const int* __restrict__ pre,
                               const int* __restrict__ pre_pos, const int* __restrict__ other,
                               const int* __restrict__ other_pos, int npre) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < d.ncap; v += (long long)gridDim.x * SB) {
        int i, kind;
        if (pre[v]) {
            i = pre_pos[v];
            kind = KS_DELTA_PREEMPT;
        } else if (other[v]) {
            i = npre + other_pos[v];
            kind = other[v] == 1 ? KS_DELTA_PLACE : KS_DELTA_MIGRATE;
        } else {
            continue;
        }
        if (i < 0 || i >= c.np) continue;
        c.pl_task[i] = (int)v;
        c.pl_kind[i] = kind;
        c.pl_pu[i] = kind == KS_DELTA_PREEMPT ? -1 : (int)newpu[rank[v]] - 1;
        c.pl_old[i] = kind == KS_DELTA_PLACE ? -1 : (int)d.n_bind[v] - 1;
        const int x = d.perm[v];
        int len = 0;
        if (x >= 0) len = min(d.used[x], d.first[x + 1] - d.first[x]);
        c.nch[i] = (max(len, 0) + 63) >> 6;
        if (!c.preempt) c.fl[v] |= 2;
    }
}

// Chunk item w → its item i (ch_off[i] ≤ w < ch_off[i + 1]) and the position this lane reads.
__device__ __forceinline__ int commit_item(const SchedDev& d, const CommitDev& c, int w, int lane, int* place) {
    int lo = 0, hi = c.np - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.ch_off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    *place = lo;
    const int x = d.perm[c.pl_task[lo]];
    const int b = d.first[x];
    const int len = min(d.used[x], d.first[x + 1] - b);
    const int p = b + ((w - c.ch_off[lo]) << 6) + lane;
    return p < b + len ? p : -1;
}

// The record the live out-arc in slot s of item i gets. 1: the arc into the PU the task
// enters, it becomes the running arc. 2: a delete (DeleteArc's "x src dst 0 0",
// graph_change_manager.go:184-193); pinned every other arc, preemptive the running arc
// into the PU the task leaves (an arc into it that is no running arc counts as missing:
// the reference panics, graph_manager.go:416-419). 3, preemptive: an arc into an
// unscheduled aggregator whose cost changes (ChangeArcCost emits nothing otherwise,
// graph_change_manager.go:171-182). 0: none.
__device__ __forceinline__ int commit_arc_class(const SchedDev& d, const CommitDev& c, int i, int s) {
    const int dst = d.a_dst[s];
    if (dst == c.pl_pu[i]) return 1;
    if (!c.preempt) return 2;
    if (dst == c.pl_old[i]) return d.a_type[s] == 1 ? 2 : 0;
    if ((c.fl[dst] & 1) && c.pl_kind[i] != KS_DELTA_PREEMPT && d.a_cost[s] != c.pcost) return 3;
    return 0;
}

// Chunk item w of both passes: this lane's arc slot *s (−1 if it reads no live out-arc), its
// item *i and the arc's class.
__device__ __forceinline__ int commit_lane_arc(const SchedDev& d, const CommitDev& c, int w, int lane, int* i, int* s) {
    const int p = commit_item(d, c, w, lane, i);
    const int e = p >= 0 ? d.ent[p] : -1;
    *s = e >= 0 && !(e & 1) ? e >> 1 : -1;   // forward positions: the task's out-arcs
    return *s >= 0 ? commit_arc_class(d, c, *i, *s) : 0;
}

__global__ void k_commit_count(SchedDev d, CommitDev c) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(c.ch_off[c.np], c.ni_max);
    // Class counts over this wave's chunk items, one atomic each at the end. Preemptive only:
    // pinned, every wave deletes, and its 16k atomics on one word cost 0.13 ms at 100k
    // tasks; that mode's stats follow from rec_pin and rec_add.
    int converted = 0, removed = 0;
    for (int w = wave; w < ni; w += nwaves) {
        int i, s;
        const int cls = commit_lane_arc(d, c, w, lane, &i, &s);
        if (cls == 1) c.pl_has[i] = 1;
        if (cls == 2) c.pl_found[i] = 1;
        // pinned: the aggregators lose the task (one task per wave and one arc per (src, dst):
        // the lanes' aggregators are distinct words)
        if (!c.preempt && s >= 0 && (c.fl[d.a_dst[s]] & 1)) atomicAdd(&c.agg_cnt[d.a_dst[s]], 1ULL);
        const unsigned long long m = __ballot(cls != 0);
        if (lane == 0) c.icnt[w] = __popcll(m);
        converted += __popcll(__ballot(cls == 1));
        removed += __popcll(__ballot(cls == 2));
    }
    if (c.preempt && lane == 0 && converted) atomicAdd(&c.ctl->converted, converted);
    if (c.preempt && lane == 0 && removed) atomicAdd(&c.ctl->removed, removed);
}

// An item that enters a PU without an arc into it gets the running arc added; one that
// leaves a PU must have found its running arc.
__global__ void k_commit_noarc(CommitDev c) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i <= c.np; i += (long long)gridDim.x * SB) {
        int na = 0;
        if (i < c.np) {
            const int kind = c.pl_kind[i];
            na = kind != KS_DELTA_PREEMPT && !c.pl_has[i];
            if (kind != KS_DELTA_PLACE && !c.pl_found[i]) atomicOr(&c.ctl->bad, 2);
        }
        c.pl_noarc[i] = na;
    }
}

// A PU's slots are the capacity of its arc into the sink. Pinned, its running count is the
// running arcs (type 1) into it that stay — a placed task's own arcs go or are converted —
// plus the tasks this call places on it; the preemptive mode subtracts no running tasks.
__global__ void k_commit_pu_arcs(SchedDev d, CommitDev c) {
    for (long long s0 = blockIdx.x * (long long)SB; s0 < d.hi; s0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long s = s0 + threadIdx.x;
        bool run = false;
        int dst = 0;
        if (s < d.hi && d.a_alive[s]) {
            const int src = d.a_src[s];
            dst = d.a_dst[s];
            if (d.n_type[dst] == KS_NODE_SINK && d.n_type[src] == KS_NODE_PU) c.pu_slots[src] = (unsigned long long)d.a_cap[s];
            // (completing: a completed task's running arc goes with it)
            run = !c.preempt && d.a_type[s] == 1 && !(c.fl[src] & (c.completing ? 2 | RM_FLAG : 2));
        }
        wave_add_distinct(c.pu_run, dst, run);
    }
}

__global__ void k_commit_pu_places(CommitDev c) {
    for (long long i0 = blockIdx.x * (long long)SB; i0 < c.np; i0 += (long long)gridDim.x * SB) {
        const long long i = i0 + threadIdx.x;
        wave_add_distinct(c.pu_run, i < c.np ? c.pl_pu[i] : 0, i < c.np);
    }
}

// The capacity arc slot s gets from this commit: 1 an aggregator → sink arc (minus
// the tasks pinned out of it), 2 a resource arc (slots − running below its head), 0
// none or unchanged.
// Preemptive (capacityFromResNodeToParent returning NumSlotsBelow) kind 1 never fires and
// a resource arc gets slots below its head: running tasks may move.
__device__ __forceinline__ int commit_arc_cap(const SchedDev& d, const CommitDev& c, int s, long long* cap) {
    if (!d.a_alive[s]) return 0;
    const int u = d.a_src[s], v = d.a_dst[s];
    // ks_remove_resources: an arc with an endpoint in the subtree goes with it (no record may
    // name a removed node after its removal)
    if (c.removing && ((c.fl[u] | c.fl[v]) & RM_FLAG)) return 0;
    const unsigned char tu = d.n_type[u], tv = d.n_type[v];
    if (tv == KS_NODE_SINK) {
        // (completing: TaskCompleted's −1 holds under both capacity rules)
        if ((c.preempt && !c.completing) || !(c.fl[u] & 1) || c.agg_cnt[u] == 0) return 0;
        *cap = d.a_cap[s] - (long long)c.agg_cnt[u];
        return 1;
    }
    if (!c.resource_caps || tu == KS_NODE_TASK) return 0;
    const bool res = tv == KS_NODE_PU || tv == KS_NODE_MACHINE || tv == KS_NODE_INTERMEDIATE ||
                     (tv == KS_NODE_OTHER && c.slots[v] > 0);
    if (!res) return 0;
    *cap = (long long)c.slots[v] - (c.preempt ? 0 : (long long)c.running[v]);
    return *cap != d.a_cap[s] ? 2 : 0;
}

__global__ void k_commit_arc_flags(SchedDev d, CommitDev c) {
    for (long long s0 = blockIdx.x * (long long)SB; s0 <= d.hi; s0 += (long long)gridDim.x * SB) {
        const long long s = s0 + threadIdx.x;
        int kind = 0;
        if (s < d.hi) {
            long long cap = 0;
            kind = commit_arc_cap(d, c, (int)s, &cap);
            if (kind && cap < d.a_low[s]) atomicOr(&c.ctl->bad, 1);
        }
        if (s <= d.hi) c.aflag[s] = kind != 0;
        wave_count(&c.ctl->unsched, kind == 1);
        wave_count(&c.ctl->caps, kind == 2);
    }
}

__global__ void k_commit_totals(SchedDev d, CommitDev c) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        c.ctl->rec_pin = c.i_off[c.ni_max];
        c.ctl->rec_add = c.add_off[c.np];
        c.ctl->rec_arc = c.a_off[d.hi];
    }
}

__device__ __forceinline__ ks_delta arc_record(int kind, int type, int src, int dst, long long low, long long cap,
                                               long long cost, long long old_cost) {
    ks_delta r{};
    r.kind = kind;
    r.type = type;
    r.src = (uint64_t)src + 1;
    r.dst = (uint64_t)dst + 1;
    r.low = (uint64_t)low;
    r.cap = (uint64_t)cap;
    r.cost = cost;
    r.old_cost = old_cost;
    return r;
}

// Per out-arc of an item, by class: the running arc (type 1, cap 1, the continuation
// cost; low 1 pins the task, low 0 lets it move), a delete, or the preemption cost.
__global__ void k_commit_emit_items(SchedDev d, CommitDev c, ks_delta* __restrict__ recs) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(c.ch_off[c.np], c.ni_max);
    for (int w = wave; w < ni; w += nwaves) {
        int i, s;
        const int cls = commit_lane_arc(d, c, w, lane, &i, &s);
        const unsigned long long m = __ballot(cls != 0);
        if (!cls) continue;
        const int t = c.pl_task[i], dst = d.a_dst[s];
        const int r = c.i_off[w] + __popcll(m & ((1ULL << lane) - 1));
        const long long co = d.a_cost[s];
        recs[r] = cls == 1   ? arc_record(KS_UPDATE_ARC, 1, t, dst, c.preempt ? 0 : 1, 1, c.ccost, co)
                  : cls == 2 ? arc_record(KS_UPDATE_ARC, d.a_type[s], t, dst, 0, 0, co, co)
                             : arc_record(KS_UPDATE_ARC, d.a_type[s], t, dst, d.a_low[s], d.a_cap[s], c.pcost, co);
    }
}

// An item that enters a PU without an arc into it gets the running arc; every item its
// binding (0 for a PREEMPT: pl_pu is −1).
__global__ void k_commit_emit_adds(SchedDev d, CommitDev c, ks_delta* __restrict__ recs) {
    const int base = c.ctl->rec_pin;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < c.np; i += (long long)gridDim.x * SB) {
        const int t = c.pl_task[i], pu = c.pl_pu[i];
        d.n_bind[t] = (unsigned long long)(pu + 1);
        if (c.pl_noarc[i]) recs[base + c.add_off[i]] = arc_record(KS_ADD_ARC, 1, t, pu, c.preempt ? 0 : 1, 1, c.ccost, 0);
    }
}

__global__ void k_commit_emit_arcs(SchedDev d, CommitDev c, ks_delta* __restrict__ recs) {
    const int base = c.ctl->rec_pin + c.ctl->rec_add;
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < d.hi; s += (long long)gridDim.x * SB) {
        if (!c.aflag[s]) continue;
        long long cap = 0;
        if (!commit_arc_cap(d, c, (int)s, &cap)) continue;
        // capacity 0 removes the arc (the store's low == cap == 0 rule; cap ≥ low was checked)
        const long long co = d.a_cost[s];
        recs[base + c.a_off[s]] = arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], cap ? d.a_low[s] : 0,
                                             cap, co, co);
    }
}

// ------------------------------------------------------------- remove resources ---
// DeregisterResource (flowscheduler/scheduler.go:162-210) on the device-resident graph.
// The subtree is marked by a level-synchronous descent from the roots along forward arcs
// whose head is a PU, a machine or an intermediate resource (traverseAndRemoveTopology,
// graph_manager.go:829-844); the sink, tasks and type-0 nodes are never entered. A frontier
// node's residual segment is cut into 64-position chunk items (chunk counts → scan →
// bisection, as k_commit_items / commit_item), one wave per item: a rack's thousands of
// preference in-arcs cost it their chunks, not one wave walking them. A node is claimed by
// an atomicOr of its flag byte's word; the claiming lanes of a wave take their places in
// the next frontier with one atomic on its counter.

// True for the one caller that sets slot v's RM_FLAG.
__device__ __forceinline__ bool rm_claim(unsigned char* fl, int v) {
    const unsigned bit = (unsigned)RM_FLAG << (8 * (v & 3));
    return !(atomicOr((unsigned*)&fl[v & ~3], bit) & bit);
}

// list[*ctr ...] = v on the pred lanes, in lane order (every lane of the wave calls it).
__device__ __forceinline__ void wave_push(int* list, int* ctr, int v, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (!m) return;
    const int me = (int)__lane_id(), lead = __ffsll((long long)m) - 1;
    int base = 0;
    if (me == lead) base = atomicAdd(ctr, __popcll(m));
    base = __shfl(base, lead);
    if (pred) list[base + __popcll(m & ((1ULL << me) - 1))] = v;
}

// A root must be a live node that is neither a task nor a sink: a PU, a machine, an
// intermediate resource, or a type-0 node (a Quincy rack; an unscheduled aggregator, which
// then goes alone: removeUnscheduledAggNode). A root listed twice is claimed once.
__global__ void k_remove_seed(SchedDev d, RemoveDev r) {
    for (long long i0 = blockIdx.x * (long long)SB; i0 < r.k; i0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long i = i0 + threadIdx.x;
        bool claim = false;
        int v = 0;
        if (i < r.k) {
            const unsigned long long id = r.roots[i];
            bool ok = id >= 1 && id <= (unsigned long long)d.ncap;
            if (ok) {
                v = (int)(id - 1);
                const unsigned char t = d.n_type[v];
                ok = d.n_alive[v] && d.perm[v] >= 0 && t != KS_NODE_TASK && t != KS_NODE_SINK;
            }
            if (ok) claim = rm_claim(r.fl, v);
            else atomicMax(&r.ctl->bad_root, (int)(r.k - i));
        }
        wave_push(r.next, &r.ctl->nfront, v, claim);
    }
}

__device__ __forceinline__ int remove_seg_len(const SchedDev& d, int x) {
    return max(min(d.used[x], d.first[x + 1] - d.first[x]), 0);
}

__global__ void k_remove_chunks(SchedDev d, RemoveDev r, int nf) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i <= nf; i += (long long)gridDim.x * SB)
        r.nch[i] = i < nf ? (remove_seg_len(d, d.perm[r.front[i]]) + 63) >> 6 : 0;
}

// Chunk item w → the frontier node i with ch_off[i] ≤ w < ch_off[i + 1]; the position this
// lane reads in its segment, −1 past the positions handed out.
__device__ __forceinline__ int remove_item_pos(const SchedDev& d, const RemoveDev& r, int nf, int w, int lane) {
    int lo = 0, hi = nf - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (r.ch_off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    const int x = d.perm[r.front[lo]];
    const int b = d.first[x];
    const int p = b + ((w - r.ch_off[lo]) << 6) + lane;
    return p < b + remove_seg_len(d, x) ? p : -1;
}

__global__ void k_remove_level(SchedDev d, RemoveDev r, int nf, int ni_max) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(r.ch_off[nf], ni_max);
    for (int w = wave; w < ni; w += nwaves) {
        const int p = remove_item_pos(d, r, nf, w, lane);
        bool claim = false;
        int us = 0;
        if (p >= 0) {
            const int e = d.ent[p];
            if (e >= 0 && !(e & 1)) {   // forward positions only: the node's live out-arcs
                us = d.iperm[d.pos[p].head];
                if (us >= 0) {
                    const unsigned char t = d.n_type[us];
                    if (t == KS_NODE_PU || t == KS_NODE_MACHINE || t == KS_NODE_INTERMEDIATE) claim = rm_claim(r.fl, us);
                }
            }
        }
        wave_push(r.next, &r.ctl->nfront, us, claim);
    }
}

// dfsEvictTasks (scheduler.go:533-566): the tasks to evict are those the device-kept
// bindings place on a removed node.
__global__ void k_remove_flags(SchedDev d, RemoveDev r) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v <= d.ncap; v += (long long)gridDim.x * SB) {
        int rm = 0, ev = 0;
        if (v < d.ncap) {
            rm = (r.fl[v] & RM_FLAG) != 0;
            if (d.n_alive[v] && d.n_type[v] == KS_NODE_TASK) {
                const unsigned long long b = d.n_bind[v];
                ev = b >= 1 && b <= (unsigned long long)d.ncap && (r.fl[b - 1] & RM_FLAG);
            }
        }
        r.rm[v] = rm;
        r.ev[v] = ev;
    }
}

__global__ void k_remove_zero_pus(SchedDev d, RemoveDev r, CommitDev c) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < d.ncap; v += (long long)gridDim.x * SB)
        if (r.fl[v] & RM_FLAG) c.pu_slots[v] = c.pu_run[v] = 0;
}

__global__ void k_remove_totals(SchedDev d, RemoveDev r, CommitDev c, int caps) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r.ctl->nremoved = r.rm_pos[d.ncap];
        r.ctl->nevicted = r.ev_pos[d.ncap];
        r.ctl->rec_arc = caps ? c.a_off[d.hi] : 0;
        r.ctl->bad = caps ? c.ctl->bad : 0;
        c.ctl->rec_pin = r.rm_pos[d.ncap];   // k_commit_emit_arcs writes behind the REMOVE_NODE records
        c.ctl->rec_add = 0;
    }
}

__global__ void k_remove_emit_nodes(SchedDev d, RemoveDev r, unsigned long long* __restrict__ ids,
                                    ks_delta* __restrict__ recs) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < d.ncap; v += (long long)gridDim.x * SB) {
        if (!r.rm[v]) continue;
        const int i = r.rm_pos[v];
        ids[i] = (unsigned long long)v + 1;
        ks_delta x{};
        x.kind = KS_REMOVE_NODE;
        x.id = (uint64_t)v + 1;
        recs[i] = x;
    }
}

__global__ void k_remove_emit_evictions(SchedDev d, RemoveDev r, ks_sched_delta* __restrict__ out) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < d.ncap; v += (long long)gridDim.x * SB) {
        if (!r.ev[v]) continue;
        out[r.ev_pos[v]] = ks_sched_delta{KS_DELTA_PREEMPT, 0, (uint64_t)v + 1, d.n_bind[v]};
        d.n_bind[v] = 0;   // TaskEvicted: the task is unbound, nothing else of it changes here
    }
}

// --------------------------------------------------------------- complete tasks ---
// HandleTaskCompletion (flowscheduler/scheduler.go:106-132) → TaskCompleted
// (graph_manager.go:389-405) → removeTaskNode (:803-813) on the device-resident graph; TaskFailed
// and TaskKilled (:435-452) are the same edit. The seed is k_remove_seed with the type test
// inverted; a completed task's out-arcs are found in its residual segment, one wave per
// 64-position chunk item (k_remove_chunks → scan → remove_item_pos), so the work follows the
// completions and not the aggregators' in-degree.

// An id must be a live task. left[i] is read here, before the store unbinds the removed
// task. An id listed twice is claimed once; both entries of left get its binding.
__global__ void k_complete_seed(SchedDev d, RemoveDev r, unsigned long long* __restrict__ left) {
    for (long long i0 = blockIdx.x * (long long)SB; i0 < r.k; i0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long i = i0 + threadIdx.x;
        bool claim = false, bound = false;
        int v = 0;
        if (i < r.k) {
            const unsigned long long id = r.roots[i];
            bool ok = id >= 1 && id <= (unsigned long long)d.ncap;
            if (ok) {
                v = (int)(id - 1);
                ok = d.n_alive[v] && d.perm[v] >= 0 && d.n_type[v] == KS_NODE_TASK;
            }
            unsigned long long b = 0;
            if (ok) {
                b = d.n_bind[v];
                claim = rm_claim(r.fl, v);
                bound = claim && b != 0;
            } else {
                atomicMax(&r.ctl->bad_root, (int)(r.k - i));
            }
            left[i] = b;
        }
        wave_push(r.next, &r.ctl->nfront, v, claim);
        wave_count(&r.ctl->nbound, bound);
    }
}

// updateUnscheduledAggNode(−1) (:396, :1291-1305): an aggregator loses one unit per completed
// task that still has an arc into it. The lanes of a wave read one task's arcs, at most one
// per (src, dst): their aggregators are distinct words; waves of one job meet on its word.
__global__ void k_complete_count(SchedDev d, RemoveDev r, CommitDev c, int nf, int ni_max) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(r.ch_off[nf], ni_max);
    for (int w = wave; w < ni; w += nwaves) {
        const int p = remove_item_pos(d, r, nf, w, lane);
        const int e = p >= 0 ? d.ent[p] : -1;
        if (e < 0 || (e & 1)) continue;   // forward positions only: the task's live out-arcs
        const int dst = d.a_dst[e >> 1];
        if (c.fl[dst] & 1) atomicAdd(&c.agg_cnt[dst], 1ULL);
    }
}

__global__ void k_gather_bindings(int k, const unsigned long long* __restrict__ ids,
                                  const unsigned long long* __restrict__ bind, unsigned long long* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < k; i += (long long)gridDim.x * SB)
        out[i] = bind[ids[i] - 1];
}

// -------------------------------------------------------------------- add tasks ---
// AddOrUpdateJobNodes (graph_manager.go:166-208) on the device-resident graph: addTaskNode
// (:632-648), the arcs of updateTaskNode (:1183-1285) and updateUnscheduledAggNode(+1) (:194,
// :1291-1305). The work follows the arrivals: one lane per input arc, one per new task, and a
// pass over the node slots for the aggregators that gain; nothing walks a segment.

// The task of input arc j: the last i with arc_off[i] ≤ j (a task without arcs shares its
// offset with its successor, which owns the arc).
__device__ __forceinline__ int task_of_arc(const unsigned long long* arc_off, int k, long long j) {
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (arc_off[mid] <= (unsigned long long)j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int add_task_of(const AddDev& a, long long j) { return task_of_arc(a.arc_off, a.k, j); }

// A head must be a node that was live before the call and is no task (the new tasks are dead
// slots here: an arc into one of them is refused with the rest). Arrivals of one job meet on
// their aggregator's word, 64 to a wave: the lanes combine into one atomic per distinct
// aggregator (wave_add_distinct), so a job's 5,000 arrivals cost ~80 same-word atomics, not 5,000.
__global__ void k_add_heads(SchedDev d, AddDev a) {
    for (long long j0 = blockIdx.x * (long long)SB; j0 < a.na; j0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long j = j0 + threadIdx.x;
        bool agg = false;
        int v = 0;
        if (j < a.na) {
            const ks_task_arc x = a.arcs[j];
            bool ok = x.dst >= 1 && x.dst <= (unsigned long long)a.nst;
            if (ok) {
                v = (int)(x.dst - 1);
                ok = d.n_alive[v] && d.n_type[v] != KS_NODE_TASK;
            }
            if (!ok) {
                v = 0;
                atomicMax(&a.ctl->bad_head, (int)(a.na - j));
            } else if (x.cost > (1LL << 40) || x.cost < -(1LL << 40)) {
                atomicMax(&a.ctl->bad_cost, (int)(a.na - j));
            } else if (a.fl[v] & 1) {
                agg = true;
                atomicAdd(&a.t_agg[add_task_of(a, j)], 1);   // (a task's own word: one arc per task in a legal call)
            }
        }
        wave_add_distinct(a.agg_cnt, v, agg);
        wave_count(&a.ctl->units, agg);
    }
}

// A task has one job: more than one arc into the flagged aggregators (two of them, or one
// twice) is refused, and under the NULL rule so is none (its aggregator may have lost the arc
// into the sink that would have flagged it).
__global__ void k_add_task_check(AddDev a) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < a.k; i += (long long)gridDim.x * SB) {
        const int c = a.t_agg[i];
        if (c > 1) atomicMax(&a.ctl->bad_multi, (int)(a.k - i));
        else if (c == 0 && a.null_rule) atomicMax(&a.ctl->bad_none, (int)(a.k - i));
    }
}

// The cell of node slot v: the last one with first[cell] ≤ v (as k_mark_cells), −1 outside the partition.
__device__ __forceinline__ int cell_of_slot(const int* __restrict__ first, int ncells, long long v) {
    if (ncells < 1 || v < first[0] || v >= first[ncells]) return -1;
    int lo = 0, hi = ncells;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A union's sink table (one word per cell, −1 before): the first live sink of a cell claims its
// word, any further one turns it into −2. A union has one sink per graph, far apart in slot
// space: each is its own atomic (nothing to combine per wave, as in k_seed_sinks).
__global__ void k_cell_sinks(long long nst, const unsigned char* __restrict__ alive,
                             const unsigned char* __restrict__ type, const int* __restrict__ first, int ncells,
                             int* __restrict__ cell_sink) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < nst; v += (long long)gridDim.x * SB) {
        if (!alive[v] || type[v] != KS_NODE_SINK) continue;
        const int c = cell_of_slot(first, ncells, v);
        if (c < 0) continue;
        if (atomicCAS(&cell_sink[c], -1, (int)v) != -1) atomicExch(&cell_sink[c], -2);
    }
}

// The listed arcs of a batch call leave their graphs' own ids: arc j belongs to the last graph g
// with arc_goff[g] ≤ j (a graph without arcs shares its offset with its successor, which owns
// the arc). A head outside 1..span is reported (the first in input order wins) and becomes 0,
// which the head pass refuses as well; every other head gets its graph's base. Arc: ks_task_arc
// or the 24-byte ks_node_arc of ks_batch_update_nodes; only the dst word of a record is read and
// written, and only an offending lane touches the call's control word.
template <class Arc>
__global__ void k_translate_heads(Arc* __restrict__ arcs, int na, const unsigned long long* __restrict__ arc_goff,
                                  const long long* __restrict__ base, int ng, int* __restrict__ bad_range) {
    for (long long j = blockIdx.x * (long long)SB + threadIdx.x; j < na; j += (long long)gridDim.x * SB) {
        const int g = task_of_arc(arc_goff, ng, j);
        const unsigned long long span = (unsigned long long)(base[g + 1] - base[g]);
        const unsigned long long dst = arcs[j].dst;
        if (dst < 1 || dst > span) {
            atomicMax(bad_range, (int)(na - j));
            arcs[j].dst = 0;
        } else {
            arcs[j].dst = dst + (unsigned long long)base[g];
        }
    }
}

// The sink an aggregator's capacity record ends at: the one sink, or over a union's sink table
// the sink of the aggregator's own cell; negative: there is no such sink.
__device__ __forceinline__ long long add_sink_of(const AddDev& a, long long v) {
    if (!a.cell_sink) return a.sink;
    const int c = cell_of_slot(a.cell_first, a.ncells, v);
    return c < 0 ? -1 : (long long)a.cell_sink[c];
}

// updateUnscheduledAggNode(+1) (:1291-1305): the store's (src, dst) index tells "raise the
// capacity" (the arc is there) from "the arc is gone, re-create it" (:1300-1304).
__global__ void k_add_agg_flags(SchedDev d, AddDev a) {
    for (long long v0 = blockIdx.x * (long long)SB; v0 <= a.nst; v0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long v = v0 + threadIdx.x;
        int f = 0, slot = -1;
        if (v < a.nst && a.agg_cnt[v] > 0) {
            f = 1;
            const long long sink = add_sink_of(a, v);
            if (a.cell_sink && sink < 0) atomicMax(&a.ctl->bad_sink, (int)(a.nst - v));
            if (sink >= 0 && a.hmask >= 0) {
                const int e = store_hfind(a.hkey, a.hmask, arc_hkey(v + 1, sink + 1));
                const int s = e >= 0 ? a.hval[e] : -1;
                if (s >= 0 && s < d.hi && d.a_alive[s]) slot = s;
            }
        }
        if (v <= a.nst) {
            a.aflag[v] = f;
            a.a_slot[v] = slot;
        }
        wave_count(&a.ctl->rec_upd, f && slot >= 0);
        wave_count(&a.ctl->rec_add, f && slot < 0);
    }
}

__global__ void k_add_totals(AddDev a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->rec_agg = a.a_off[a.nst];
}

// Stream positions 0 … k − 1: the ADD_NODE records in input order; k … k + na − 1: the task
// arcs in input order (AddArc(task, head, 0, 1, cost, ArcTypeOther)).
__global__ void k_add_emit_tasks(AddDev a, ks_delta* __restrict__ recs) {
    const long long n = (long long)a.k + a.na;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < n; i += (long long)gridDim.x * SB) {
        if (i < a.k) {
            ks_delta x{};
            x.kind = KS_ADD_NODE;
            x.type = KS_NODE_TASK;
            x.id = a.tasks[i];
            x.excess = 1;
            recs[i] = x;
        } else {
            const long long j = i - a.k;
            const ks_task_arc t = a.arcs[j];
            recs[i] = arc_record(KS_ADD_ARC, 0, (int)(a.tasks[add_task_of(a, j)] - 1), (int)(t.dst - 1), 0, 1, t.cost, 0);
        }
    }
}

// The aggregator records behind them (base: the records before), in ascending aggregator id
// (the scan over the node slots).
__global__ void k_add_emit_aggs(SchedDev d, AddDev a, long long base, ks_delta* __restrict__ recs) {
    for (long long v = blockIdx.x * (long long)SB + threadIdx.x; v < a.nst; v += (long long)gridDim.x * SB) {
        if (!a.aflag[v]) continue;
        const long long cnt = (long long)a.agg_cnt[v];
        const int s = a.a_slot[v];
        const int sink = (int)add_sink_of(a, v);   // (≥ 0: the host refused the call otherwise)
        recs[base + a.a_off[v]] =
            s >= 0 ? arc_record(KS_UPDATE_ARC, d.a_type[s], (int)v, sink, d.a_low[s], d.a_cap[s] + cnt, d.a_cost[s],
                                d.a_cost[s])
                   : arc_record(KS_ADD_ARC, 0, (int)v, sink, 0, cnt, a.sink_cost, 0);
    }
}

// ---------------------------------------------------------------- add resources ---
// AddResourceTopology (graph_manager.go:238-251) on the device-resident graph:
// addResourceTopologyDFS (:557-630) for the new nodes and their arcs, updateResourceStatsUpToRoot
// (:1041-1061) for the arcs above the attach point. The work follows the input: one lane per
// new node, one per edge; the per-slot scratch (newt, par, S) is the only thing written before
// the host has read every refusal.

// wave_add_distinct with a value per lane: one atomicAdd of the summed val per distinct idx
// among the pred lanes of a wave. Every lane of the wave calls it.
__device__ __forceinline__ void wave_sum_distinct(unsigned long long* base, int idx, unsigned long long val, bool pred) {
    const int me = (int)__lane_id();
    unsigned long long rem = __ballot(pred);
    while (rem) {
        const int l = __ffsll((long long)rem) - 1;
        const int il = __shfl(idx, l);
        const bool mine = pred && idx == il;
        const unsigned long long same = __ballot(mine) & rem;
        unsigned long long sum = mine ? val : 0;
        for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
        if (me == l) atomicAdd(&base[il], sum);
        rem &= ~same;
    }
}

// The first offending edge in input order, on one edge the lowest class: one word, one atomicMax.
__device__ __forceinline__ void grow_bad_edge(const GrowDev& g, long long j, int cls) {
    atomicMax(&g.ctl->bad_edge, (int)(8 * (g.m - j) + (7 - cls)));
}

// The type of node id as this call sees it: a node of the call (its slot may be a dead one the
// store still remembers otherwise), else a node that was live before it; −1: neither.
__device__ __forceinline__ int grow_type(const SchedDev& d, const GrowDev& g, unsigned long long id, bool* is_new) {
    *is_new = false;
    if (id < 1 || id > (unsigned long long)g.ntot) return -1;
    const long long v = (long long)id - 1;
    const int t = g.newt[v];
    if (t) {
        *is_new = true;
        return t - 1;
    }
    return v < g.nst && d.n_alive[v] ? (int)d.n_type[v] : -1;
}

// A batch call's resource records leave their graphs' own ids: record i (the nodes, then the
// edges) belongs to the last graph g whose offset is ≤ its index (a graph without records shares
// its offset with its successor, which owns the record). An id outside 1..span is reported (the
// first record in input order wins, nodes before edges) and becomes 0, which the node pass skips
// and the edge pass refuses as well; every other id gets its graph's base. Translating per graph
// is what makes an edge between two cells unrepresentable.
__global__ void k_translate_res(ks_res_node* __restrict__ nodes, int n, ks_res_arc* __restrict__ arcs, int m,
                                const unsigned long long* __restrict__ node_goff,
                                const unsigned long long* __restrict__ arc_goff, const long long* __restrict__ base, int ng,
                                GrowCtl* __restrict__ ctl) {
    const long long tot = (long long)n + m;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < tot; i += (long long)gridDim.x * SB) {
        const bool node = i < n;
        const long long j = node ? i : i - n;
        const int g = task_of_arc(node ? node_goff : arc_goff, ng, j);
        const unsigned long long lo = (unsigned long long)base[g], span = (unsigned long long)(base[g + 1] - base[g]);
        bool bad = false;
        if (node) {
            const unsigned long long id = nodes[j].id;
            bad = id < 1 || id > span;
            nodes[j].id = bad ? 0 : id + lo;
        } else {
            const unsigned long long p = arcs[j].parent, c = arcs[j].child;
            const bool bp = p < 1 || p > span, bc = c < 1 || c > span;
            bad = bp || bc;
            arcs[j].parent = bp ? 0 : p + lo;
            arcs[j].child = bc ? 0 : c + lo;
        }
        if (bad) atomicMax(&ctl->bad_range, (int)(tot - i));
    }
}

// The sink a new PU's arc ends at: the one sink, or over a union's sink table the sink of the PU's
// own cell (the cells' first slots cover a graph's whole span, so an id beyond the store's slots
// finds its cell too); negative: there is no such sink.
__device__ __forceinline__ long long grow_sink_of(const GrowDev& g, long long v) {
    if (!g.cell_sink) return g.sink;
    const int c = cell_of_slot(g.cell_first, g.ncells, v);
    return c < 0 ? -1 : (long long)g.cell_sink[c];
}

// addResourceNode (:528-551): the new nodes into the per-slot scratch. The host checked the
// ids (in range, distinct), so every lane owns its slot's words; an id the translation refused
// is 0 and owns nothing. Over a union's sink table a PU whose cell has no sink or several is
// reported, the first in input order.
__global__ void k_grow_nodes(GrowDev g) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < g.n; i += (long long)gridDim.x * SB) {
        const ks_res_node x = g.nodes[i];
        const int pu = x.type == KS_NODE_PU;
        g.nflag[i] = pu;
        if (x.id < 1 || x.id > (unsigned long long)g.ntot) continue;
        const long long v = (long long)x.id - 1;
        g.newt[v] = 1 + x.type;
        if (pu) g.S[v] = x.slots;
        if (pu && g.cell_sink && grow_sink_of(g, v) < 0) atomicMax(&g.ctl->bad_sink, (int)(g.n - i));
    }
}

// One lane per edge: the endpoints, the kind, the cost; a legal KS_RES_TREE edge claims its
// child's parent word for the first such edge in input order (nodeToParentNode, :618-622).
__global__ void k_grow_edges(SchedDev d, GrowDev g) {
    for (long long j = blockIdx.x * (long long)SB + threadIdx.x; j < g.m; j += (long long)gridDim.x * SB) {
        const ks_res_arc e = g.arcs[j];
        bool pnew, cnew;
        const int tp = grow_type(d, g, e.parent, &pnew), tc = grow_type(d, g, e.child, &cnew);
        int cls = -1;
        if (tp < 0 || tp == KS_NODE_TASK || tp == KS_NODE_SINK || tp == KS_NODE_PU) cls = 0;
        else if (tc < 0 || tc == KS_NODE_TASK || tc == KS_NODE_SINK) cls = 1;
        else if (e.parent == e.child) cls = 2;
        else if (e.kind != KS_RES_TREE && e.kind != KS_RES_EXTRA) cls = 3;
        else if (e.kind == KS_RES_TREE && pnew && !cnew) cls = 4;
        else if (e.cost > (1LL << 40) || e.cost < -(1LL << 40)) cls = 5;
        if (cls >= 0) grow_bad_edge(g, j, cls);
        else if (e.kind == KS_RES_TREE) atomicMax(&g.par[e.child - 1], (int)(g.m - j));
    }
}

// A resource has one parent: a KS_RES_TREE edge whose child an earlier one claimed. (A refused
// edge claims nothing and its own class outranks this one, so it may be tested like the rest.)
__global__ void k_grow_second_parent(GrowDev g) {
    for (long long j = blockIdx.x * (long long)SB + threadIdx.x; j < g.m; j += (long long)gridDim.x * SB) {
        const ks_res_arc e = g.arcs[j];
        if (e.kind == KS_RES_TREE && e.child >= 1 && e.child <= (unsigned long long)g.ntot &&
            g.par[e.child - 1] > (int)(g.m - j))
            grow_bad_edge(g, j, 6);
    }
}

// S(v): every new PU adds its slots to each of its ancestors, the whole wave one step up par at
// a time. The 64 PUs of one machine, or 64 machines of one rack, meet on one word and same-word
// atomics serialise, so each step first combines the lanes: one atomic per
// distinct ancestor per wave (wave_sum_distinct). No PU is an ancestor (a parent is never a PU),
// so the words k_grow_nodes wrote are not touched. Only legal edges claimed par: their parent
// ids are slots of the scratch. A lane whose ancestor after KS_RES_MAX_DEPTH steps still has
// a parent is on a cycle or too deep.
__global__ void k_grow_sums(GrowDev g) {
    for (long long i0 = blockIdx.x * (long long)SB; i0 < g.n; i0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long i = i0 + threadIdx.x;
        long long cur = -1;
        unsigned long long w = 0;
        if (i < g.n) {
            const ks_res_node x = g.nodes[i];
            if (x.type == KS_NODE_PU && x.id >= 1 && x.id <= (unsigned long long)g.ntot) {
                cur = (long long)x.id - 1;
                w = x.slots;
            }
        }
        for (int step = 0; step < KS_RES_MAX_DEPTH; ++step) {
            if (cur >= 0) {
                const int c = g.par[cur];
                cur = c ? (long long)g.arcs[g.m - c].parent - 1 : -1;
            }
            if (!__ballot(cur >= 0)) break;   // (uniform per wave)
            wave_sum_distinct(g.S, cur >= 0 ? (int)cur : 0, w, cur >= 0);
        }
        if (cur >= 0 && g.par[cur]) atomicMax(&g.ctl->bad_depth, (int)(g.n - i));
    }
}

// capacityFromResNodeToParent (:662-667) and updateResourceStatsUpToRoot (:1049-1055): an edge
// whose head has new slots beneath it gets a record. The store's (src, dst) index tells "raise
// the capacity" (the arc is there) from "the arc is gone, re-create it" (its capacity fell to 0).
__global__ void k_grow_edge_flags(SchedDev d, GrowDev g) {
    for (long long j0 = blockIdx.x * (long long)SB; j0 < g.m; j0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long j = j0 + threadIdx.x;
        int f = 0, slot = -1;
        if (j < g.m) {
            const ks_res_arc e = g.arcs[j];
            const bool in = e.child >= 1 && e.child <= (unsigned long long)g.ntot;   // (a refused edge holds anything)
            const unsigned long long sv = in ? g.S[e.child - 1] : 0;
            if (sv > 0) {
                f = 1;
                if (!g.newt[e.child - 1] && e.parent >= 1 && e.parent < (1ULL << 30) && g.hmask >= 0) {
                    const int h = store_hfind(g.hkey, g.hmask, arc_hkey((long long)e.parent, (long long)e.child));
                    const int s = h >= 0 ? g.hval[h] : -1;
                    if (s >= 0 && s < d.hi && d.a_alive[s]) slot = s;
                }
                if (slot >= 0 && (unsigned long long)d.a_cap[slot] + sv > (1ULL << 53))
                    atomicMax(&g.ctl->bad_cap, (int)(g.m - j));
            }
            g.eflag[j] = f;
            g.e_slot[j] = slot;
        }
        wave_count(&g.ctl->rec_upd, f && slot >= 0);
        wave_count(&g.ctl->rec_add, f && slot < 0);
        wave_count(&g.ctl->skipped, j < g.m && !f);
    }
}

__global__ void k_grow_totals(GrowDev g) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g.ctl->rec_pu = g.n_off[g.n];
        g.ctl->rec_edge = g.e_off[g.m];
    }
}

// Stream positions 0 … n − 1: the ADD_NODE records in input order; behind them the PU → sink
// arcs in input order of the PUs (updateResToSinkArc, :1124); behind those the edge records in
// input order (AddArc, :624-627, or ChangeArcCapacity, :1054-1055).
__global__ void k_grow_emit(SchedDev d, GrowDev g, int rec_pu, ks_delta* __restrict__ recs) {
    const long long tot = (long long)g.n + g.m;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < tot; i += (long long)gridDim.x * SB) {
        if (i < g.n) {
            const ks_res_node x = g.nodes[i];
            ks_delta r{};
            r.kind = KS_ADD_NODE;
            r.type = x.type;
            r.id = x.id;
            recs[i] = r;
            if (g.nflag[i])   // (its sink is ≥ 0: the host refused the call otherwise)
                recs[g.n + g.n_off[i]] = arc_record(KS_ADD_ARC, 0, (int)(x.id - 1), (int)grow_sink_of(g, (long long)x.id - 1),
                                                    0, (long long)x.slots, x.sink_cost, 0);
        } else {
            const long long j = i - g.n;
            if (!g.eflag[j]) continue;
            const ks_res_arc e = g.arcs[j];
            const long long sv = (long long)g.S[e.child - 1];
            const int s = g.e_slot[j];
            recs[(long long)g.n + rec_pu + g.e_off[j]] =
                s >= 0 ? arc_record(KS_UPDATE_ARC, d.a_type[s], (int)(e.parent - 1), (int)(e.child - 1), d.a_low[s],
                                    d.a_cap[s] + sv, d.a_cost[s], d.a_cost[s])
                       : arc_record(KS_ADD_ARC, 0, (int)(e.parent - 1), (int)(e.child - 1), 0, sv, e.cost, 0);
        }
    }
}

// ----------------------------------------------------------------- update tasks ---
// UpdateTimeDependentCosts = AddOrUpdateJobNodes (graph_manager.go:211-213, :166-208) for tasks
// that have their node: updateTaskNode (:1183-1192). Each arc writer (:1197-1285) adds the arc the
// graph lacks or calls ChangeArcCost, which logs only a cost that differs
// (graph_change_manager.go:171-182), and then drops the arcs that are no longer preferred
// (removeInvalidECPrefArcs / removeInvalidPrefResArcs, :732-790). Here that is a diff of each
// task's list against the store: a listed arc asks the (src, dst) index for its slot and marks it
// seen; the task's held arcs that nobody marked are found in its own residual segment, one wave
// per 64-position chunk item as in k_complete_count, or with KS_UPDATE_KEEP_UNLISTED (nothing to
// delete, only the aggregator counts to complete) by a pass over the arc table. Three record
// families at fixed positions: held arcs by slot, new arcs in input order, aggregators by id.

// The arc slot of src → dst (node slots), −1: the store does not hold it (u: UpdDev or NodDev).
template <class Dev>
__device__ __forceinline__ int upd_held_slot(const SchedDev& d, const Dev& u, int src, int dst) {
    if (u.hmask < 0) return -1;
    const int e = store_hfind(u.hkey, u.hmask, arc_hkey((long long)src + 1, (long long)dst + 1));
    const int s = e >= 0 ? u.hval[e] : -1;
    return s >= 0 && s < u.hi && d.a_alive[s] ? s : -1;
}

// An id must be a live task and listed once: the first listing holds t_own (atomicMax of k − i),
// every other one loses a comparison there exactly once, as the arriving or the displaced value,
// and is reported then. walk: the task's segment is read, so the id must lie in the built CSR.
__global__ void k_upd_seed(SchedDev d, UpdDev u, int walk) {
    const unsigned long long lim = walk ? (unsigned long long)d.ncap : (unsigned long long)u.nst;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < u.k; i += (long long)gridDim.x * SB) {
        const unsigned long long id = u.tasks[i];
        bool ok = id >= 1 && id <= lim;
        int v = -1, nch = 0;
        if (ok) {
            v = (int)(id - 1);
            ok = d.n_alive[v] && d.n_type[v] == KS_NODE_TASK && (!walk || d.perm[v] >= 0);
        }
        if (ok) {
            const int mine = (int)(u.k - i);
            const int old = atomicMax(&u.t_own[v], mine);
            if (old) atomicMax(&u.ctl->bad_task, min(old, mine));
            if (walk) nch = (remove_seg_len(d, d.perm[v]) + 63) >> 6;
        } else {
            v = -1;
            atomicMax(&u.ctl->bad_task, (int)(u.k - i));
        }
        u.t_slot[i] = v;
        u.nch[i] = nch;
    }
}

// One lane per listed arc. A held arc is marked seen and compared: a running arc keeps its cost
// (:1250-1255), any other gets a record only when the cost differs. An arc the store does not
// hold is an AddArc; into a flagged aggregator it is the task's unit coming back
// (updateUnscheduledAggNode(+1), :1291-1305): an eviction of one job's tasks puts 64 lanes on
// one word, so the lanes combine into one atomic per distinct aggregator (wave_add_distinct).
__global__ void k_upd_heads(SchedDev d, UpdDev u) {
    for (long long j0 = blockIdx.x * (long long)SB; j0 < u.na; j0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long j = j0 + threadIdx.x;
        bool gain = false, cost = false, same = false, run = false;
        int v = 0;
        if (j < u.na) {
            const ks_task_arc x = u.arcs[j];
            bool ok = x.dst >= 1 && x.dst <= (unsigned long long)u.nst;
            if (ok) {
                v = (int)(x.dst - 1);
                ok = d.n_alive[v] && d.n_type[v] != KS_NODE_TASK;
            }
            const int i = task_of_arc(u.arc_off, u.k, j);
            const int t = u.t_slot[i];
            if (!ok) {
                v = 0;
                atomicMax(&u.ctl->bad_head, (int)(u.na - j));
            } else if (x.cost > (1LL << 40) || x.cost < -(1LL << 40)) {
                atomicMax(&u.ctl->bad_cost, (int)(u.na - j));
            } else if (t >= 0) {
                const bool agg = (u.fl[v] & 1) != 0;
                if (agg) atomicAdd(&u.t_agg[i], 1);   // (a task's own word: one such arc per task in a legal call)
                const int s = upd_held_slot(d, u, t, v);
                if (s < 0) {
                    u.lflag[j] = 1;
                    gain = agg;
                } else {
                    u.seen[s] = (int)(u.na - j);
                    run = d.a_type[s] == 1;
                    cost = !run && d.a_cost[s] != x.cost;
                    same = !run && !cost;
                    if (cost) u.sflag[s] = 1;
                }
            }
        }
        wave_add_distinct(u.agg_cnt, v, gain);
        wave_count(&u.ctl->units, gain);
        wave_count(&u.ctl->n_cost, cost);
        wave_count(&u.ctl->n_same, same);
        wave_count(&u.ctl->n_run, run);
    }
}

// A held arc of a listed task that no listed arc named. A running arc stays (the reference's
// removeInvalidPrefResArcs would drop one whose PU left the preferences and panic at the next
// updateRunningTaskNode); an arc into a flagged aggregator stays with its cost, which may have
// aged on the device, and counts as the task's job; any other is no longer preferred. → deleted.
__device__ __forceinline__ bool upd_unlisted(const SchedDev& d, const UpdDev& u, int s) {
    if (!d.a_alive[s] || u.seen[s]) return false;
    const int own = u.t_own[d.a_src[s]];
    if (!own) return false;
    if (u.fl[d.a_dst[s]] & 1) {
        atomicAdd(&u.t_agg[u.k - own], 1);
        return false;
    }
    if (d.a_type[s] == 1 || u.keep) return false;
    u.sflag[s] = 1;
    return true;
}

__global__ void k_upd_walk(SchedDev d, UpdDev u, int ni_max) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(u.ch_off[u.k], ni_max);
    RemoveDev r{};   // (the chunk items of remove_item_pos: the tasks' node slots and their chunk scan)
    r.front = u.t_slot;
    r.ch_off = u.ch_off;
    for (int w = wave; w < ni; w += nwaves) {
        const int p = remove_item_pos(d, r, u.k, w, lane);
        const int e = p >= 0 ? d.ent[p] : -1;
        const bool del = e >= 0 && !(e & 1) && (e >> 1) < u.hi && upd_unlisted(d, u, e >> 1);   // forward positions only
        wave_count(&u.ctl->n_del, del);
    }
}

__global__ void k_upd_table(SchedDev d, UpdDev u) {
    for (long long s0 = blockIdx.x * (long long)SB; s0 < u.hi; s0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long s = s0 + threadIdx.x;
        const bool del = s < u.hi && upd_unlisted(d, u, (int)s);
        wave_count(&u.ctl->n_del, del);
    }
}

// A task does not change its job: arcs into two flagged aggregators, listed, held or a mix, are
// refused. Under the NULL rule an unbound task with none is refused too (its aggregator may have
// lost the arc into the sink that would have flagged it, and its unit would be lost with it); a
// bound task may have none (a pinned running task has no aggregator arc).
__global__ void k_upd_task_check(SchedDev d, UpdDev u) {
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < u.k; i += (long long)gridDim.x * SB) {
        const int t = u.t_slot[i];
        if (t < 0) continue;
        const int c = u.t_agg[i];
        if (c > 1) atomicMax(&u.ctl->bad_multi, (int)(u.k - i));
        else if (c == 0 && u.null_rule && d.n_bind[t] == 0) atomicMax(&u.ctl->bad_none, (int)(u.k - i));
    }
}

__global__ void k_upd_totals(UpdDev u) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        u.ctl->rec_held = u.s_off[u.hi];
        u.ctl->rec_add = u.l_off[u.na];
    }
}

// Stream part 1, ascending arc slot: ChangeArcCost (low, cap and type kept, the listed cost) on a
// seen slot, else the delete (UPDATE_ARC 0/0, as the commit writes it).
__global__ void k_upd_emit_held(SchedDev d, UpdDev u, ks_delta* __restrict__ recs) {
    for (long long s = blockIdx.x * (long long)SB + threadIdx.x; s < u.hi; s += (long long)gridDim.x * SB) {
        if (!u.sflag[s]) continue;
        const long long co = d.a_cost[s];
        const int sn = u.seen[s];
        recs[u.s_off[s]] = sn ? arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], d.a_low[s], d.a_cap[s],
                                           u.arcs[u.na - sn].cost, co)
                              : arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], 0, 0, co, co);
    }
}

// Stream part 2, input order: AddArc(task, head, 0, 1, cost, ArcTypeOther).
__global__ void k_upd_emit_adds(UpdDev u, int rec_held, ks_delta* __restrict__ recs) {
    for (long long j = blockIdx.x * (long long)SB + threadIdx.x; j < u.na; j += (long long)gridDim.x * SB) {
        if (!u.lflag[j]) continue;
        const ks_task_arc x = u.arcs[j];
        recs[(long long)rec_held + u.l_off[j]] =
            arc_record(KS_ADD_ARC, 0, u.t_slot[task_of_arc(u.arc_off, u.k, j)], (int)(x.dst - 1), 0, 1, x.cost, 0);
    }
}

// ----------------------------------------------------------------- update nodes ---
// The other two thirds of updateFlowGraph (graph_manager.go:1012-1033). updateEquivClassNode
// (:931-1010) gives every class arc a cost and a capacity, AddArc(0, cap, cost) where the graph
// lacks it and ChangeArc(low kept, cap, cost) where it holds it, and then drops what is no longer
// preferred (:732-790); updateResOutgoingArcs (:1094-1111) and updateResToSinkArc (:1116-1129)
// re-cost the resource arcs and delete nothing. The diff is that of the tasks' refresh with a
// narrower scratch: a listed arc keeps the slot it found (l_slot), so the one array over the arc
// slots is sflag; the unlisted walk covers the type-0 tails' segments only, one wave per
// 64-position chunk item (a cluster aggregator's segment also holds the reverse positions of
// every task that points at it: no lane walks it).

// An id must be a live class, machine, intermediate node or PU and listed once (the claim of
// k_upd_seed). Only a type-0 tail loses unlisted arcs: every other chunk count is 0.
__global__ void k_nod_seed(SchedDev d, NodDev u, int walk) {
    const unsigned long long lim = walk ? (unsigned long long)d.ncap : (unsigned long long)u.nst;
    for (long long i = blockIdx.x * (long long)SB + threadIdx.x; i < u.k; i += (long long)gridDim.x * SB) {
        const unsigned long long id = u.nodes[i];
        bool ok = id >= 1 && id <= lim;
        int v = -1, nch = 0;
        unsigned char ty = 0;
        if (ok) {
            v = (int)(id - 1);
            ty = d.n_type[v];
            ok = d.n_alive[v] && (!walk || d.perm[v] >= 0) &&
                 (ty == KS_NODE_OTHER || ty == KS_NODE_MACHINE || ty == KS_NODE_INTERMEDIATE || ty == KS_NODE_PU);
        }
        if (ok) {
            const int mine = (int)(u.k - i);
            const int old = atomicMax(&u.n_own[v], mine);
            if (old) atomicMax(&u.ctl->bad_node, min(old, mine));
            if (walk && ty == KS_NODE_OTHER) nch = (remove_seg_len(d, d.perm[v]) + 63) >> 6;
        } else {
            v = -1;
            atomicMax(&u.ctl->bad_node, (int)(u.k - i));
        }
        u.n_slot[i] = v;
        u.nch[i] = nch;
    }
}

// The capacity a listed arc asks for on the held slot s.
__device__ __forceinline__ long long nod_cap(const SchedDev& d, const ks_node_arc& x, int s) {
    return x.cap == KS_CAP_KEEP ? d.a_cap[s] : (long long)x.cap;
}

// One lane per listed arc: the head against its tail's type, then the table's row. The costs,
// the capacities and the repeats are the host's checks, so no two lanes name one slot.
__global__ void k_nod_heads(SchedDev d, NodDev u) {
    for (long long j0 = blockIdx.x * (long long)SB; j0 < u.na; j0 += (long long)gridDim.x * SB) {   // (uniform per workgroup)
        const long long j = j0 + threadIdx.x;
        bool add = false, upd = false, same = false, skip = false, zero = false;
        const int t = j < u.na ? u.n_slot[task_of_arc(u.arc_off, u.k, j)] : -1;
        if (t >= 0) {   // (a refused tail is reported before any arc)
            const ks_node_arc x = u.arcs[j];
            bool ok = x.dst >= 1 && x.dst <= (unsigned long long)u.nst;
            int v = 0;
            if (ok) {
                v = (int)(x.dst - 1);
                const unsigned char tt = d.n_type[t], ht = d.n_type[v];
                ok = d.n_alive[v] && ht != KS_NODE_TASK && v != t &&
                     (ht == KS_NODE_SINK ? (tt == KS_NODE_PU || tt == KS_NODE_OTHER) : tt != KS_NODE_PU);
            }
            if (!ok) {
                atomicMax(&u.ctl->bad_head, (int)(u.na - j));
            } else {
                const int s = upd_held_slot(d, u, t, v);
                if (s < 0) {
                    if (x.cap == KS_CAP_KEEP) atomicMax(&u.ctl->bad_keep, (int)(u.na - j));
                    else if (x.cap == 0) skip = true;
                    else u.lflag[j] = 1, add = true;
                } else {
                    u.l_slot[j] = s + 1;
                    const long long c = nod_cap(d, x, s);
                    if (c < d.a_low[s]) {
                        u.sflag[s] = NOD_LISTED;
                        atomicMax(&u.ctl->bad_low, (int)(u.na - j));
                    } else {
                        zero = c == 0;
                        same = !zero && c == d.a_cap[s] && x.cost == d.a_cost[s];
                        upd = !zero && !same;
                        u.sflag[s] = same ? NOD_LISTED : NOD_RECORD;
                    }
                }
            }
        }
        wave_count(&u.ctl->n_add, add);
        wave_count(&u.ctl->n_upd, upd);
        wave_count(&u.ctl->n_same, same);
        wave_count(&u.ctl->n_skip, skip);
        wave_count(&u.ctl->n_zero, zero);
    }
}

// The arc slot of a type-0 tail's held arc that no listed arc named, −1 for every other
// position: forward positions only, and an arc into a sink stays (removeInvalid* never looks at
// the sink, and an unscheduled aggregator's arc into it belongs to the task calls).
__device__ __forceinline__ int nod_unlisted_slot(const SchedDev& d, const NodDev& u, int w, int lane) {
    RemoveDev r{};   // (the chunk items of remove_item_pos: the tails' node slots and their chunk scan)
    r.front = u.n_slot;
    r.ch_off = u.ch_off;
    const int p = remove_item_pos(d, r, u.k, w, lane);
    const int e = p >= 0 ? d.ent[p] : -1;
    if (e < 0 || (e & 1) || (e >> 1) >= u.hi) return -1;
    const int s = e >> 1;
    if (!d.a_alive[s] || d.n_type[d.a_dst[s]] == KS_NODE_SINK) return -1;
    return s;
}

__global__ void k_nod_walk(SchedDev d, NodDev u, int ni_max) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(u.ch_off[u.k], ni_max);
    for (int w = wave; w < ni; w += nwaves) {
        const int s = nod_unlisted_slot(d, u, w, lane);
        const bool del = s >= 0 && u.sflag[s] == 0;
        if (del) u.sflag[s] = NOD_UNLISTED;
        wave_count(&u.ctl->n_del, del);
    }
}

__global__ void k_nod_totals(NodDev u) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        u.ctl->rec_held = u.s_off[u.hi];
        u.ctl->rec_add = u.l_off[u.na];
    }
}

// One lane per listed arc. A held one with a record writes it at its slot's place in stream part
// 1: ChangeArc (low and type kept, the new capacity, the listed cost), or the delete (UPDATE_ARC
// 0/0, as the commit writes it) of a zeroed arc. One the store lacks is stream part 2, input
// order: AddArc(tail, head, 0, cap, cost, ArcTypeOther).
__global__ void k_nod_emit_listed(SchedDev d, NodDev u, int rec_held, ks_delta* __restrict__ recs) {
    for (long long j = blockIdx.x * (long long)SB + threadIdx.x; j < u.na; j += (long long)gridDim.x * SB) {
        const ks_node_arc x = u.arcs[j];
        if (u.lflag[j]) {
            recs[(long long)rec_held + u.l_off[j]] =
                arc_record(KS_ADD_ARC, 0, u.n_slot[task_of_arc(u.arc_off, u.k, j)], (int)(x.dst - 1), 0, (long long)x.cap,
                           x.cost, 0);
            continue;
        }
        const int s = u.l_slot[j] - 1;
        if (s < 0 || u.sflag[s] != NOD_RECORD) continue;
        const long long c = nod_cap(d, x, s), co = d.a_cost[s];
        recs[u.s_off[s]] = c ? arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], d.a_low[s], c, x.cost, co)
                             : arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], 0, 0, co, co);
    }
}

// The deletes of the unlisted arcs, found by the chunk items as k_nod_walk found them.
__global__ void k_nod_emit_unlisted(SchedDev d, NodDev u, int ni_max, ks_delta* __restrict__ recs) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * SB + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * SB) >> 6;
    const int ni = min(u.ch_off[u.k], ni_max);
    for (int w = wave; w < ni; w += nwaves) {
        const int s = nod_unlisted_slot(d, u, w, lane);
        if (s < 0 || u.sflag[s] != NOD_UNLISTED) continue;
        const long long co = d.a_cost[s];
        recs[u.s_off[s]] = arc_record(KS_UPDATE_ARC, d.a_type[s], d.a_src[s], d.a_dst[s], 0, 0, co, co);
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers ---
hipError_t sched_delta_kinds(const SchedDev& d, const int* is_task, const int* rank, const unsigned long long* newpu,
                             int* pre, int* other, int* bad, hipStream_t st) {
    hipLaunchKernelGGL(k_delta_kinds, dim3(grid(d.ncap)), dim3(SB), 0, st, d.ncap, is_task, rank, newpu,
                       (const unsigned long long*)d.n_bind, d.n_type, (long long)d.nstore, pre, other, bad);
    return hipGetLastError();
}

hipError_t sched_delta_emit(const SchedDev& d, const int* rank, const unsigned long long* newpu, const int* pre,
                            const int* pre_pos, const int* other, const int* other_pos, int npre, ks_sched_delta* out,
                            int commit, hipStream_t st) {
    hipLaunchKernelGGL(k_delta_emit, dim3(grid(d.ncap)), dim3(SB), 0, st, d.ncap, rank, newpu,
                       (const unsigned long long*)d.n_bind, pre, pre_pos, other, other_pos, npre, out, d.n_bind,
                       commit);
    return hipGetLastError();
}

hipError_t sched_running_counts(const SchedDev& d, const unsigned long long* ids, const unsigned long long* vals,
                                int k, unsigned long long* cnt, hipStream_t st) {
    if (ids) {
        if (k) hipLaunchKernelGGL(k_scatter_running, dim3(grid(k)), dim3(SB), 0, st, k, ids, vals, cnt);
    } else if (d.hi) {
        hipLaunchKernelGGL(k_running_into, dim3(grid(d.hi)), dim3(SB), 0, st, d.hi, d.a_alive, d.a_type, d.a_dst, cnt);
    }
    return hipGetLastError();
}

hipError_t sched_topo_level(const SchedDev& d, const int* front, int nfront, int level, int* lvl, int* next,
                            int* nnext, unsigned long long mtpp, const unsigned long long* pu_slots,
                            const unsigned long long* pu_running, unsigned long long* slots,
                            unsigned long long* running, hipStream_t st) {
    const int blocks = std::max(1, std::min(4096, (nfront + 3) / 4));
    hipLaunchKernelGGL(k_topo_level, dim3(blocks), dim3(SB), 0, st, d, front, nfront, level, lvl, next, nnext, mtpp,
                       pu_slots, pu_running, slots, running);
    return hipGetLastError();
}

// fl bit 1 on the unscheduled aggregators: the k node ids, or (ids == nullptr) every type-0
// node with an arc into the sink.
static void mark_aggregators(const SchedDev& d, const unsigned long long* ids, int k, unsigned char* fl,
                             hipStream_t st) {
    if (ids) {
        if (k) hipLaunchKernelGGL(k_mark_ids, dim3(grid(k)), dim3(SB), 0, st, k, ids, fl);
    } else if (d.hi) {
        hipLaunchKernelGGL(k_mark_unsched_auto, dim3(grid(d.hi)), dim3(SB), 0, st, d.hi, d.a_alive, d.a_src, d.a_dst,
                           d.n_type, fl);
    }
}

hipError_t sched_commit_items(const SchedDev& d, const CommitDev& c, const int* rank, const unsigned long long* newpu,
                              const int* pre, const int* pre_pos, const int* other, const int* other_pos, int npre,
                              const unsigned long long* ids, int k, hipStream_t st) {
    mark_aggregators(d, ids, k, c.fl, st);
    if (c.np)
        hipLaunchKernelGGL(k_commit_items, dim3(grid(d.ncap)), dim3(SB), 0, st, d, c, rank, newpu, pre, pre_pos, other,
                           other_pos, npre);
    return hipGetLastError();
}

hipError_t sched_commit_count(const SchedDev& d, const CommitDev& c, hipStream_t st) {
    if (c.np) hipLaunchKernelGGL(k_commit_count, dim3(grid(64LL * c.ni_max)), dim3(SB), 0, st, d, c);
    hipLaunchKernelGGL(k_commit_noarc, dim3(grid(c.np + 1)), dim3(SB), 0, st, c);
    return hipGetLastError();
}

hipError_t sched_commit_pu(const SchedDev& d, const CommitDev& c, hipStream_t st) {
    if (d.hi) hipLaunchKernelGGL(k_commit_pu_arcs, dim3(grid(d.hi)), dim3(SB), 0, st, d, c);
    if (c.np && !c.preempt) hipLaunchKernelGGL(k_commit_pu_places, dim3(grid(c.np)), dim3(SB), 0, st, c);
    return hipGetLastError();
}

hipError_t sched_commit_arc_flags(const SchedDev& d, const CommitDev& c, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_arc_flags, dim3(grid(d.hi + 1)), dim3(SB), 0, st, d, c);
    return hipGetLastError();
}

hipError_t sched_commit_totals(const SchedDev& d, const CommitDev& c, hipStream_t st) {
    hipLaunchKernelGGL(k_commit_totals, dim3(1), dim3(64), 0, st, d, c);
    return hipGetLastError();
}

hipError_t sched_commit_emit(const SchedDev& d, const CommitDev& c, ks_delta* recs, hipStream_t st) {
    if (c.np) {
        hipLaunchKernelGGL(k_commit_emit_items, dim3(grid(64LL * c.ni_max)), dim3(SB), 0, st, d, c, recs);
        hipLaunchKernelGGL(k_commit_emit_adds, dim3(grid(c.np)), dim3(SB), 0, st, d, c, recs);
    }
    // (preemptive without resource capacities: no arc slot is flagged)
    if (d.hi && (!c.preempt || c.resource_caps))
        hipLaunchKernelGGL(k_commit_emit_arcs, dim3(grid(d.hi)), dim3(SB), 0, st, d, c, recs);
    return hipGetLastError();
}

hipError_t sched_remove_seed(const SchedDev& d, const RemoveDev& r, hipStream_t st) {
    if (r.k) hipLaunchKernelGGL(k_remove_seed, dim3(grid(r.k)), dim3(SB), 0, st, d, r);
    return hipGetLastError();
}

hipError_t sched_remove_chunks(const SchedDev& d, const RemoveDev& r, int nf, hipStream_t st) {
    hipLaunchKernelGGL(k_remove_chunks, dim3(grid(nf + 1)), dim3(SB), 0, st, d, r, nf);
    return hipGetLastError();
}

hipError_t sched_remove_level(const SchedDev& d, const RemoveDev& r, int nf, int ni_max, hipStream_t st) {
    hipLaunchKernelGGL(k_remove_level, dim3(grid(64LL * ni_max)), dim3(SB), 0, st, d, r, nf, ni_max);
    return hipGetLastError();
}

hipError_t sched_remove_flags(const SchedDev& d, const RemoveDev& r, hipStream_t st) {
    hipLaunchKernelGGL(k_remove_flags, dim3(grid(d.ncap + 1)), dim3(SB), 0, st, d, r);
    return hipGetLastError();
}

hipError_t sched_remove_zero_pus(const SchedDev& d, const RemoveDev& r, const CommitDev& c, hipStream_t st) {
    if (d.ncap) hipLaunchKernelGGL(k_remove_zero_pus, dim3(grid(d.ncap)), dim3(SB), 0, st, d, r, c);
    return hipGetLastError();
}

hipError_t sched_remove_totals(const SchedDev& d, const RemoveDev& r, const CommitDev& c, int caps, hipStream_t st) {
    hipLaunchKernelGGL(k_remove_totals, dim3(1), dim3(64), 0, st, d, r, c, caps);
    return hipGetLastError();
}

hipError_t sched_remove_emit_nodes(const SchedDev& d, const RemoveDev& r, unsigned long long* ids, ks_delta* recs,
                                   hipStream_t st) {
    if (d.ncap) hipLaunchKernelGGL(k_remove_emit_nodes, dim3(grid(d.ncap)), dim3(SB), 0, st, d, r, ids, recs);
    return hipGetLastError();
}

hipError_t sched_remove_emit_evictions(const SchedDev& d, const RemoveDev& r, ks_sched_delta* out, hipStream_t st) {
    if (d.ncap) hipLaunchKernelGGL(k_remove_emit_evictions, dim3(grid(d.ncap)), dim3(SB), 0, st, d, r, out);
    return hipGetLastError();
}

hipError_t sched_complete_seed(const SchedDev& d, const RemoveDev& r, const unsigned long long* ids, int nu,
                               unsigned long long* left, hipStream_t st) {
    if (!r.k) return hipSuccess;
    // (the byte stores of the aggregator marks come first: the claims are atomicOrs on top of them)
    mark_aggregators(d, ids, nu, r.fl, st);
    hipLaunchKernelGGL(k_complete_seed, dim3(grid(r.k)), dim3(SB), 0, st, d, r, left);
    return hipGetLastError();
}

hipError_t sched_complete_count(const SchedDev& d, const RemoveDev& r, const CommitDev& c, int nf, int ni_max,
                                hipStream_t st) {
    if (nf) hipLaunchKernelGGL(k_complete_count, dim3(grid(64LL * ni_max)), dim3(SB), 0, st, d, r, c, nf, ni_max);
    return hipGetLastError();
}

hipError_t sched_gather_bindings(const SchedDev& d, const unsigned long long* ids, int k, unsigned long long* out,
                                 hipStream_t st) {
    if (k)
        hipLaunchKernelGGL(k_gather_bindings, dim3(grid(k)), dim3(SB), 0, st, k, ids,
                           (const unsigned long long*)d.n_bind, out);
    return hipGetLastError();
}

hipError_t sched_add_check(const SchedDev& d, const AddDev& a, const unsigned long long* ids, int nu, hipStream_t st) {
    mark_aggregators(d, ids, nu, a.fl, st);
    if (a.na) hipLaunchKernelGGL(k_add_heads, dim3(grid(a.na)), dim3(SB), 0, st, d, a);
    if (a.k) hipLaunchKernelGGL(k_add_task_check, dim3(grid(a.k)), dim3(SB), 0, st, a);
    hipLaunchKernelGGL(k_add_agg_flags, dim3(grid(a.nst + 1)), dim3(SB), 0, st, d, a);
    return hipGetLastError();
}

hipError_t sched_cell_sinks(const SchedDev& d, long long nst, const int* cell_first, int ncells, int* cell_sink,
                            hipStream_t st) {
    if (nst > 0 && ncells > 0)
        hipLaunchKernelGGL(k_cell_sinks, dim3(grid(nst)), dim3(SB), 0, st, nst, d.n_alive, d.n_type, cell_first, ncells,
                           cell_sink);
    return hipGetLastError();
}

template <class Arc>
hipError_t sched_translate_heads(Arc* arcs, int na, const unsigned long long* arc_goff, const long long* base, int ng,
                                 int* bad_range, hipStream_t st) {
    if (na > 0 && ng > 0)
        hipLaunchKernelGGL(k_translate_heads<Arc>, dim3(grid(na)), dim3(SB), 0, st, arcs, na, arc_goff, base, ng,
                           bad_range);
    return hipGetLastError();
}
template hipError_t sched_translate_heads(ks_task_arc*, int, const unsigned long long*, const long long*, int, int*, hipStream_t);
template hipError_t sched_translate_heads(ks_node_arc*, int, const unsigned long long*, const long long*, int, int*, hipStream_t);

hipError_t sched_add_totals(const AddDev& a, hipStream_t st) {
    hipLaunchKernelGGL(k_add_totals, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t sched_add_emit(const SchedDev& d, const AddDev& a, ks_delta* recs, hipStream_t st) {
    hipLaunchKernelGGL(k_add_emit_tasks, dim3(grid((long long)a.k + a.na)), dim3(SB), 0, st, a, recs);
    return sched_add_emit_aggs(d, a, (long long)a.k + a.na, recs, st);
}

hipError_t sched_add_agg_flags(const SchedDev& d, const AddDev& a, hipStream_t st) {
    hipLaunchKernelGGL(k_add_agg_flags, dim3(grid(a.nst + 1)), dim3(SB), 0, st, d, a);
    return hipGetLastError();
}

hipError_t sched_add_emit_aggs(const SchedDev& d, const AddDev& a, long long base, ks_delta* recs, hipStream_t st) {
    if (a.nst) hipLaunchKernelGGL(k_add_emit_aggs, dim3(grid(a.nst)), dim3(SB), 0, st, d, a, base, recs);
    return hipGetLastError();
}

hipError_t sched_upd_check(const SchedDev& d, const UpdDev& u, const unsigned long long* ids, int nu, bool walk,
                           hipStream_t st) {
    // (the byte stores of the aggregator marks come first, as in sched_complete_seed)
    mark_aggregators(d, ids, nu, u.fl, st);
    hipLaunchKernelGGL(k_upd_seed, dim3(grid(u.k)), dim3(SB), 0, st, d, u, walk ? 1 : 0);
    if (u.na) hipLaunchKernelGGL(k_upd_heads, dim3(grid(u.na)), dim3(SB), 0, st, d, u);
    return hipGetLastError();
}

hipError_t sched_upd_unlisted(const SchedDev& d, const UpdDev& u, bool walk, int ni_max, hipStream_t st) {
    if (walk) hipLaunchKernelGGL(k_upd_walk, dim3(grid(64LL * ni_max)), dim3(SB), 0, st, d, u, ni_max);
    else if (u.hi) hipLaunchKernelGGL(k_upd_table, dim3(grid(u.hi)), dim3(SB), 0, st, d, u);
    hipLaunchKernelGGL(k_upd_task_check, dim3(grid(u.k)), dim3(SB), 0, st, d, u);
    return hipGetLastError();
}

hipError_t sched_upd_totals(const UpdDev& u, hipStream_t st) {
    hipLaunchKernelGGL(k_upd_totals, dim3(1), dim3(64), 0, st, u);
    return hipGetLastError();
}

hipError_t sched_upd_emit(const SchedDev& d, const UpdDev& u, int rec_held, ks_delta* recs, hipStream_t st) {
    if (u.hi) hipLaunchKernelGGL(k_upd_emit_held, dim3(grid(u.hi)), dim3(SB), 0, st, d, u, recs);
    if (u.na) hipLaunchKernelGGL(k_upd_emit_adds, dim3(grid(u.na)), dim3(SB), 0, st, u, rec_held, recs);
    return hipGetLastError();
}

hipError_t sched_nod_check(const SchedDev& d, const NodDev& u, bool walk, hipStream_t st) {
    hipLaunchKernelGGL(k_nod_seed, dim3(grid(u.k)), dim3(SB), 0, st, d, u, walk ? 1 : 0);
    if (u.na) hipLaunchKernelGGL(k_nod_heads, dim3(grid(u.na)), dim3(SB), 0, st, d, u);
    return hipGetLastError();
}

hipError_t sched_nod_unlisted(const SchedDev& d, const NodDev& u, int ni_max, hipStream_t st) {
    hipLaunchKernelGGL(k_nod_walk, dim3(grid(64LL * ni_max)), dim3(SB), 0, st, d, u, ni_max);
    return hipGetLastError();
}

hipError_t sched_nod_totals(const NodDev& u, hipStream_t st) {
    hipLaunchKernelGGL(k_nod_totals, dim3(1), dim3(64), 0, st, u);
    return hipGetLastError();
}

hipError_t sched_nod_emit(const SchedDev& d, const NodDev& u, bool walk, int ni_max, int rec_held, ks_delta* recs,
                          hipStream_t st) {
    if (u.na) hipLaunchKernelGGL(k_nod_emit_listed, dim3(grid(u.na)), dim3(SB), 0, st, d, u, rec_held, recs);
    if (walk) hipLaunchKernelGGL(k_nod_emit_unlisted, dim3(grid(64LL * ni_max)), dim3(SB), 0, st, d, u, ni_max, recs);
    return hipGetLastError();
}

hipError_t sched_translate_res(ks_res_node* nodes, int n, ks_res_arc* arcs, int m, const unsigned long long* node_goff,
                               const unsigned long long* arc_goff, const long long* base, int ng, GrowCtl* ctl,
                               hipStream_t st) {
    if (n + m > 0 && ng > 0)
        hipLaunchKernelGGL(k_translate_res, dim3(grid((long long)n + m)), dim3(SB), 0, st, nodes, n, arcs, m, node_goff,
                           arc_goff, base, ng, ctl);
    return hipGetLastError();
}

hipError_t sched_grow_check(const SchedDev& d, const GrowDev& g, hipStream_t st) {
    if (g.n) hipLaunchKernelGGL(k_grow_nodes, dim3(grid(g.n)), dim3(SB), 0, st, g);
    if (g.m) hipLaunchKernelGGL(k_grow_edges, dim3(grid(g.m)), dim3(SB), 0, st, d, g);
    if (g.m) hipLaunchKernelGGL(k_grow_second_parent, dim3(grid(g.m)), dim3(SB), 0, st, g);
    if (g.n) hipLaunchKernelGGL(k_grow_sums, dim3(grid(g.n)), dim3(SB), 0, st, g);
    if (g.m) hipLaunchKernelGGL(k_grow_edge_flags, dim3(grid(g.m)), dim3(SB), 0, st, d, g);
    return hipGetLastError();
}

hipError_t sched_grow_totals(const GrowDev& g, hipStream_t st) {
    hipLaunchKernelGGL(k_grow_totals, dim3(1), dim3(64), 0, st, g);
    return hipGetLastError();
}

hipError_t sched_grow_emit(const SchedDev& d, const GrowDev& g, int rec_pu, ks_delta* recs, hipStream_t st) {
    hipLaunchKernelGGL(k_grow_emit, dim3(grid((long long)g.n + g.m)), dim3(SB), 0, st, d, g, rec_pu, recs);
    return hipGetLastError();
}

hipError_t sched_unsched_costs(const SchedDev& d, const unsigned long long* ids, int k, unsigned char* fl, int mode,
                               long long ucost, long long ccost, int* changed, hipStream_t st) {
    mark_aggregators(d, ids, k, fl, st);
    if (d.hi) {
        hipLaunchKernelGGL(k_mark_tasks, dim3(grid(d.hi)), dim3(SB), 0, st, d, d.hi, fl);
        hipLaunchKernelGGL(k_unsched_costs, dim3(grid(d.hi)), dim3(SB), 0, st, d, d.hi, (const unsigned char*)fl, mode,
                           ucost, ccost, changed);
    }
    return hipGetLastError();
}

}  // namespace ks
