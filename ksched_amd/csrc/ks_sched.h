// ks_sched.h — scheduler-side device sweeps of a round (ks_sched.hip), internal.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/ksmcmf.h"
#include "ks_pos.h"

namespace ks {

// Raw pointers the scheduler sweeps read or edit (a view of the engine's store).
struct SchedDev {
    int ncap;                      // node slots covered by the build (ids 1..ncap)
    long long nstore;              // allocated node slots
    const int* perm;               // slot → internal id
    const int* iperm;              // internal id → slot (−1 = padding)
    const unsigned char* n_alive;
    const unsigned char* n_type;
    unsigned long long* n_bind;    // per task slot: bound PU node id, 0 = none (TaskBindings)
    int hi;                        // arc slots handed out
    const unsigned char* a_alive;
    const unsigned char* a_type;
    const int* a_src;
    const int* a_dst;
    const long long* a_low;
    const long long* a_cap;
    long long* a_cost;
    const int* fwd;
    const int* first;              // residual CSR (internal ids)
    const int* used;               // positions handed out in each segment
    Pos* pos;                      // residual positions (ks_pos.h)
    const int* ent;
    long long mult;
    int csr_valid;
};

hipError_t sched_delta_kinds(const SchedDev& d, const int* is_task, const int* rank, const unsigned long long* newpu,
                             int* pre, int* other, int* bad, hipStream_t st);
hipError_t sched_delta_emit(const SchedDev& d, const int* rank, const unsigned long long* newpu, const int* pre,
                            const int* pre_pos, const int* other, const int* other_pos, int npre, ks_sched_delta* out,
                            int commit, hipStream_t st);
hipError_t sched_running_counts(const SchedDev& d, const unsigned long long* ids, const unsigned long long* vals,
                                int k, unsigned long long* cnt, hipStream_t st);
// pu_slots: per node slot, the slots of a PU (ks_commit_schedule: the capacity of its
// arc into the sink); nullptr: every PU has mtpp slots (ks_topology_stats).
hipError_t sched_topo_level(const SchedDev& d, const int* front, int nfront, int level, int* lvl, int* next,
                            int* nnext, unsigned long long mtpp, const unsigned long long* pu_slots,
                            const unsigned long long* pu_running, unsigned long long* slots,
                            unsigned long long* running, hipStream_t st);
hipError_t sched_unsched_costs(const SchedDev& d, const unsigned long long* ids, int k, unsigned char* flags, int mode,
                               long long ucost, long long ccost, int* changed, hipStream_t st);


// ---- ks_commit_schedule and ks_commit_preemptive: the graph edit of the last solve's
// scheduling deltas as ks_delta records generated in device memory. Pinned mode:
// pinTaskToNode (graph_manager.go:675-720), the unscheduled aggregators' capacities
// (:1291-1305) and the resource arcs' (:662-667). Preemptive mode: TaskScheduled with
// Preemption == true (:855-888, :1164-1181), TaskEvicted (:412-433), TaskMigrated
// (:407-410) and the resource arcs' slots below. An item is a task with a delta, in delta
// order (the PREEMPTs first); in the pinned mode every item is a PLACE.
// Device counters of one commit; the host reads them in one copy.
struct CommitCtl {
    int rec_pin;      // records on existing arcs of the items (conversions, deletes, cost changes)
    int rec_add;      // new running arcs
    int rec_arc;      // aggregator and resource-arc capacity records
    int unsched;      // of those, aggregator → sink arcs
    int caps;         // of those, resource arcs
    int bad;          // 1: a capacity would fall below its arc's lower bound; 2: a PREEMPT or MIGRATE
                      // without its running arc
    int converted;    // preemptive: of rec_pin, arcs turned into running arcs
    int removed;      //   and running arcs deleted (the rest of rec_pin are cost records); pinned they stay 0:
                      //   np − rec_add are converted, the rest of rec_pin deleted
};

// Mode and scratch of one commit (device pointers; np items, ni_max chunk items at most).
struct CommitDev {
    int preempt;                   // 0 pinned (ks_commit_schedule), 1 preemptive (ks_commit_preemptive)
    int resource_caps;             // KS_COMMIT_RESOURCE_CAPS: also the resource arcs' capacities
    long long ccost;               // cost of a running arc (continuation)
    long long pcost;               // preemptive: cost of an item's arcs into unscheduled aggregators
    int np;                        // items
    int ni_max;                    // upper bound of the chunk items (np + residual positions / 64)
    int* pl_task;                  // [np + 1] task node slot, in delta order
    int* pl_kind;                  // [np + 1] KS_DELTA_* of the item
    int* pl_pu;                    // [np + 1] PU node slot the task enters, −1 for a PREEMPT
    int* pl_old;                   // [np + 1] PU node slot the task leaves, −1 for a PLACE
    int* pl_has;                   // [np + 1] 1: the arc task → pl_pu exists (it is converted)
    int* pl_found;                 // [np + 1] 1: an arc of the task is deleted (preemptive: the running arc into pl_old)
    int* pl_noarc;                 // [np + 1] 1: the running arc into pl_pu is added; add_off its scan
    int* add_off;                  // [np + 1]
    int* nch;                      // [np + 1] 64-position chunks of the task's segment; ch_off its scan
    int* ch_off;                   // [np + 1]
    int* icnt;                     // [ni_max + 1] records of one chunk item; i_off its scan
    int* i_off;                    // [ni_max + 1]
    int* aflag;                    // [hi + 1] arc slot emits a capacity record; a_off its scan
    int* a_off;                    // [hi + 1]
    unsigned char* fl;             // per node slot: 1 unscheduled aggregator, 2 (pinned) placed by this call
    unsigned long long* agg_cnt;   // per node slot (pinned): items that had an arc into the aggregator
    unsigned long long* pu_slots;  // per node slot: capacity of the PU → sink arc
    unsigned long long* pu_run;    // per node slot (pinned): running arcs into the PU after the commit
    unsigned long long* slots;     // per node slot: slots_below (resource caps)
    unsigned long long* running;   // per node slot: running_below
    CommitCtl* ctl;
    int removing;                  // ks_remove_resources: fl bit 4 marks a removed node; the capacity pass
                                   //   skips every arc with such an endpoint
    int completing;                // ks_complete_tasks: fl bit 4 marks a completed task; its running arc no
                                   //   longer counts, and the aggregator → sink kind fires in both rule modes
};

// The items of the delta kinds (sched_delta_kinds) in delta order, their chunk counts, and
// the aggregator flags (ids: k node ids, or nullptr for every type-0 node with an arc into
// the sink).
hipError_t sched_commit_items(const SchedDev& d, const CommitDev& c, const int* rank, const unsigned long long* newpu,
                              const int* pre, const int* pre_pos, const int* other, const int* other_pos, int npre,
                              const unsigned long long* ids, int k, hipStream_t st);
// Count pass over the chunk items (after the scan nch → ch_off).
hipError_t sched_commit_count(const SchedDev& d, const CommitDev& c, hipStream_t st);
// PU slots, pinned also the running counts, for the resource capacities (before the level BFS).
hipError_t sched_commit_pu(const SchedDev& d, const CommitDev& c, hipStream_t st);
// Arc slots that emit a capacity record (aflag). Pinned: the aggregator → sink arcs and, with
// resource_caps, a resource arc gets slots − running below its head. Preemptive: no aggregator
// record, a resource arc gets slots_below.
hipError_t sched_commit_arc_flags(const SchedDev& d, const CommitDev& c, hipStream_t st);
// Record totals into c.ctl (after the scans icnt → i_off, pl_noarc → add_off, aflag → a_off).
hipError_t sched_commit_totals(const SchedDev& d, const CommitDev& c, hipStream_t st);
// Emit pass: the records into recs (item records, then new running arcs, then capacities) and
// the bindings of every item.
hipError_t sched_commit_emit(const SchedDev& d, const CommitDev& c, ks_delta* recs, hipStream_t st);

// ---- ks_remove_resources: a resource subtree leaves the graph. DeregisterResource
// (flowscheduler/scheduler.go:162-210): dfsEvictTasks (:533-566) → TaskEvicted
// (graph_manager.go:412-433) for every task bound in the subtree, RemoveResourceTopology
// (:362-387) with traverseAndRemoveTopology (:829-844) for its nodes, and the ancestors'
// capacities (updateResourceStatsUpToRoot) through the commit's capacity pass over the
// graph without the subtree. The REMOVE_NODE records and the capacity records are
// generated in device memory for store_apply, as a commit's.
constexpr unsigned char RM_FLAG = 4;   // CommitDev::fl bit of a node in the removed subtree

// Device counters of one removal; the host reads them in one 32-byte copy.
struct RemoveCtl {
    int nfront;      // nodes the seed or the running level claimed: the next frontier's length
    int bad_root;    // k − the index of the first illegal root (dead, out of range, a task or a sink), 0 none
    int nremoved;    // flagged node slots (the REMOVE_NODE records, stream positions 0 … nremoved − 1)
    int nevicted;    // live tasks whose binding names a flagged slot
    int rec_arc;     // capacity records (resource arcs whose capacity changes)
    int bad;         // 1: a capacity would fall below its arc's lower bound
    int nbound;      // ks_complete_tasks: of the claimed tasks, those bound to a PU
    int reserved;
};

// Scratch of one removal (device pointers; ncap node slots).
struct RemoveDev {
    const unsigned long long* roots;   // [k] the caller's root ids, unchecked
    int k;
    unsigned char* fl;                 // per node slot (word-aligned length): RM_FLAG
    int* front;                        // [ncap + 1] node slots of the level being expanded
    int* next;                         // [ncap + 1] node slots it claims
    int* nch;                          // [ncap + 1] 64-position chunks of a frontier node's segment; ch_off its scan
    int* ch_off;                       // [ncap + 1]
    int* rm;                           // [ncap + 1] 1: the slot is removed; rm_pos its scan
    int* rm_pos;                       // [ncap + 1]
    int* ev;                           // [ncap + 1] 1: a live task bound to a removed slot; ev_pos its scan
    int* ev_pos;                       // [ncap + 1]
    RemoveCtl* ctl;
};

// Check and flag the roots; the distinct legal ones are the first frontier (next, ctl->nfront).
hipError_t sched_remove_seed(const SchedDev& d, const RemoveDev& r, hipStream_t st);
// Chunk counts of the nf frontier nodes (before the scan nch → ch_off).
hipError_t sched_remove_chunks(const SchedDev& d, const RemoveDev& r, int nf, hipStream_t st);
// One level of the descent: one wave per 64-position chunk item of the frontier's segments
// follows the live forward arcs into PUs, machines and intermediate nodes and claims them
// (next, ctl->nfront; the caller zeroes nfront first). ni_max bounds the chunk items.
hipError_t sched_remove_level(const SchedDev& d, const RemoveDev& r, int nf, int ni_max, hipStream_t st);
// Per node slot: removed (rm), a live task whose binding is removed (ev).
hipError_t sched_remove_flags(const SchedDev& d, const RemoveDev& r, hipStream_t st);
// A removed PU has no slots and runs nothing: the capacity sums are those of the graph
// without the subtree (after sched_commit_pu, before the level BFS).
hipError_t sched_remove_zero_pus(const SchedDev& d, const RemoveDev& r, const CommitDev& c, hipStream_t st);
// Totals into r.ctl after the scans (caps: also a_off and the capacity pass's bad word),
// and the capacity records' base into c.ctl (they follow the REMOVE_NODE records).
hipError_t sched_remove_totals(const SchedDev& d, const RemoveDev& r, const CommitDev& c, int caps, hipStream_t st);
// The removed ids ascending and their REMOVE_NODE records at stream positions 0 … nremoved − 1.
hipError_t sched_remove_emit_nodes(const SchedDev& d, const RemoveDev& r, unsigned long long* ids, ks_delta* recs,
                                   hipStream_t st);
// One PREEMPT (task, the PU it leaves) per evicted task in task order; the task is unbound.
hipError_t sched_remove_emit_evictions(const SchedDev& d, const RemoveDev& r, ks_sched_delta* out, hipStream_t st);

// ---- ks_complete_tasks: finished tasks leave the graph. HandleTaskCompletion
// (flowscheduler/scheduler.go:106-132) → TaskCompleted (flowmanager/graph_manager.go:389-405)
// → removeTaskNode (:803-813) with updateUnscheduledAggNode(−1) (:396, :1291-1305); TaskFailed
// and TaskKilled (:435-452) are the same edit. The scratch is the removal's (RemoveDev: roots
// are the caller's task ids, RM_FLAG marks a completed task) and the commit's in its
// completing mode; the flag scan, the REMOVE_NODE records and the capacity records are
// sched_remove_flags / _totals / _emit_nodes and sched_commit_arc_flags / _emit.

// The aggregator flags (ids: nu node ids, or nullptr for every type-0 node with an arc into
// the sink) into r.fl, then the check of the k ids: each must be a live task, else
// ctl->bad_root = k − its index (the first one wins). left[i] = the PU ids[i] is bound to;
// the distinct tasks are claimed (next, ctl->nfront), ctl->nbound of them bound.
hipError_t sched_complete_seed(const SchedDev& d, const RemoveDev& r, const unsigned long long* ids, int nu,
                               unsigned long long* left, hipStream_t st);
// One wave per 64-position chunk item of the nf claimed tasks' segments (r.front, after
// sched_remove_chunks and the scan nch → ch_off): c.agg_cnt[a] += 1 per live out-arc into a
// flagged aggregator a. ni_max bounds the chunk items.
hipError_t sched_complete_count(const SchedDev& d, const RemoveDev& r, const CommitDev& c, int nf, int ni_max,
                                hipStream_t st);
// ks_get_bindings: out[i] = the PU ids[i] is bound to (ids checked by the caller).
hipError_t sched_gather_bindings(const SchedDev& d, const unsigned long long* ids, int k, unsigned long long* out,
                                 hipStream_t st);

// ---- ks_add_tasks: arriving tasks enter the graph. AddOrUpdateJobNodes
// (flowmanager/graph_manager.go:166-208) → addTaskNode (:632-648), updateUnscheduledAggNode(+1)
// (:194, :1291-1305) and updateTaskNode (:1183-1192) with its arc writers (:1197-1285), each an
// AddArc(task, head, 0, 1, cost, ArcTypeOther). The ids are the host's business (its node
// table); the device checks every arc's head against node liveness and types, counts the
// aggregators' gains, asks the store's (src, dst) index whether each gaining aggregator still
// has its arc into the sink, and writes the ADD_NODE, ADD_ARC and aggregator records at fixed
// stream positions for store_apply. Only the node store, the arc table and the index are
// read: no residual CSR is needed and no BFS runs.

// Device counters of one arrival; the host reads them in one copy.
struct AddCtl {
    int bad_head;    // na − the index of the first arc whose head is 0, beyond the graph, dead or a task, 0 none
    int bad_cost;    // na − the index of the first arc whose cost is beyond ±2^40, 0 none
    int bad_multi;   // k − the index of the first task with more than one arc into flagged aggregators, 0 none
    int bad_none;    // k − the index of the first task with none (counted under the NULL rule only), 0 none
    int units;       // arcs into flagged aggregators: the capacity the aggregators gain
    int rec_upd;     // gaining aggregators whose arc into the sink the store holds (UPDATE_ARC)
    int rec_add;     // gaining aggregators without it (ADD_ARC)
    int rec_agg;     // the scan's total: rec_upd + rec_add
    int bad_sink;    // per-cell sinks: nst − the slot of the first gaining aggregator whose cell has no single sink, 0 none
    int bad_range;   // batch ids: na − the index of the first arc whose head lies outside 1..span of its graph, 0 none
};

// Inputs and scratch of one arrival (device pointers; nst node slots before the call).
struct AddDev {
    int k;                             // tasks
    int na;                            // arcs
    const unsigned long long* tasks;   // [k] the new ids, checked by the host
    const unsigned long long* arc_off; // [k + 1] checked by the host: 0 first, never decreasing, na last
    const ks_task_arc* arcs;           // [na] unchecked
    long long nst;                     // node slots the head pass may read
    unsigned char* fl;                 // per node slot: 1 unscheduled aggregator
    int* t_agg;                        // [k + 1] arcs of task i into flagged aggregators
    unsigned long long* agg_cnt;       // [nst + 1] per node slot: arriving tasks with an arc into the aggregator
    int* aflag;                        // [nst + 1] 1: the aggregator gains and gets a record; a_off its scan
    int* a_off;                        // [nst + 1]
    int* a_slot;                       // [nst + 1] arc slot of aggregator → sink, −1: the store does not hold it
    int null_rule;                     // unsched_ids == NULL: a task without an aggregator arc is refused
    long long sink;                    // the sink's node slot, −1: other than one sink
    long long sink_cost;               // cost of a re-created aggregator → sink arc
    const int* cell_sink;              // [ncells] a union's sinks (sched_cell_sinks): an aggregator's records end
                                       //   at its own cell's sink, and sink is not read; nullptr: the one sink
    const int* cell_first;             // [ncells + 1] the cells' first node slots
    int ncells;
    const unsigned long long* hkey;    // the store's (src, dst) index (ks_store.h)
    const int* hval;
    int hmask;                         // capacity − 1, −1: no index yet
    AddCtl* ctl;
};

// A union's sinks: cell_sink[c] = the node slot of cell c's one live sink, negative when the
// cell has none or several (cell_sink starts at −1 in every word; nst node slots are read, each
// live sink finds its cell by bisection over cell_first).
hipError_t sched_cell_sinks(const SchedDev& d, long long nst, const int* cell_first, int ncells, int* cell_sink,
                            hipStream_t st);
// A batch call's listed arcs, the graphs' lists back to back (graph g owns the arcs
// [arc_goff[g], arc_goff[g + 1]) and the union ids (base[g], base[g + 1]]): one lane per arc
// finds its graph by bisection, checks 1 ≤ dst ≤ span (else *bad_range, the call's control word
// of that name, and the head becomes 0) and adds the graph's base in place. Only the dst word of a
// record is read and written: the 16-byte arcs of the task lists and the 24-byte arcs of the
// node lists (whose cost and capacity are the host's to check) go through the same kernel
// (Arc: ks_task_arc or ks_node_arc, instantiated in ks_sched.hip).
template <class Arc>
hipError_t sched_translate_heads(Arc* arcs, int na, const unsigned long long* arc_goff, const long long* base, int ng,
                                 int* bad_range, hipStream_t st);

// The aggregator flags (ids: nu node ids, or nullptr for every type-0 node with an arc into the
// sink) into a.fl; the head pass, one lane per arc (head and cost checks, t_agg, agg_cnt with one
// atomic per distinct aggregator per wave, ctl->units); the per-task count check; the
// per-aggregator lookup (aflag, a_slot, ctl->rec_upd / rec_add). The caller scans aflag → a_off.
hipError_t sched_add_check(const SchedDev& d, const AddDev& a, const unsigned long long* ids, int nu, hipStream_t st);
// ctl->rec_agg after the scan.
hipError_t sched_add_totals(const AddDev& a, hipStream_t st);
// The records: ADD_NODE at 0 … k − 1, the task arcs at k + their index, the aggregator records
// in ascending id behind them (d: the arc table as it is now, after any growth).
hipError_t sched_add_emit(const SchedDev& d, const AddDev& a, ks_delta* recs, hipStream_t st);

// ---- ks_add_resources: machines, racks and PUs join the graph. AddResourceTopology
// (flowmanager/graph_manager.go:238-251) → addResourceTopologyDFS (:557-630) with addResourceNode
// (:528-551), updateResToSinkArc (:1116-1129) and capacityFromResNodeToParent (:662-667), and
// updateResourceStatsUpToRoot (:1041-1061) above the attach point. The ids and the nodes'
// values are the host's business (its node table); the device checks every edge's endpoints
// against node liveness and types, sums the new PUs' slots up the KS_RES_TREE edges, asks the
// store's (src, dst) index whether each edge into a live head is still held, and writes the
// ADD_NODE, PU → sink and edge records at fixed stream positions for store_apply. Only the node
// store, the arc table and the index are read: no residual CSR is needed and no BFS runs.

// Device counters of one growth; the host reads them in one 40-byte copy.
struct GrowCtl {
    int bad_edge;    // 8·(m − j) + (7 − class) of the first offending edge j, lowest class first; 0 none.
                     // class 0 parent, 1 child, 2 parent == child, 3 kind, 4 a live node would move,
                     // 5 cost, 6 a second KS_RES_TREE edge into the child
    int bad_depth;   // n − the index of the first new PU whose walk has not ended after KS_RES_MAX_DEPTH
                     // edges, 0 none
    int bad_cap;     // m − the index of the first edge whose raised capacity exceeds 2^53, 0 none
    int rec_upd;     // edges whose arc the store holds (UPDATE_ARC)
    int rec_add;     // edges that create their arc (ADD_ARC)
    int skipped;     // edges without a record (no new slot beneath the head)
    int rec_pu;      // the node scan's total: PU → sink records
    int rec_edge;    // the edge scan's total: rec_upd + rec_add
    int bad_sink;    // per-cell sinks: n − the index of the first new PU whose cell has no single sink, 0 none
    int bad_range;   // batch ids: n + m − the index (nodes, then edges) of the first record with an id outside
                     // 1..span of its graph, 0 none
};

// Inputs and scratch of one growth (device pointers). nst node slots before the call, ntot ≥
// nst slots with the highest new id: the per-slot scratch covers ids beyond the store.
struct GrowDev {
    int n;                             // new nodes
    int m;                             // edges
    const ks_res_node* nodes;          // [n] checked by the host
    const ks_res_arc* arcs;            // [m] unchecked
    long long nst;                     // node slots whose liveness and type may be read
    long long ntot;                    // node slots of the scratch
    int* newt;                         // [ntot + 1] per node slot: 1 + the type of a new node, 0: not of this call
    int* par;                          // [ntot + 1] per node slot: m − j of the first KS_RES_TREE edge j into it, 0
                                       //   none (claimed with atomicMax, so the array starts zeroed)
    unsigned long long* S;             // [ntot + 1] per node slot: the new slots beneath it
    int* nflag;                        // [n + 1] 1: node i is a PU (its arc into the sink); n_off its scan
    int* n_off;                        // [n + 1]
    int* eflag;                        // [m + 1] 1: edge j gets a record; e_off its scan
    int* e_off;                        // [m + 1]
    int* e_slot;                       // [m + 1] arc slot of parent → child, −1: the store does not hold it
    long long sink;                    // the sink's node slot, −1: other than one sink
    const int* cell_sink;              // [ncells] a union's sinks (sched_cell_sinks): a new PU's arc ends at its
                                       //   own cell's sink, and sink is not read; nullptr: the one sink
    const int* cell_first;             // [ncells + 1] the cells' first node slots (they cover every id of a
                                       //   graph's span, also ids beyond the store's slots)
    int ncells;
    const unsigned long long* hkey;    // the store's (src, dst) index (ks_store.h)
    const int* hval;
    int hmask;                         // capacity − 1, −1: no index yet
    GrowCtl* ctl;
};

// A batch call's resource records, the graphs' lists back to back (graph g owns the nodes
// [node_goff[g], node_goff[g + 1]), the edges [arc_goff[g], arc_goff[g + 1]) and the union ids
// (base[g], base[g + 1]]): one lane per node record and one per edge record finds its graph by
// bisection, checks 1 ≤ id ≤ span for the node id and for both endpoints (else ctl->bad_range,
// and the id becomes 0, which every later pass refuses or skips) and adds the graph's base in place.
hipError_t sched_translate_res(ks_res_node* nodes, int n, ks_res_arc* arcs, int m, const unsigned long long* node_goff,
                               const unsigned long long* arc_goff, const long long* base, int ng, GrowCtl* ctl,
                               hipStream_t st);

// The new nodes into the per-slot scratch (newt, S of the PUs, nflag); the edge pass, one lane
// per edge (endpoints, kind, cost, the claim of par); the second-parent check; the sums, one
// lane per new PU walking par with one atomic per distinct ancestor per wave and step; the
// per-edge lookup (eflag, e_slot, ctl->rec_upd / rec_add / skipped / bad_cap). Nothing outside
// the scratch is written. The caller scans nflag → n_off and eflag → e_off.
hipError_t sched_grow_check(const SchedDev& d, const GrowDev& g, hipStream_t st);
// ctl->rec_pu and ctl->rec_edge after the scans.
hipError_t sched_grow_totals(const GrowDev& g, hipStream_t st);
// The records: ADD_NODE at 0 … n − 1, the PU → sink arcs at n + n_off, the edge records at
// n + rec_pu + e_off (d: the arc table as it is now, after any growth).
hipError_t sched_grow_emit(const SchedDev& d, const GrowDev& g, int rec_pu, ks_delta* recs, hipStream_t st);

// ---- ks_update_tasks: live tasks' arcs follow the cost model. UpdateTimeDependentCosts =
// AddOrUpdateJobNodes (flowmanager/graph_manager.go:211-213, :166-208) → updateTaskNode
// (:1183-1192) with its arc writers (:1197-1285), each AddArc or ChangeArcCost
// (graph_change_manager.go:171-182) followed by removeInvalidECPrefArcs /
// removeInvalidPrefResArcs (:732-790), and updateRunningTaskNode (:1140-1158). The device
// diffs each listed task's list against the arcs the store holds: a listed arc is found
// through the store's (src, dst) index, a held arc nobody listed in the task's own residual
// segment (or, with KS_UPDATE_KEEP_UNLISTED, in a pass over the arc table: no CSR is needed
// then). The aggregators' part (aflag, a_off, a_slot, the lookup and the records) is that of
// ks_add_tasks on an AddDev that shares fl and agg_cnt.

// Device counters of one refresh; the host reads them in one 64-byte copy.
struct UpdCtl {
    int bad_task;    // k − the index of the first id that is 0, beyond the graph, dead, no task or listed before, 0 none
    int bad_head;    // na − the index of the first arc whose head is 0, beyond the graph, dead or a task, 0 none
    int bad_cost;    // na − the index of the first arc whose cost is beyond ±2^40, 0 none
    int bad_multi;   // k − the index of the first task that would end with arcs into two flagged aggregators, 0 none
    int bad_none;    // k − the index of the first unbound task that would end with none (NULL rule only), 0 none
    int units;       // listed arcs into flagged aggregators that the store did not hold: the aggregators' gain
    int n_cost;      // listed, held with type 0, another cost (UPDATE_ARC)
    int n_same;      // listed, held with type 0, the same cost
    int n_run;       // listed, held as a running arc
    int n_del;       // held, unlisted, deleted
    int rec_held;    // the arc-slot scan's total: n_cost + n_del
    int rec_add;     // the listed-arc scan's total: listed arcs the store did not hold (ADD_ARC)
    int reserved[4];
};

// Inputs and scratch of one refresh (device pointers; nst node slots, hi arc slots).
struct UpdDev {
    int k;                             // tasks
    int na;                            // listed arcs
    int hi;                            // arc slots handed out when the call began
    int keep;                          // KS_UPDATE_KEEP_UNLISTED: nothing is deleted, no segment is walked
    int null_rule;                     // unsched_ids == NULL: an unbound task without an aggregator arc is refused
    const unsigned long long* tasks;   // [k] unchecked
    const unsigned long long* arc_off; // [k + 1] checked by the host: 0 first, never decreasing, na last
    const ks_task_arc* arcs;           // [na] unchecked (a head repeated within one task: the host's sort)
    long long nst;                     // node slots the passes may read
    unsigned char* fl;                 // per node slot: 1 unscheduled aggregator
    int* t_own;                        // [nst + 1] per node slot: k − i of the first listing i of the task, 0: not
                                       //   listed (claimed with atomicMax, so the array starts zeroed)
    int* t_slot;                       // [k + 1] node slot of task i, −1: the id is refused
    int* t_agg;                        // [k + 1] arcs into flagged aggregators task i would end with
    int* nch;                          // [k + 1] 64-position chunks of task i's segment; ch_off its scan
    int* ch_off;                       // [k + 1]
    int* seen;                         // [hi + 1] per arc slot: na − j of the listed arc j that names it, 0 none
    int* sflag;                        // [hi + 1] 1: the arc slot gets a record (a cost change where seen, else a
                                       //   deletion); s_off its scan
    int* s_off;                        // [hi + 1]
    int* lflag;                        // [na + 1] 1: the store does not hold listed arc j (ADD_ARC); l_off its scan
    int* l_off;                        // [na + 1]
    unsigned long long* agg_cnt;       // [nst + 1] per node slot: the aggregator's gain
    const unsigned long long* hkey;    // the store's (src, dst) index (ks_store.h)
    const int* hval;
    int hmask;                         // capacity − 1, −1: no index yet
    UpdCtl* ctl;
};

// The aggregator flags (ids: nu node ids, or nullptr for every type-0 node with an arc into the
// sink) into u.fl; the task seed, one lane per id (liveness, type, the claim of t_own, t_slot,
// nch; walk: the id must lie in the built CSR, whose segments are walked); the listed-arc pass,
// one lane per arc (head and cost checks, the index lookup, seen, sflag / lflag, t_agg, agg_cnt
// with one atomic per distinct aggregator per wave). Nothing outside the scratch is written.
// The caller scans nch → ch_off when it walks.
hipError_t sched_upd_check(const SchedDev& d, const UpdDev& u, const unsigned long long* ids, int nu, bool walk,
                           hipStream_t st);
// The held arcs nobody listed (kept: running arcs and arcs into flagged aggregators, which count
// into t_agg; else sflag, n_del): walk, one wave per 64-position chunk item of the tasks'
// segments (ni_max bounds the items), else one lane per arc slot. Then the per-task check
// (bad_multi, bad_none). The caller scans sflag → s_off and lflag → l_off.
hipError_t sched_upd_unlisted(const SchedDev& d, const UpdDev& u, bool walk, int ni_max, hipStream_t st);
// ctl->rec_held and ctl->rec_add after the scans.
hipError_t sched_upd_totals(const UpdDev& u, hipStream_t st);
// The records on held arcs at s_off (ascending arc slot), the ADD_ARC records of the listed
// arcs at rec_held + l_off (input order); d: the arc table as it is now, after any growth.
hipError_t sched_upd_emit(const SchedDev& d, const UpdDev& u, int rec_held, ks_delta* recs, hipStream_t st);
// The aggregator part of ks_add_tasks alone: the per-aggregator lookup (a.aflag, a.a_slot,
// ctl->rec_upd / rec_add), and the aggregator records at base + a.a_off.
hipError_t sched_add_agg_flags(const SchedDev& d, const AddDev& a, hipStream_t st);
hipError_t sched_add_emit_aggs(const SchedDev& d, const AddDev& a, long long base, ks_delta* recs, hipStream_t st);

// ---- ks_update_nodes: class and resource arcs follow the cost model. The rest of the sweep of
// AddOrUpdateJobNodes → updateFlowGraph (flowmanager/graph_manager.go:1012-1033):
// updateEquivClassNode (:931-1010), each AddArc or ChangeArc with a cost and a capacity, then
// removeInvalidECPrefArcs / removeInvalidPrefResArcs (:732-790); updateResourceNode →
// updateResOutgoingArcs (:1094-1111) with updateResToSinkArc (:1116-1129). The tails are few and
// wide, so the scratch is per listed arc and per chunk position: a listed arc finds its slot
// through the store's (src, dst) index, a type-0 tail's held arcs nobody listed are found in its
// residual segment. One array over the arc slots (sflag) and its scan give the held records
// their ascending-slot order.

// sflag of an arc slot: what the call found for it.
constexpr int NOD_LISTED = 1;     // a listed arc names it, no record (same cost and capacity)
constexpr int NOD_RECORD = 2;     // a listed arc names it and it gets a record (an update or the 0/0 of a zeroed arc)
constexpr int NOD_UNLISTED = 3;   // a type-0 tail's arc nobody listed: deleted

// Device counters of one refresh; the host reads them in one 64-byte copy.
struct NodCtl {
    int bad_node;    // k − the index of the first id that is 0, beyond the graph, dead, a task, a sink or listed before, 0 none
    int bad_head;    // na − the index of the first arc whose head is illegal for its tail, 0 none
    int bad_keep;    // na − the index of the first KS_CAP_KEEP arc the store does not hold, 0 none
    int bad_low;     // na − the index of the first held arc whose new capacity is below its lower bound, 0 none
    int n_add;       // listed, not held, cap > 0 (ADD_ARC)
    int n_upd;       // listed, held, another cost or capacity (UPDATE_ARC)
    int n_same;      // listed, held, the same cost and capacity
    int n_skip;      // listed, not held, cap == 0
    int n_zero;      // listed, held, cap == 0: deleted
    int n_del;       // held, unlisted, deleted
    int rec_held;    // the arc-slot scan's total: n_upd + n_zero + n_del
    int rec_add;     // the listed-arc scan's total: n_add
    int bad_range;   // batch ids: na − the index of the first arc whose head lies outside 1..span of its graph, 0 none
    int reserved[3];
};

// Inputs and scratch of one refresh (device pointers; nst node slots, hi arc slots).
struct NodDev {
    int k;                             // tails
    int na;                            // listed arcs
    int hi;                            // arc slots handed out when the call began
    int keep;                          // KS_NODES_KEEP_UNLISTED: nothing is deleted, no segment is walked
    const unsigned long long* nodes;   // [k] unchecked
    const unsigned long long* arc_off; // [k + 1] checked by the host: 0 first, never decreasing, na last
    const ks_node_arc* arcs;           // [na] costs, capacities and repeats checked by the host, heads unchecked
    long long nst;                     // node slots the passes may read
    int* n_own;                        // [nst + 1] per node slot: k − i of the first listing i of the tail, 0: not
                                       //   listed (claimed with atomicMax, so the array starts zeroed)
    int* n_slot;                       // [k + 1] node slot of tail i, −1: the id is refused
    int* nch;                          // [k + 1] 64-position chunks of a type-0 tail's segment, 0 for a resource
                                       //   tail and under keep; ch_off its scan
    int* ch_off;                       // [k + 1]
    int* l_slot;                       // [na + 1] 1 + the arc slot listed arc j names, 0: the store does not hold it
    int* lflag;                        // [na + 1] 1: listed arc j is an ADD_ARC; l_off its scan
    int* l_off;                        // [na + 1]
    int* sflag;                        // [hi + 1] NOD_* of the arc slot, 0: untouched; s_off the scan of its records
    int* s_off;                        // [hi + 1]
    const unsigned long long* hkey;    // the store's (src, dst) index (ks_store.h)
    const int* hval;
    int hmask;                         // capacity − 1, −1: no index yet
    NodCtl* ctl;
};

// The tail seed, one lane per id (liveness, type, the claim of n_own, n_slot, nch; walk: the id
// must lie in the built CSR, whose segments are walked), then the listed-arc pass, one lane per
// arc (the head against its tail's type, the index lookup, the table's row: l_slot, lflag, sflag
// and the counters). Nothing outside the scratch is written. The caller scans nch → ch_off when
// it walks.
hipError_t sched_nod_check(const SchedDev& d, const NodDev& u, bool walk, hipStream_t st);
// The held arcs of the type-0 tails that nobody listed, one wave per 64-position chunk item of
// their segments (ni_max bounds the items); an arc into a sink stays. The caller scans
// sflag → s_off (records only) and lflag → l_off.
hipError_t sched_nod_unlisted(const SchedDev& d, const NodDev& u, int ni_max, hipStream_t st);
// ctl->rec_held and ctl->rec_add after the scans.
hipError_t sched_nod_totals(const NodDev& u, hipStream_t st);
// The records on held arcs at s_off (ascending arc slot: the listed ones by their lane, the
// unlisted by the chunk items again), the ADD_ARC records at rec_held + l_off (input order);
// d: the arc table as it is now, after any growth.
hipError_t sched_nod_emit(const SchedDev& d, const NodDev& u, bool walk, int ni_max, int rec_held, ks_delta* recs,
                          hipStream_t st);

}  // namespace ks
