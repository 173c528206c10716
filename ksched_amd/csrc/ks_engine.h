// ks_engine.h — device engine of libksmcmf (gfx950). Internal to the library:
// the public boundary is include/ksmcmf.h.
//
// The engine owns the device-resident graph (ks_store.h: node store, arc table,
// hash index, residual CSR with slack), the solver state (excess,
// double-buffered prices, frontiers) and the control block the host polls
// between kernel batches. See DESIGN.md §3-§4 for the algorithm.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/ksmcmf.h"
#include "ks_store.h"

namespace ks {

struct EngineImpl;
struct CommitCtl;   // ks_sched.h

// A batch call's ids (ks_batch_add_tasks, ks_batch_complete_tasks, ks_batch_update_tasks,
// ks_batch_update_nodes): the lists of a union's graphs lie back to back. The task, tail and
// aggregator ids are already the
// union's (the host's O(k) part); the arcs' heads are still in each graph's own numbering and
// leave it on the device (sched_translate_heads). Messages name a node as its caller knows
// it: the graph and the graph-local id.
struct BatchView {
    size_t ng = 0;                        // graphs of this device's union
    const int64_t* off = nullptr;         // [ng + 1] graph i owns the union ids (off[i], off[i + 1]]
    const int* graph = nullptr;           // [ng] the caller's number of graph i
    const uint64_t* arc_goff = nullptr;   // [ng + 1] the first listed arc of graph i (calls with arcs)
    const uint64_t* node_goff = nullptr;  // [ng + 1] the first listed resource node of graph i (ks_batch_add_resources,
                                          //   whose node ids and edges are all graph-local: arc_goff counts its edges)
    uint64_t base_of(uint64_t id) const;  // the base of the graph that owns union id `id`
};
// "task 17" on a lone context, "graph 3: task 17" (graph-local) under a view; id: the context's own id.
std::string id_name(const BatchView* bv, const char* what, uint64_t id);

class Engine {
public:
    Engine();
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    int init(int device, const ks_opts& opts, std::string& err);

    // Replace the device store: node slots [0, nslots) (slot = NodeID − 1) with
    // their supply, DIMACS type and liveness, and the arcs (1-based ids, already
    // validated; a repeated (src, dst) pair: the last one wins).
    int load(int64_t nslots, const int64_t* supply, const uint8_t* type, const uint8_t* alive, const ks_arc* arcs,
             size_t m, std::string& err);

    // Apply a validated delta stream on the device (ks_store.h): the final state
    // of every node it touches plus the raw records; nslots = node slots in use.
    int apply(const NodeEdit* edits, size_t ne, const ks_delta* recs, size_t k, int64_t nslots, std::string& err);

    // The graph is a disjoint union of independent cells: cell i owns the node ids
    // (off[i], off[i+1]] (k + 1 offsets; no arc may cross two cells). Cells the cell
    // solver holds are then solved one workgroup each in ONE launch (ks_cell.h);
    // k = 0 forgets the partition (the whole graph is one cell).
    void set_cells(const int64_t* off, size_t k);
    // Deltas will follow the load (ks_batch_reserve): node slots [0, nslots) are in use from
    // now on (ids reserved past the highest loaded one) and the next build lays the
    // residual CSR out with an edited graph's slack, so the first stream lands in place.
    int expect_deltas(int64_t nslots, std::string& err);

    // Node state changes outside a stream (the auto-sink demand).
    int set_nodes(const NodeEdit* edits, size_t ne, std::string& err);

    // ε-scaling push-relabel to optimality on the device-resident graph, then
    // on-device verification. Fills r. warm: start from the flow and prices in
    // place (the previous solve's, edited by the deltas since).
    int solve(ks_result& r, bool warm, std::string& err);

    // Per-partition sums of the last solve for a disjoint union of graphs: graph i
    // owns node ids (off[i], off[i+1]]; cost[i] = Σ flow·cost over its arcs, flow[i] =
    // net inflow into its demand nodes. off has k+1 entries (host); outputs are
    // device pointers (k int64 each).
    int cell_sums(const int64_t* off, size_t k, int64_t* dev_cost, int64_t* dev_flow, std::string& err);
    hipStream_t stream() const;

    // Live arcs of the store (1-based ids), arc-slot order.
    int arcs(std::vector<ks_arc>& out, std::string& err);

    // Arcs with positive flow in the last solve (the "f" lines), arc-slot order.
    int flows(std::vector<ks_flow>& out, std::string& err);

    // Task → PU placement of the last solve, decomposed on device: for the i-th
    // live task slot in slot order, the node id of the last PU its flow unit
    // crosses, 0 when unscheduled. *count = n_tasks; dev_out (device memory,
    // ≥ n_tasks entries) may be null to query the count.
    int task_pu(uint64_t* dev_out, size_t cap, size_t* count, int64_t n_tasks, std::string& err);

    // Engine-owned device scratch of n uint64 (valid until the next call).
    int scratch(uint64_t** dev, size_t n, std::string& err);
    int download(void* host_dst, const void* dev_src, size_t bytes, std::string& err);

    int64_t live_arcs() const;
    bool solved() const;
    void store_stats(ks_store_stats* out) const;

    // Scheduler-side sweeps of a round (ks_sched.hip); see include/ksmcmf.h.
    int set_bindings(const uint64_t* task, const uint64_t* pu, size_t k, std::string& err);
    int sched_deltas(int commit, std::vector<ks_sched_delta>* out, size_t* count, int64_t n_tasks, std::string& err);
    int unsched_costs(const uint64_t* ids, size_t k, int mode, int64_t ucost, int64_t ccost, size_t* changed,
                      std::string& err);
    int topology_stats(uint64_t mtpp, const uint64_t* pu_ids, const uint64_t* pu_running, size_t k, int64_t sink_slot,
                       uint64_t* slots_below, uint64_t* running_below, std::string& err);
    // ks_commit_schedule: *out receives the deltas (cap: the caller's room for them);
    // sink_slot < 0: no single sink; kEverySink: a cell partition's sinks, one per cell (the
    // capacity refresh then starts from every live sink; refused without a partition).
    // *dirty: device state was touched before a failure.
    static constexpr int64_t kEverySink = -2;
    int commit_schedule(int flags, int64_t ccost, const uint64_t* ids, size_t k, int64_t sink_slot, int64_t n_tasks,
                        size_t cap, std::vector<ks_sched_delta>* out, size_t* count, ks_commit_stats* stats,
                        bool* dirty, std::string& err);
    // ks_commit_preemptive: the same contract; pcost: the preemption cost.
    int commit_preemptive(int flags, int64_t ccost, int64_t pcost, const uint64_t* ids, size_t k, int64_t sink_slot,
                          int64_t n_tasks, size_t cap, std::vector<ks_sched_delta>* out, size_t* count,
                          ks_preempt_stats* stats, bool* dirty, std::string& err);
    // ks_remove_resources (the subtree of the k roots, its evictions, the capacities of what
    // stays). probe: the counts only. Otherwise *removed receives the ids ascending and
    // *evicted the PREEMPTs; make_edits is called once with the removed ids, before anything
    // changes on the device: the host checks them against its node table, takes them out of
    // it and returns the node edits of the stream (a failure there changes nothing).
    using RemoveEdits = std::function<int(const uint64_t* ids, size_t n, std::vector<NodeEdit>* edits, std::string& err)>;
    int remove_resources(int flags, const uint64_t* roots, size_t k, int64_t sink_slot, bool probe, size_t rcap,
                         size_t ecap, std::vector<uint64_t>* removed, std::vector<ks_sched_delta>* evicted,
                         size_t* nremoved, size_t* nevicted, ks_remove_stats* stats, const RemoveEdits& make_edits,
                         bool* dirty, std::string& err, const BatchView* bv = nullptr);
    // ks_complete_tasks (the k task ids leave the graph; the aggregators' and, with the caps
    // flag, the resource arcs' capacities follow). left (k entries, may be null) receives the
    // bindings read before anything changes. make_edits is called once with the distinct ids
    // ascending, as in remove_resources. *changed: records were applied (the solution is
    // invalid); a call with k == 0 whose refresh finds every capacity right changes nothing.
    int complete_tasks(int flags, const uint64_t* tasks, size_t k, const uint64_t* unsched_ids, size_t nu,
                       int64_t sink_slot, uint64_t* left, ks_complete_stats* stats, const RemoveEdits& make_edits,
                       bool* dirty, bool* changed, std::string& err, const BatchView* bv = nullptr);
    // ks_add_tasks (the k new task ids, checked and already entered in the host's node table,
    // with their arcs; the aggregators gain a unit per task). nslots: the node slots in use
    // with the new ids. Every refusal is found before make_edits is called, once, for the node
    // edits of the stream (the host's aggregates move there); *dirty is set from then on.
    // sink_slot == kEverySink over a cell partition: every aggregator's record ends at the sink
    // of its own cell. bv: the arcs' heads are graph-local (BatchView), also in update_tasks.
    using AddEdits = std::function<void(std::vector<NodeEdit>* edits)>;
    int add_tasks(const uint64_t* tasks, size_t k, const uint64_t* arc_off, const ks_task_arc* arcs,
                  const uint64_t* unsched_ids, size_t nu, int64_t sink_slot, int64_t sink_cost, int64_t nslots,
                  ks_add_stats* stats, const AddEdits& make_edits, bool* dirty, std::string& err,
                  const BatchView* bv = nullptr);
    // ks_add_resources (the n new resource nodes, checked and already entered in the host's node
    // table, and the m edges; first_pair: the first edge that repeats an earlier (parent, child),
    // m when none does). make_edits and *dirty as in add_tasks; *changed: records were applied.
    // sink_slot == kEverySink over a cell partition: every new PU's arc ends at the sink of its own
    // cell. bv: the node ids and the edges' endpoints are graph-local (BatchView::node_goff).
    int add_resources(const ks_res_node* nodes, size_t n, const ks_res_arc* arcs, size_t m, size_t first_pair,
                      int64_t sink_slot, int64_t nslots, ks_grow_stats* stats, const AddEdits& make_edits, bool* dirty,
                      bool* changed, std::string& err, const BatchView* bv = nullptr);
    // ks_update_tasks (the k live task ids with the arcs each should have; offsets checked by the
    // caller). first_pair: the first arc that repeats an earlier head of its own task, arc_off[k]
    // when none does. No node is edited. *dirty: records were emitted (a failure from then on
    // leaves the device state unknown); *changed: records were applied.
    int update_tasks(int flags, const uint64_t* tasks, size_t k, const uint64_t* arc_off, const ks_task_arc* arcs,
                     size_t first_pair, const uint64_t* unsched_ids, size_t nu, int64_t sink_slot, int64_t sink_cost,
                     ks_update_stats* stats, bool* dirty, bool* changed, std::string& err,
                     const BatchView* bv = nullptr);
    // ks_update_nodes (the k tails with the arcs each should have; offsets checked by the caller).
    // first_pair, first_cost, first_cap: the first arc that repeats an earlier head of its own
    // tail, whose cost and whose capacity is out of range, arc_off[k] when none does or is. No
    // node is edited. *dirty, *changed: as in update_tasks. bv: the tails are the union's, the
    // arcs' heads are graph-local (BatchView).
    int update_nodes(int flags, const uint64_t* nodes, size_t k, const uint64_t* arc_off, const ks_node_arc* arcs,
                     size_t first_pair, size_t first_cost, size_t first_cap, ks_node_stats* stats, bool* dirty,
                     bool* changed, std::string& err, const BatchView* bv = nullptr);
    // ks_get_bindings: pu[i] = the device-kept binding of task[i] (ids checked by the caller).
    int get_bindings(const uint64_t* task, uint64_t* pu, size_t k, std::string& err);
    int device() const;

private:
    // the body of both commits (ks_engine_sched.hip); *h: the device counters of the call
    int commit(bool preempt, int flags, int64_t ccost, int64_t pcost, const uint64_t* ids, size_t k, int64_t sink_slot,
               int64_t n_tasks, size_t cap, std::vector<ks_sched_delta>* out, size_t* count, CommitCtl* h,
               bool* dirty, std::string& err);
    EngineImpl* p_;
};

}  // namespace ks
