/*
 * ksmcmf.h — C-ABI of the MI355X-native min-cost max-flow solver that replaces
 * ksched's Flowlessly round-trip (the `placement.Solver` hot path).
 *
 * What each entry point replaces in the reference (paths relative to the
 * ksched tree, scheduling/flow/…):
 *
 *   ks_create / ks_destroy   placement/solver.go:49-55 NewSolver, :92-109 startSolver
 *                            (the exec'd flow_scheduler child becomes a device context)
 *   ks_load_graph            placement/solver.go:111-116 writeGraph → dimacs/export.go:11-29
 *                            (full "p/n/a" DIMACS text export becomes an array upload)
 *   ks_apply_deltas          placement/solver.go:118-123 writeIncremental →
 *                            dimacs/export.go:31-38 + the GenerateChange methods of
 *                            dimacs/{add_node,create_arc,update_arc,remove_node}_change.go
 *                            — validated on the host, applied IN PLACE on the device:
 *                            the graph (arc table, (src, dst) hash index, residual
 *                            CSR with slack) stays resident in HBM between rounds; a
 *                            stream is all-or-nothing (an invalid record applies none)
 *   ks_coalesce_deltas       the change optimisers graph_change_manager.go:220-279
 *                            (optimizeChanges: RemoveDuplicate, MergeToSameArc,
 *                            PurgeBeforeNodeRemoval — declared there, never implemented)
 *   ks_solve                 the external Flowlessly solve (solver.go:30-34, Dockerfile:10-12)
 *                            — min-cost flow, bit-exact total cost and flow value
 *   ks_get_flows             the "f src dst flow" lines read by readFlowGraph
 *                            (placement/solver.go:134-179); only arcs with flow > 0
 *   ks_get_task_mapping      parseFlowToMapping + addPUToSourceNodes
 *                            (placement/solver.go:183-269) → flowmanager.TaskMapping
 *                            (flowmanager/types.go:6)
 *   ks_commit_schedule       TaskScheduled → pinTaskToNode and capacityFromResNodeToParent
 *                            (flowmanager/graph_manager.go:454-460, 675-720, 662-667) and the
 *                            change records they would log, generated and applied on device
 *   ks_commit_preemptive     the same step with Preemption == true: TaskScheduled →
 *                            updateArcsForScheduledTask (graph_manager.go:855-888) with
 *                            updateRunningTaskToUnscheduledAggArc (:1164-1181), TaskEvicted
 *                            (:412-433), TaskMigrated (:407-410) and capacityFromResNodeToParent
 *                            returning NumSlotsBelow (:662-667)
 *   ks_remove_resources      DeregisterResource (flowscheduler/scheduler.go:162-210): dfsEvictTasks
 *                            (:533-566) → TaskEvicted, RemoveResourceTopology (:362-387) with
 *                            traverseAndRemoveTopology (graph_manager.go:829-844) and the
 *                            ancestors' capacities, generated and applied on device
 *   ks_complete_tasks        HandleTaskCompletion (flowscheduler/scheduler.go:106-132) →
 *                            TaskCompleted (graph_manager.go:389-405) → removeTaskNode
 *                            (:803-813) and updateUnscheduledAggNode(−1) (:1291-1305); also
 *                            TaskFailed / TaskKilled (:435-452), generated and applied on device
 *   ks_update_tasks          UpdateTimeDependentCosts (graph_manager.go:211-213) → updateTaskNode
 *                            (:1183-1192) for tasks that have their node: arcs added, re-costed
 *                            and dropped as the cost model lists them, generated and applied on
 *                            device
 *   ks_update_nodes          the rest of that sweep, updateFlowGraph (graph_manager.go:1012-1033):
 *                            updateEquivClassNode (:931-1010) and updateResourceNode →
 *                            updateResOutgoingArcs (:1094-1111), updateResToSinkArc (:1116-1129):
 *                            class and resource arcs added, re-costed, re-sized and dropped,
 *                            generated and applied on device
 *   ks_get_bindings          the TaskBindings the device keeps (ks_set_bindings, the commits)
 *   ks_last_error           the panics of solver.go:97-108, 148-153, 175-178, 223-225
 *                            become status codes + a message
 *
 * Semantics (flowgraph/graph.go:25-41, arc.go:26-36, node.go:76-106):
 *   - node ids are ksched NodeIDs (dense from 1, reused FIFO after removal,
 *     graph.go:169-182); excess is the node supply (tasks +1, sink −#tasks);
 *     type is the DIMACS node type code of export.go:56-68 (task 1, PU 2,
 *     sink 3, machine 4, numa/socket/cache/core 5, other 0).
 *   - arcs are (src, dst, low, cap, cost, type); at most one arc per ordered
 *     (src, dst) pair (node.go:118-131). ADD_ARC on an existing pair upserts.
 *   - UPDATE_ARC with low == cap == 0 REMOVES the arc (DeleteArc emits this
 *     record, graph_change_manager.go:184-193; ChangeArc to 0/0, :142-156, keeps
 *     a zero-capacity arc in the reference, which carries no flow either, so the
 *     two are equivalent for the solve). A later ADD_ARC / UPDATE_ARC re-creates
 *     it. The arc then no longer counts in n_arcs.
 *   - REMOVE_NODE drops every incident arc implicitly (the reference emits only
 *     "r id", graph_change_manager.go:129-139); the id may be reused later.
 *   - SET_EXCESS sets a node's supply explicitly (the sink's demand drifts in
 *     the reference without a message: graph_manager.go:640, 808). With
 *     ks_opts.auto_sink != 0 (default) the sink's demand is recomputed as
 *     −Σ(other supplies) at every solve, which is what keeps an incremental
 *     DIMACS stream balanced.
 *
 * Ownership: input arrays belong to the caller and are copied during the call.
 * Output buffers are caller-allocated; call with cap = 0 to get the count.
 * One context per thread; calls on one context are not reentrant
 * (placement/solver.go:59). Contexts on different devices may run concurrently.
 */
#ifndef KSMCMF_H
#define KSMCMF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSMCMF_ABI_VERSION 5   /* 2: ks_opts tuning fields, ks_result.recoveries, batch layout calls;
                                  3: ks_opts.cell_nodes, ks_result per-kind timing and cell-solver
                                  fields; 4: ks_opts.compact_pos (the last reserved word of
                                  ks_opts), and three words of ks_result repurposed:
                                  cell_fallbacks and cycles_cancelled (two reserved words)
                                  and compact (the former _pad3); 5: ks_result.fb_resets
                                  (the last reserved word), ks_result.cycles_rejected and
                                  gu_leaf_scans; ks_result grew to 352 B (2 reserved words);
                                  Batch rounds (still 5: entry points were only added and
                                  no struct changed size or moved a field, so a caller
                                  built against ABI 5 keeps working) — ks_batch_reserve,
                                  ks_batch_apply_deltas,
                                  ks_batch_get_graph, ks_batch_set_bindings, both
                                  ks_batch_commit_* calls, the layout helpers
                                  ks_batch_node_offsets / ks_batch_translate_deltas, and
                                  ks_result.cells_run (half of a reserved word: the struct
                                  keeps its size). ks_remove_resources (still 5: an
                                  entry point and its stats struct were added).
                                  ks_complete_tasks and ks_get_bindings (still 5: two
                                  entry points and one stats struct were added).
                                  ks_add_tasks (still 5: one entry point and two structs
                                  were added, nothing was resized).
                                  ks_add_resources (still 5: one entry point and three
                                  structs were added).
                                  ks_update_tasks (still 5: one entry point and one
                                  struct were added, nothing was resized).
                                  ks_update_nodes (still 5: one entry point and two
                                  structs were added, nothing was resized).
                                  ks_batch_update_nodes (still 5: one entry point and one
                                  struct were added, nothing was resized).
                                  ks_opts (96 B) CHANGED SIZE in ABI 2 and ks_result in
                                  ABI 2, 3 and 5: a caller must check
                                  ks_abi_version() == KSMCMF_ABI_VERSION before ks_create. */

/* status codes (0 = OK) */
#define KS_OK            0
#define KS_E_INVALID    (-1)  /* bad argument / malformed graph or delta          */
#define KS_E_INFEASIBLE (-2)  /* supplies cannot be routed to the demands         */
#define KS_E_DEVICE     (-3)  /* HIP runtime error or device not available        */
#define KS_E_VERIFY     (-4)  /* on-device verification of the result failed      */
#define KS_E_RANGE      (-5)  /* value outside the solver's integer range         */

/* DIMACS node-type codes (dimacs/add_node_change.go:27-36, export.go:56-68) */
#define KS_NODE_OTHER    0
#define KS_NODE_TASK     1
#define KS_NODE_PU       2
#define KS_NODE_SINK     3
#define KS_NODE_MACHINE  4
#define KS_NODE_INTERMEDIATE 5

typedef struct ks_ctx ks_ctx;

typedef struct ks_opts {
    int32_t  alpha;            /* cost-scaling factor per ε-phase; 0 (ks_default_opts):
                                  8, or 32 for graphs under 32,768 nodes on the
                                  multi-kernel engine                                   */
    int32_t  verify;           /* run the on-device verifier after every solve (1)      */
    int32_t  auto_sink;        /* sink demand = −Σ other supplies at solve time (1)     */
    int32_t  price_refine;     /* certify optimality early [1]: 1 — the phase before the
                                  final one drains, then price refinement cancels the
                                  negative cycles it meets until it certifies the flow
                                  (the final phase runs only if it gives up); 2 — the
                                  final phase, then plain price refinement; 0 — off    */
    int32_t  gu_interval;      /* sweeps between global price updates (default 24)      */
    int32_t  warm_start;       /* 1: re-solve from the previous flow and prices after
                                  ks_apply_deltas (the first phase saturates only the
                                  arcs violating its ε); 2: every phase does; 0
                                  (default): every solve from scratch  */
    /* solver tuning; 0 selects the library default given in brackets.
       None of these changes the result — only how fast it is reached. */
    int32_t  walk_slack;       /* a phase's tail walkers take residual arcs of reduced cost
                                  ≤ walk_slack·ε toward a smaller distance while ε > 1
                                  [4]; < 0 disables the walkers                       */
    int32_t  final_div;        /* the phase price refinement certifies runs at 1/final_div
                                  of a cost unit [20 for cells and graphs under 32,768
                                  nodes, else 24 with the cycle-cancelling finish
                                  (price_refine 1) and 48 without]; < 0: the plain
                                  max|cost|/α^k ladder                                  */
    int32_t  pr_rounds;        /* Bellman-Ford rounds one price refinement may take [160] */
    int32_t  phase_exit;       /* a coarse phase ends once ≤ phase_exit nodes hold excess
                                  [256] ... */
    int32_t  phase_frac;       /* ... and ≤ 1/phase_frac of the phase's peak [128]; < 0 in
                                  phase_exit: coarse phases always drain completely   */
    int32_t  tail_sweeps;      /* sweeps per cycle once ≤ 64 nodes hold excess [4]      */
    int32_t  bf_margin;        /* Bellman-Ford rounds enqueued per cycle beyond the last
                                  update's count [6]                                    */
    int32_t  two_hop;          /* hops one Bellman-Ford launch covers. 1: a task's / PU's
                                  in-arcs are relaxed in the round its distance dropped
                                  (two hops). 2: the continuation — a 16-, 32- or 64-lane
                                  class node (a machine) lowered by that second hop is
                                  relaxed, and the tasks it lowers expanded, by the same
                                  workgroup before it retires (four hops; a workgroup-
                                  local LDS queue, overflow falls back to the frontier
                                  flag). < 0: one hop. [2]                              */
    int32_t  log_cycles;       /* 1: one diagnostic line per update cycle on stderr [0] */
    int32_t  fault_inject;     /* TESTS ONLY [0]: bit 0 — the last phase's walks use the
                                  coarse slack at ε = 1 (may end non-1-optimal); bit 1 —
                                  the final prices are perturbed before verification.
                                  Both must be repaired by the certificate recovery.
                                  Bit 2 (ks_batch_create*): global rank 0 fails to pack
                                  its rows in ks_batch_gather (every rank must still
                                  reach the collective and return the error). Bit 3
                                  (ks_batch_create*): rank 0's receive buffer
                                  allocation fails in ks_batch_gather (the same).
                                  Bit 4 (ks_batch_create*): the middle cell of the
                                  batch gives up in the cell solver and is re-solved
                                  on the engine; the result then reports solver 1,
                                  cells = the batch's cells, warm_started 1 (the
                                  other cells' optima are carried), cell_fallbacks 1
                                  and fb_resets. Bit 5: the cycle-cancelling finish gives
                                  up after its first batch (the final phase runs).
                                  Bit 6: one unit is moved on an arc after the solve
                                  without its endpoints' excess (the verifier's
                                  conservation check must fail: KS_E_VERIFY).
                                  Bit 7: every parent-graph search of the finish
                                  doubles only 5 steps (a 32-node window, shorter than
                                  the parent chains: their nodes are marked and meet
                                  cycles, and the union-of-cycles test must reject
                                  them — cycles_rejected). Bit 8 (engine): that test
                                  only counts, rejecting nothing (with bit 7 a chain
                                  is pushed along: the verifier must then fail the
                                  solve with KS_E_VERIFY, never return a wrong cost).
                                  Bit 9 (engine, two_hop 2): the continuation queue
                                  holds 2 entries, so almost every enqueue takes the
                                  overflow path (the frontier flag).                    */
    int32_t  walk_passes;      /* tail walker passes from the update's excess nodes per
                                  cycle [1]; later passes retry units left short        */
    int32_t  tail_nodes;       /* a phase's tail — walks over each update, few sweeps —
                                  starts once ≤ tail_nodes nodes hold excess [64]; at
                                  most 4096                                             */
    int32_t  bf_bound;         /* a global update with ≤ 64 excess nodes drops Bellman-Ford
                                  offers at or above the largest tentative distance of
                                  those nodes and caps prices there [on]; < 0 off       */
    int32_t  fwd_nodes;        /* in a coarse phase (one a finer phase follows), once
                                  ≤ fwd_nodes nodes hold excess, a cycle searches from them
                                  to the nearest deficit and pushes along the search's
                                  shortest paths instead of a global update [32 below
                                  32,768 nodes, else 64]; a search
                                  whose frontier grows past n/4 nodes, or that runs longer
                                  than twice the last global update's rounds, costs ONE
                                  global update and the next cycle searches forward again.
                                  The last phase always uses global updates. < 0 off      */
    int32_t  cell_nodes;       /* the cell solver (one workgroup per graph)
                                  solves every graph — or every cell of a ks_batch union —
                                  of at most cell_nodes node slots [0: a ks_batch cell up
                                  to what its LDS holds (13,1xx), a lone graph up to 4,096
                                  (larger ones solve sooner on the whole chip)]; < 0:
                                  always the multi-kernel engine                          */
    int32_t  warm_shift;       /* warm start: a node whose flow-carrying out-arc got dearer
                                  since the last solve (ksched's ageing of unscheduled
                                  arcs) is priced down by the rise, so that arc keeps its
                                  reduced cost [0: on]; < 0 off                          */
    int32_t  warm_canon;       /* warm start: each solve ends by replacing its prices with
                                  the flow's canonical ones (a Bellman-Ford at ε = 1 from
                                  d = p), so carried prices do not drift [0: on]; < 0 off.
                                  Multi-kernel engine only: a cell-solver solve keeps the
                                  prices its workgroup ended with                      */
    int32_t  compact_pos;      /* the multi-kernel engine's solve reads 16-byte residual
                                  records (32-bit residual, pair capacity, scaled cost,
                                  head) when every scaled cost and capacity fits, else
                                  the 32-byte ones [0: on]; < 0: always 32-byte (ABI 4)  */
} ks_opts;

typedef struct ks_node {       /* one "n id excess type" line                            */
    uint64_t id;
    int64_t  excess;
    int32_t  type;
    int32_t  _pad;
} ks_node;

typedef struct ks_arc {        /* one "a src dst low cap cost [type]" line               */
    uint64_t src, dst;
    uint64_t low, cap;
    int64_t  cost;
    int32_t  type;             /* flowgraph.ArcType: 0 other, 1 running (arc.go:18-23)   */
    int32_t  _pad;
} ks_arc;

enum ks_delta_kind {
    KS_ADD_NODE    = 0,        /* "n id excess type"                                     */
    KS_REMOVE_NODE = 1,        /* "r id"                                                 */
    KS_ADD_ARC     = 2,        /* "a src dst low cap cost type" (upsert)                 */
    KS_UPDATE_ARC  = 3,        /* "x src dst low cap cost type oldcost"                  */
    KS_SET_EXCESS  = 4         /* explicit supply change (sink drift)                    */
};

typedef struct ks_delta {
    int32_t  kind;             /* enum ks_delta_kind                                     */
    int32_t  type;             /* node type (ADD_NODE) or arc type (ADD/UPDATE_ARC)      */
    uint64_t id;               /* node id (ADD_NODE, REMOVE_NODE, SET_EXCESS)            */
    uint64_t src, dst;         /* arc endpoints (ADD_ARC, UPDATE_ARC)                    */
    uint64_t low, cap;
    int64_t  cost;
    int64_t  old_cost;         /* UPDATE_ARC only (informational, as in the "x" line)    */
    int64_t  excess;           /* ADD_NODE, SET_EXCESS                                   */
} ks_delta;

#define KS_N_PHASE_TIMERS 6    /* build, saturate, cycles, price-refine, verify, total   */

typedef struct ks_result {
    int64_t  total_cost;       /* Σ flow·cost over all arcs (lower bounds included)      */
    int64_t  flow_value;       /* units routed from supply nodes to demand nodes         */
    int32_t  status;           /* same code as the ks_solve return value                 */
    int32_t  phases;           /* ε-phases executed                                      */
    uint64_t sweeps;           /* push/relabel sweep kernels that did work               */
    uint64_t arc_scans;        /* residual-arc scans (device counter)                    */
    uint64_t node_visits;      /* active-node discharges (device counter)                */
    uint64_t pushes;
    uint64_t relabels;
    uint64_t global_updates;
    uint64_t gu_iterations;    /* Bellman-Ford rounds that did work (updates+refinement) */
    uint64_t gu_arc_scans;     /* in-arc relaxations inside Bellman-Ford rounds          */
    double   ms_phase[KS_N_PHASE_TIMERS];
    int64_t  n_nodes;          /* node slots on device                                   */
    int64_t  n_arcs;           /* live input arcs                                        */
    uint64_t sweep_launches;   /* push/relabel sweep kernel launches (incl. early exits) */
    double   ms_sweep_kernels; /* HIP-event-timed span of all sweep batches (ms)         */
    uint64_t gu_launches;      /* Bellman-Ford round launches (price updates, refinement)*/
    double   ms_gu_kernels;    /* HIP-event-timed span of all Bellman-Ford batches (ms)  */
    int32_t  warm_started;     /* 1 when this solve started from the previous solution   */
    int32_t  rebuilt;          /* 1 when this solve rebuilt the residual CSR from the arc
                                  table (after a load, or a delta that did not fit)     */
    int32_t  recoveries;       /* times the final optimality certificate failed and was
                                  repaired (price refinement, else one more ε = 1 phase
                                  from the current flow) before the solve returned      */
    int32_t  solver;           /* 0: multi-kernel engine; 1: cell solver (ABI 3)         */
    /* ABI 3. Per-kind device time: each span starts at an event recorded right before
       its first kernel and ends at one right after its last (no host gap inside).
       ms_gu_kernels / gu_launches: the backward Bellman-Ford rounds (global updates,
       price refinement); ms_sweep_kernels / sweep_launches: the sweep bursts;
       forward tail updates (k_fs_*) are their own kind:                               */
    uint64_t fs_launches;      /* forward search rounds launched (k_fs_round)           */
    double   ms_fs_kernels;    /* event-timed span of the forward-update batches (ms)   */
    uint64_t fwd_updates;      /* forward tail updates completed                        */
    int32_t  cells;            /* cells the cell solver ran (one workgroup each)        */
    int32_t  compact;          /* 1: the engine's solve read 16-byte residual records   */
    double   ms_cell_kernel;   /* event-timed duration of the cell-solver launches (ms) */
    uint64_t cell_ticks_max;   /* slowest cell's in-kernel solve time (100 MHz ticks)   */
    uint64_t cell_ticks_sum;   /* Σ over cells of their in-kernel solve times            */
    uint64_t fs_arc_scans;     /* residual out-arcs the forward tail searches examined    */
    uint64_t cell_fallbacks;   /* cells of this solve that did not converge in the cell
                                  solver (step cap or wall-clock limit) and were re-solved
                                  on the multi-kernel engine, the other cells' optima
                                  kept (the status stays KS_OK)                         */
    uint64_t cycles_cancelled; /* negative cycles the cycle-cancelling finish cancelled
                                  (ks_opts.price_refine 1)                  */
    uint64_t fb_resets;        /* ABI 5. A per-cell fallback solve: live arc slots plus
                                  node slots of the failing cells whose carried flow /
                                  price it reset (they restart cold; 0 otherwise)      */
    uint64_t cycles_rejected;  /* ABI 5. The finish's parent-graph searches: marked nodes
                                  the union-of-cycles test found with other than one
                                  member pointing at them (engine), or leader walks
                                  that did not close a cycle (cell solver)            */
    uint64_t gu_leaf_scans;    /* ABI 5. Bellman-Ford rounds also relax the in-arcs of a task
                                  or PU whose distance just dropped, in the same round
                                  (two hops per round): those second-hop in-arc positions
                                  examined (gu_arc_scans counts the first hop only)      */
    int32_t  cells_run;        /* Batch rounds. Cells the cell solver launched in this solve: with
                                  ks_opts.warm_start >= 1 a cell of a ks_batch union that no
                                  record touched since its last solve is skipped (its flow,
                                  prices and rows stay as they were); cells stays the
                                  partition size                                         */
    int32_t  reserved4;
    uint64_t reserved3[1];
} ks_result;

/* Counters of the device-resident graph store (ks_get_store_stats). */
typedef struct ks_store_stats {
    int64_t  live_arcs;        /* arcs in the store                                      */
    int64_t  inserted;         /* last ks_apply_deltas: arcs inserted in place           */
    int64_t  updated;          /*   arcs whose bounds / cost were edited in place        */
    int64_t  killed;           /*   arcs removed (UPDATE 0/0 or an endpoint removed)     */
    int64_t  superseded;       /*   records overridden by a later record for the arc     */
    int64_t  rebuilds;         /* CSR rebuilds since ks_load_graph (1 = the load's own)  */
    int64_t  residual_slots;   /* residual positions allocated (live pairs + slack)      */
    int64_t  reserved[4];
} ks_store_stats;

typedef struct ks_flow {       /* one "f src dst flow" line                              */
    uint64_t src, dst;
    int64_t  flow;
} ks_flow;

int         ks_abi_version(void);
void        ks_default_opts(ks_opts* opts);
ks_ctx*     ks_create(int device, const ks_opts* opts);
void        ks_destroy(ks_ctx* ctx);
const char* ks_last_error(ks_ctx* ctx);

/* Replace the whole graph (first Solve: solver.go:63-83).
 *
 * Value ranges (checked here and, record by record, in ks_apply_deltas; a value
 * outside them is KS_E_RANGE and leaves the context, host and device, as it was):
 *   cost      |cost| <= 2^40, either sign; negative-cost cycles are legal input
 *   capacity  low <= cap <= 2^53
 *   node ids  1 .. 2^30 - 1
 *   excess    any int64; it is not range-checked, but a supply that the capacities
 *             cannot carry makes the solve KS_E_INFEASIBLE, and the sum of the
 *             supplies (the flow value) must fit int64
 * Two more limits depend on the whole graph and are checked by ks_solve (below). */
int ks_load_graph(ks_ctx* ctx, const ks_node* nodes, size_t n,
                  const ks_arc* arcs, size_t m);

/* Apply a delta stream in mutation order (later Solves: solver.go:86-88). */
int ks_apply_deltas(ks_ctx* ctx, const ks_delta* deltas, size_t k);

/* Shrink a delta stream without changing what ks_apply_deltas makes of it
 * (graph_change_manager.go:220-279): per arc only its last ADD/UPDATE record
 * survives (both are upserts; UPDATE 0/0 deletes); arc and SET_EXCESS records
 * touching a node before its REMOVE_NODE are dropped; per node only the last
 * SET_EXCESS survives. ADD_NODE / REMOVE_NODE records are kept; survivors keep
 * their order. Host-only (no context, no device). Writes at most `cap` records
 * to `out` (out == in allowed), *count = surviving records. KS_E_INVALID on a
 * zero or out-of-range node id. Validation errors a dropped record would have
 * raised in ks_apply_deltas are not reported. */
int ks_coalesce_deltas(const ks_delta* in, size_t k, ks_delta* out, size_t cap, size_t* count);

/* Solve min-cost flow on the current graph. result may be NULL.
 *
 * Solve-time ranges (KS_E_RANGE from ks_solve; the graph stays loaded, and deltas
 * that bring it into range make the next solve succeed):
 *   scaled prices  costs are multiplied by mult = N + 1, N the node-slot count (the
 *                  highest node id in use, ks_result.n_nodes, plus max(64, N/16) spare
 *                  slots once deltas have been applied), and prices stay within
 *                  int64 only while  max|cost| * mult^2 * 8 <= 4e18:
 *                  max|cost| ~ 5e17 / (highest id)^2. Sparse ids count in full: ids up
 *                  to 4,000 allow max|cost| = 31,234,380,857, ids up to 10^6 about 5e5.
 *   total cost     total_cost is exact whenever the sum over all arcs of |flow * cost|
 *                  is below 2^63. Otherwise ks_solve returns KS_E_RANGE and
 *                  ks_last_error names the sum; it never returns KS_OK with a wrapped
 *                  number. (The same bound covers every partial sum, so the per-graph
 *                  costs of ks_batch_gather are exact whenever the union's solve is.)
 * Inside those limits which solver ran (the cell solver, the engine on 16- or 32-byte
 * positions: ks_result.solver, .compact) depends on the values, the answer does not. */
int ks_solve(ks_ctx* ctx, ks_result* result);

/* Solve k independent contexts concurrently (config 5: cluster cells /
 * what-if graphs). `workers` host threads (0 = min(k, 4)) each take the next
 * unsolved context and call ks_solve on it; contexts on one device run on
 * their own streams and overlap on the GPU. results[i] (may be NULL) receives
 * context i's result. Returns KS_OK, or the status of the first failing
 * context in index order (the others still ran). No reference counterpart:
 * ksched solves one graph per round (flowscheduler/scheduler.go:350). */
int ks_solve_many(ks_ctx* const* ctxs, size_t k, int workers, ks_result* results);

/* Arcs with positive flow from the last solve (the "f" lines). */
int ks_get_flows(ks_ctx* ctx, ks_flow* out, size_t cap, size_t* count);

/* task NodeID → PU NodeID for every task whose unit reaches a PU (TaskMapping).
 * The flow is decomposed on the device: each task's unit is followed along
 * positive-flow arcs (units numbered per node in arc order) to the sink, and
 * the last PU on the way is its placement. */
int ks_get_task_mapping(ks_ctx* ctx, uint64_t* task, uint64_t* pu,
                        size_t cap, size_t* count);

/* Device-resident mapping for RCCL gathers: for the i-th task node in id order
 * writes the PU node id it maps to, or 0 when unscheduled, computed on device
 * (nothing crosses PCIe). dev_out is a device pointer with room for `cap`
 * uint64 (KS_E_INVALID when cap < the task count); dev_out = NULL only sets
 * *count, the number of task nodes. */
int ks_get_task_pu_device(ks_ctx* ctx, uint64_t* dev_out, size_t cap, size_t* count);

/* The device-resident graph as it stands (the reference's dimacs.Export view,
 * export.go:11-29, e.g. for a checkpoint or a DIMACS dump): live nodes in id order
 * and live arcs in arc-slot order. A node's excess is the supply last stated for it
 * (ks_load_graph, ADD_NODE, SET_EXCESS): the sink's demand that auto_sink recomputes
 * at solve time is not written back. Call with caps of 0 to size. */
int ks_get_graph(ks_ctx* ctx, ks_node* nodes, size_t ncap, size_t* n, ks_arc* arcs, size_t acap, size_t* m);

/* Store counters (no device work). */
int ks_get_store_stats(ks_ctx* ctx, ks_store_stats* out);

/* ---- scheduler-side sweeps of a round, on the device-resident graph ------- */

/* pb.SchedulingDelta_ChangeType (proto/scheduling_delta.proto:11-16) */
#define KS_DELTA_PLACE   0
#define KS_DELTA_PREEMPT 1
#define KS_DELTA_MIGRATE 2
#define KS_DELTA_NOOP    3

typedef struct ks_sched_delta {
    int32_t  type;             /* KS_DELTA_*                                             */
    int32_t  _pad;
    uint64_t task;             /* task NodeID                                            */
    uint64_t pu;               /* PU NodeID (PLACE / MIGRATE: the new one; PREEMPT: the
                                  one it leaves)                                         */
} ks_sched_delta;

/* Seed the device-kept task bindings (TaskBindings, flowscheduler/scheduler.go:421-437):
 * task NodeID → bound PU NodeID (0 = unbind). A REMOVE_NODE of a task unbinds it. */
int ks_set_bindings(ks_ctx* ctx, const uint64_t* task, const uint64_t* pu, size_t k);

/* Scheduling deltas of the last solve against the bindings, on device:
 * SchedulingDeltasForPreemptedTasks (graph_manager.go:297-339) — a bound task absent
 * from the mapping → PREEMPT, emitted first — then NodeBindingToSchedulingDelta
 * (:253-295) per mapped task: unbound → PLACE, bound elsewhere → MIGRATE, bound here
 * → nothing; each in task-id order. Every destination must be a PU (:259-262),
 * else KS_E_VERIFY. commit != 0 applies the deltas to the bindings
 * (applySchedulingDeltas, scheduler.go:377-412). out == NULL: *count only, nothing
 * committed; otherwise cap ≥ the count is required (KS_E_INVALID, nothing committed). */
int ks_scheduling_deltas(ks_ctx* ctx, int commit, ks_sched_delta* out, size_t cap, size_t* count);

#define KS_COST_SET 0
#define KS_COST_ADD 1

/* UpdateAllCostsToUnscheduledAggs (graph_manager.go:462-475, called by Solve before
 * every incremental export, solver.go:86) on device, in place: for every task with
 * an arc into an unscheduled aggregator, a running task (it has a running arc,
 * type 1) gets its running arc set to continuation_cost (TaskContinuationCost),
 * any other task its arc to the aggregator set to (KS_COST_SET) or raised by
 * (KS_COST_ADD: waiting-time ageing) unsched_cost (TaskToUnscheduledAggCost).
 * Aggregators: unsched_ids (k of them), or with unsched_ids == NULL every type-0
 * node with an arc into the sink. *changed (may be NULL) = arcs whose cost changed. */
int ks_update_unsched_costs(ks_ctx* ctx, const uint64_t* unsched_ids, size_t k, int32_t mode,
                            int64_t unsched_cost, int64_t continuation_cost, size_t* changed);

/* ComputeTopologyStatistics (graph_manager.go:480-511; trivial model PrepareStats /
 * GatherStats, costmodel/trivial_cost_modeler.go:147-176) on device: BFS from the
 * sink over in-arcs; a PU takes (len(CurrentRunningTasks), max_tasks_per_pu), every
 * resource node above sums its children. CurrentRunningTasks lengths: pu_running[i]
 * for PU pu_ids[i] (k of them), or with pu_ids == NULL the running arcs (type 1)
 * into each PU. Writes slots_below[id-1] / running_below[id-1] for ids 1..*count
 * (0 for nodes that are not resources); cap < *count → KS_E_INVALID. */
int ks_topology_stats(ks_ctx* ctx, uint64_t max_tasks_per_pu, const uint64_t* pu_ids,
                      const uint64_t* pu_running, size_t k, uint64_t* slots_below,
                      uint64_t* running_below, size_t cap, size_t* count);

#define KS_COMMIT_RESOURCE_CAPS 1   /* also refresh resource-arc capacities (below) */

typedef struct ks_commit_stats {
    int64_t placed;            /* PLACE deltas pinned                                  */
    int64_t arcs_removed;      /* task out-arcs deleted                                */
    int64_t running_added;     /* new task→PU running arcs                             */
    int64_t running_converted; /* existing task→PU arcs turned into running arcs       */
    int64_t unsched_updates;   /* aggregator→sink arcs whose capacity changed          */
    int64_t cap_updates;       /* resource arcs whose capacity changed                 */
    int64_t records;           /* delta records generated on device and applied        */
    int64_t reserved[5];
} ks_commit_stats;

/* The graph edit that follows applySchedulingDeltas with Preemption == false, on device:
 * TaskScheduled → updateArcsForScheduledTask → pinTaskToNode (graph_manager.go:454-460,
 * 855-859, 675-720), updateUnscheduledAggNode(−1) (:706, :1291-1305) and, with
 * KS_COMMIT_RESOURCE_CAPS, capacityFromResNodeToParent (:662-667) after a
 * ComputeTopologyStatistics pass. The records a host would export for it (about six
 * per placed task) are generated in device memory and applied as ONE stream with the
 * semantics of ks_apply_deltas (all or nothing, in place, store counters, warm-start
 * bookkeeping; no (src, dst) twice, so superseded is 0); nothing but the deltas
 * crosses PCIe.
 *   - The deltas are those of ks_scheduling_deltas, written to out. out == NULL:
 *     *count only, nothing changes; cap < count: KS_E_INVALID, nothing changes.
 *   - Any PREEMPT or MIGRATE delta: KS_E_INVALID, nothing changes (pinned tasks carry
 *     low = 1 and never move; an evicted task's arcs come from the host's cost model).
 *   - Per PLACE t → p: every out-arc of t whose head is not p is deleted; the arc
 *     t → p becomes (or is added as) the running arc — type 1, low 1, cap 1, cost
 *     continuation_cost; t is bound to p.
 *   - Each unscheduled aggregator (unsched_ids, k of them; NULL: every type-0 node
 *     with an arc into the sink, as ks_update_unsched_costs) loses, on its arc into
 *     the sink, one unit of capacity per task pinned by this call that had an arc
 *     into it. Capacity 0 removes the arc.
 *   - KS_COMMIT_RESOURCE_CAPS: the BFS and sums of ks_topology_stats, a PU's slots
 *     being the capacity of its arc into the sink and its running count the running
 *     arcs (type 1) into it, this call's included; every arc u → v with u not a task,
 *     v not the sink and v a PU, machine, intermediate node or a type-0 node with
 *     slots_below[v] > 0 is set to slots_below[v] − running_below[v] (0 removes it;
 *     only changed arcs get a record). Type-0 heads count as resources exactly as
 *     ks_topology_stats counts them (the coordinator, an equivalence class above
 *     machines): a cost model with arcs between equivalence classes leaves the
 *     flag off and sends those capacities itself (ks_update_nodes).
 *   - A capacity that would fall below its arc's lower bound: KS_E_VERIFY, nothing
 *     changes.
 * Requires a successful solve on the context (KS_E_INVALID otherwise) and, on
 * success, invalidates it as ks_apply_deltas does: fetch the mapping or the flows
 * before committing. A device failure leaves the store unusable until the next
 * ks_load_graph, as for ks_apply_deltas. stats may be NULL. */
int ks_commit_schedule(ks_ctx* ctx, int32_t flags, int64_t continuation_cost,
                       const uint64_t* unsched_ids, size_t k,
                       ks_sched_delta* out, size_t cap, size_t* count,
                       ks_commit_stats* stats /* may be NULL */);

typedef struct ks_preempt_stats {        /* 96 B */
    int64_t placed, preempted, migrated;      /* deltas by kind                               */
    int64_t running_added;                    /* new task→PU running arcs                     */
    int64_t running_converted;                /* existing task→PU arcs turned into running    */
    int64_t running_removed;                  /* running arcs deleted (PREEMPT, MIGRATE)      */
    int64_t unsched_cost_updates;             /* task→aggregator arcs set to preemption_cost  */
    int64_t cap_updates;                      /* resource arcs whose capacity changed         */
    int64_t records;                          /* delta records generated and applied          */
    int64_t reserved[3];
} ks_preempt_stats;

/* The graph edit that follows applySchedulingDeltas with Preemption == true, on device:
 * the other branch of ks_commit_schedule, for a scheduler whose running tasks may move.
 * The context stores no mode: pinned or preemptive is the caller's choice per call. The
 * records (about two per placed task) are generated in device memory and applied as ONE
 * stream with the semantics of ks_apply_deltas (no (src, dst) twice, so superseded is 0).
 *   - The deltas are those of ks_scheduling_deltas, written to out in that call's order
 *     (PREEMPTs first). out == NULL: *count only, nothing changes; cap < count:
 *     KS_E_INVALID, nothing changes.
 *   - PLACE t → p (updateArcsForScheduledTask, graph_manager.go:855-888): no arc of t is
 *     deleted. The arc t → p becomes (UPDATE_ARC) or is added as (ADD_ARC) the running
 *     arc — type 1, low 0, cap 1, cost continuation_cost; t is bound to p. Every arc of t
 *     into an unscheduled aggregator (unsched_ids, k of them; NULL: every type-0 node with
 *     an arc into the sink, as ks_update_unsched_costs) gets cost preemption_cost, bounds
 *     and type kept (updateRunningTaskToUnscheduledAggArc, :1164-1181); a record only if
 *     the cost differs (ChangeArcCost, graph_change_manager.go:171-182).
 *   - PREEMPT t from p (TaskEvicted, :412-433): the running arc t → p is deleted
 *     (DeleteArc's "x src dst 0 0"), t is unbound, nothing else of t changes: its arc
 *     costs are the host's business before the next solve (:432).
 *   - MIGRATE t to q (TaskMigrated, :407-410): PREEMPT from the device-kept binding of t,
 *     then PLACE t → q.
 *   - A PREEMPT or MIGRATE whose arc from t into the PU it leaves is missing or is not
 *     type 1: KS_E_VERIFY, nothing changes (the reference panics, :416-419).
 *   - No aggregator → sink capacity changes (the −1 of pinTaskToNode belongs to the
 *     other mode: a running task may return to its aggregator).
 *   - KS_COMMIT_RESOURCE_CAPS: the BFS and sums of ks_topology_stats, a PU's slots being
 *     the capacity of its arc into the sink; every arc that is a resource arc under
 *     ks_commit_schedule's rule is set to slots_below[v] — running tasks are not
 *     subtracted (capacityFromResNodeToParent returns NumSlotsBelow, :662-667). Only
 *     changed arcs get a record; 0 removes the arc; a capacity below the arc's lower
 *     bound: KS_E_VERIFY, nothing changes.
 * Any other flag: KS_E_INVALID; either cost beyond ±2^40: KS_E_RANGE; an aggregator id
 * that is no live node: KS_E_INVALID. Requires a successful solve and invalidates it on
 * success, as ks_commit_schedule; a device failure after the records were emitted leaves
 * the store unusable until the next ks_load_graph. stats may be NULL;
 * records == running_added + running_converted + running_removed + unsched_cost_updates
 * + cap_updates. */
int ks_commit_preemptive(ks_ctx* ctx, int32_t flags, int64_t continuation_cost, int64_t preemption_cost,
                         const uint64_t* unsched_ids, size_t k,
                         ks_sched_delta* out, size_t cap, size_t* count,
                         ks_preempt_stats* stats /* may be NULL */);

#define KS_REMOVE_RESOURCE_CAPS 1   /* refresh the surviving resource arcs' capacities      */
#define KS_REMOVE_PREEMPTIVE    2   /* capacity rule of ks_commit_preemptive (slots), else
                                       that of ks_commit_schedule (slots − running)         */

typedef struct ks_remove_stats {    /* 96 B */
    int64_t roots;             /* distinct roots                                         */
    int64_t nodes_removed;     /* nodes of the subtree (the REMOVE_NODE records)         */
    int64_t pus_removed;       /* of those, PUs                                          */
    int64_t tasks_evicted;     /* PREEMPT deltas written to evicted                      */
    int64_t arcs_removed;      /* arcs that left the graph: those with an endpoint in the
                                  subtree and the resource arcs whose capacity fell to 0
                                  (ks_store_stats.killed of the stream)                  */
    int64_t cap_updates;       /* resource arcs whose capacity changed                   */
    int64_t records;           /* delta records generated on device and applied:
                                  nodes_removed + cap_updates                            */
    int64_t reserved[5];
} ks_remove_stats;

/* A machine, a rack or any resource subtree leaves the cluster, on device:
 * DeregisterResource (flowscheduler/scheduler.go:162-210) — dfsEvictTasks (:533-566) →
 * HandleTaskEviction → TaskEvicted (flowmanager/graph_manager.go:412-433) for every task
 * bound anywhere in the subtree, then RemoveResourceTopology (:362-387) with
 * traverseAndRemoveTopology (:829-844) for its nodes, and updateResourceStatsUpToRoot for
 * the ancestors' capacities. The REMOVE_NODE records and the capacity records are
 * generated in device memory and applied as ONE stream with the semantics of
 * ks_apply_deltas (all or nothing, in place, store counters, warm-start bookkeeping, the
 * dirty-cell marks of a partition); only the roots, the removed ids, the evictions and
 * the host's node edits cross PCIe.
 *   - Subtree: the roots plus every node reached from them along arcs u → v whose head v
 *     is a PU, a machine or an intermediate node. The walk never enters the sink, a task
 *     or a type-0 node. A root may be a PU, a machine, an intermediate node or a type-0
 *     node: a Quincy rack is type 0, and so is an unscheduled aggregator, which then goes
 *     alone (JobCompleted's removeUnscheduledAggNode). A root that is dead, beyond the
 *     graph, a task or a sink: KS_E_INVALID, the error names the id, nothing changes. A
 *     root listed twice, or one inside another root's subtree, is removed once. A node
 *     that a surviving parent also reaches is still removed (the reference assumes a tree).
 *     The walk follows the arcs the store holds, and a capacity of 0 removes an arc: under
 *     ks_commit_schedule's rule (slots − running) a full machine has no arc into its PU and
 *     a rack none into a full machine, so after pinned commits name such PUs and machines
 *     as roots too (a root inside another root's subtree costs nothing).
 *   - removed receives the removed NodeIDs in ascending order (rcap: its room): the caller
 *     owns id reuse (flowgraph/graph.go:169-182) and needs the removed PUs.
 *   - evicted receives one KS_DELTA_PREEMPT (task, the PU it leaves) per task whose
 *     device-kept binding (ks_set_bindings, the commits) is a removed node, in task-id
 *     order (ecap: its room), and the task is unbound. Nothing else of the task changes:
 *     its running arc goes with the PU and its other arcs into removed nodes go with them;
 *     its surviving arcs and their costs are the host's business before the next solve
 *     (:432), as ks_commit_preemptive says of a PREEMPT. After ks_commit_schedule (pinned
 *     mode) an evicted task has NO out-arc left: the caller lists its arcs, the one into
 *     its aggregator among them, in ks_update_tasks, which adds them and the +1 on the
 *     aggregator → sink arc — the device cannot know the job of a task whose aggregator
 *     arc the pin deleted.
 *   - removed == NULL and evicted == NULL: a probe, *nremoved and *nevicted only, nothing
 *     changes. rcap < *nremoved or ecap < *nevicted: KS_E_INVALID, the counts are
 *     written, nothing changes.
 *   - KS_REMOVE_RESOURCE_CAPS: the BFS and sums of ks_topology_stats over the graph
 *     without the subtree, a PU's slots being the capacity of its arc into the sink and
 *     its running count the running arcs (type 1) into it; every surviving arc that is a
 *     resource arc under ks_commit_schedule's rule is set to slots_below − running_below
 *     of its head, or with KS_REMOVE_PREEMPTIVE to slots_below (ks_commit_preemptive's
 *     rule). Only changed arcs get a record; 0 removes the arc; a capacity below the arc's
 *     lower bound: KS_E_VERIFY, nothing changes. A context with other than one sink
 *     refuses the flag (KS_E_INVALID), as the commits do.
 *   - KS_REMOVE_PREEMPTIVE without KS_REMOVE_RESOURCE_CAPS, or any other flag bit:
 *     KS_E_INVALID.
 * Needs no previous solve (a pending rebuild of the residual CSR runs first, as in
 * ks_topology_stats). On success the solution and the mapping are invalid, exactly as
 * after ks_apply_deltas. A device failure after the records were emitted leaves the store
 * unusable until the next ks_load_graph; the host's node table is rolled back. stats may
 * be NULL; records == nodes_removed + cap_updates. */
int ks_remove_resources(ks_ctx* ctx, int32_t flags, const uint64_t* roots, size_t k,
                        uint64_t* removed, size_t rcap, size_t* nremoved,
                        ks_sched_delta* evicted, size_t ecap, size_t* nevicted,
                        ks_remove_stats* stats /* may be NULL */);

#define KS_COMPLETE_RESOURCE_CAPS 1   /* refresh the resource arcs' capacities            */
#define KS_COMPLETE_PREEMPTIVE    2   /* capacity rule of ks_commit_preemptive (slots),
                                         else ks_commit_schedule's (slots − running)     */

typedef struct ks_complete_stats {    /* 96 B */
    int64_t tasks;            /* distinct tasks removed (the REMOVE_NODE records)         */
    int64_t bound;            /* of those, tasks that were bound to a PU                  */
    int64_t arcs_removed;     /* arcs that left the graph (ks_store_stats.killed)         */
    int64_t unsched_updates;  /* aggregator → sink arcs whose capacity changed            */
    int64_t cap_updates;      /* resource arcs whose capacity changed                     */
    int64_t records;          /* tasks + unsched_updates + cap_updates                    */
    int64_t reserved[6];
} ks_complete_stats;

/* Finished tasks leave the graph, on device: HandleTaskCompletion
 * (flowscheduler/scheduler.go:106-132) → TaskCompleted (flowmanager/graph_manager.go:389-405)
 * → removeTaskNode (:803-813), with updateUnscheduledAggNode(−1) (:396, :1291-1305).
 * TaskFailed and TaskKilled (:435-452, scheduler.go:272-306) are the same graph edit. The
 * records are generated in device memory and applied as ONE stream with the semantics of
 * ks_apply_deltas (all or nothing, in place, store counters, warm-start bookkeeping, the
 * dirty-cell marks of a partition): one REMOVE_NODE per distinct task in ascending id order
 * at stream positions 0 … n − 1, then the capacity records in arc-slot order. No (src, dst)
 * appears twice (ks_store_stats.superseded stays 0). Only the task ids, left and the host's
 * node edits cross PCIe.
 *   - Every id must be a live task node. The first id that is 0, beyond the graph, dead or
 *     not of type task: KS_E_INVALID, the error names the id, nothing changes. An id listed
 *     twice is removed once.
 *   - left (k entries, may be NULL): left[i] is the PU tasks[i] was bound to on the device
 *     (ks_set_bindings, the commits), 0 if unbound, aligned with the input (duplicates get
 *     the same value). It is read before the store unbinds the removed task; the caller
 *     needs it for unbindTaskFromResource (scheduler.go:106-132).
 *   - Aggregators: unsched_ids, nu of them; NULL: every type-0 node with an arc into the
 *     sink, as in the commits. On its arc into the sink an aggregator loses one unit of
 *     capacity per completed task that still had an arc into it; capacity 0 removes the
 *     arc. One rule for both modes: after ks_commit_preemptive every task keeps that arc and
 *     loses the unit (TaskCompleted's −1); after ks_commit_schedule a pinned task has no such
 *     arc and nothing moves (the pin already took the unit, :393-396). In pinned mode a task
 *     that was never placed does lose the unit here, where the reference leaves the
 *     capacity one too high: there this call has no reference counterpart. A capacity that
 *     would fall below its arc's lower bound: KS_E_VERIFY, nothing changes.
 *   - KS_COMPLETE_RESOURCE_CAPS: the BFS and sums of ks_topology_stats over the graph
 *     without the completed tasks, a PU's slots being the capacity of its arc into the sink
 *     and its running count the running arcs (type 1) into it whose tail is not a completed
 *     task; every arc that is a resource arc under ks_commit_schedule's rule is set to
 *     slots_below − running_below of its head, or with KS_COMPLETE_PREEMPTIVE to
 *     slots_below. Only changed arcs get a record; 0 removes the arc; a capacity below the
 *     arc's lower bound: KS_E_VERIFY, nothing changes. A context with other than one sink
 *     refuses the flag (KS_E_INVALID), as the commits do. Under ks_commit_preemptive's rule
 *     a completion changes no resource capacity: such callers leave the flag off, the BFS
 *     is the expensive part of the call.
 *   - k == 0 is legal: without KS_COMPLETE_RESOURCE_CAPS nothing happens and the solution
 *     stays valid; with it the call is a plain refresh of the resource capacities (and
 *     keeps the solution when every capacity already stands).
 *   - KS_COMPLETE_PREEMPTIVE without KS_COMPLETE_RESOURCE_CAPS, or any other flag bit:
 *     KS_E_INVALID.
 *   - Pinned mode (slots − running): a full PU has no arc from its machine and a full
 *     machine none from its rack, since a capacity of 0 removes an arc, and the device
 *     cannot re-create an arc the store no longer holds. Before completing tasks that ran
 *     on full PUs: ks_get_bindings for the finishing tasks, ks_apply_deltas with ADD_ARC
 *     upserts of those PUs' parent chains (any positive capacity), then this call with
 *     KS_COMPLETE_RESOURCE_CAPS, which sets every one of them to its right value.
 * Needs no previous solve (a pending rebuild of the residual CSR runs first, as in
 * ks_remove_resources). On success with k > 0 or any record the solution and the mapping
 * are invalid, exactly as after ks_apply_deltas. A device failure after the records were
 * emitted leaves the store unusable until the next ks_load_graph; the host's node table is
 * rolled back. stats may be NULL; records == tasks + unsched_updates + cap_updates. */
int ks_complete_tasks(ks_ctx* ctx, int32_t flags, const uint64_t* tasks, size_t k,
                      const uint64_t* unsched_ids, size_t nu,
                      uint64_t* left /* k entries, may be NULL */,
                      ks_complete_stats* stats /* may be NULL */);

typedef struct ks_task_arc {          /* 16 B: one out-arc of an arriving task            */
    uint64_t dst;             /* the head: a live node that is no task                    */
    int64_t  cost;
} ks_task_arc;

typedef struct ks_add_stats {         /* 96 B */
    int64_t tasks;            /* ADD_NODE records                                          */
    int64_t arcs_added;       /* task out-arc records (ADD_ARC)                            */
    int64_t unsched_updates;  /* aggregator → sink arcs whose capacity rose (UPDATE_ARC)   */
    int64_t unsched_added;    /* aggregator → sink arcs the store no longer held (ADD_ARC) */
    int64_t records;          /* the sum of the four above                                 */
    int64_t reserved[7];
} ks_add_stats;

/* Arriving tasks enter the graph, on device: AddOrUpdateJobNodes
 * (flowmanager/graph_manager.go:166-208) → addTaskNode (:632-648), updateUnscheduledAggNode(+1)
 * (:194, :1291-1305) and updateTaskNode (:1183-1192) with its three arc writers,
 * updateTaskToUnscheduledAggArc (:1270-1285), updateTaskToEquivArcs (:1197-1226) and
 * updateTaskToResArcs (:1229-1264), each of which calls AddArc(task, head, 0, 1, cost,
 * ArcTypeOther). The records are generated in device memory and applied as ONE stream with
 * the semantics of ks_apply_deltas (all or nothing, in place, store counters, warm-start
 * bookkeeping, the dirty-cell marks of a partition). The stream's order is fixed, so a host
 * restatement produces the identical stream: k ADD_NODE records at positions 0 … k − 1 in
 * input order; the task arcs in input order, arc arc_off[i] + j at position k + arc_off[i] + j;
 * then one record per aggregator that gains a unit, in ascending aggregator id. Only the ids,
 * the offsets, the 16-byte arcs and the host's node edits cross PCIe.
 *   - Task ids: tasks[i] is the NodeID the caller allocated; the caller owns id reuse, as for
 *     ks_remove_resources. It must be in 1 … 2^30 − 1 (KS_E_RANGE) and must not be a live
 *     node; an id listed twice is "already present", as a second ADD_NODE would be. The
 *     first offending id is named: KS_E_INVALID, nothing changes. A reused dead id, the next
 *     id or any id beyond the highest in use is legal, dead slots in between too. The node
 *     is of type task with supply 1; the task count and the sink's auto demand follow
 *     through the host's node table, as after an ADD_NODE. A new task is unbound, also when
 *     its id belonged to a bound task that left earlier.
 *   - Arcs: task i gets arcs[arc_off[i] .. arc_off[i + 1]), each with low 0, cap 1, type 0
 *     and its cost. arc_off[0] == 0 and the offsets never decrease, else KS_E_INVALID; a
 *     task with no arc is legal. Every head must be a node that was live before the call
 *     and is no task (a task of this same call is therefore refused): a head that is 0,
 *     beyond the graph, dead or a task is KS_E_INVALID, the error names the task and the
 *     head, nothing changes. |cost| > 2^40: KS_E_RANGE, nothing changes. The first offending
 *     arc in input order is the one reported. A head listed twice for one task, other than
 *     an aggregator, is the upsert it is in ks_apply_deltas: the later record stands and
 *     ks_store_stats.superseded counts the other. This is the one place where a generated
 *     stream may supersede.
 *   - Aggregators: unsched_ids, nu of them; NULL: every type-0 node with an arc into the
 *     sink, as in the commits. On its arc into the sink an aggregator gains one unit of
 *     capacity per arriving task with an arc into it. If the store holds that arc: one
 *     UPDATE_ARC, low, cost and type kept, cap raised. If it does not (a new job's
 *     aggregator, or one whose capacity fell to 0): one ADD_ARC aggregator → sink with low 0,
 *     cap = the count, cost unsched_sink_cost, type 0 (the AddArc branch of
 *     updateUnscheduledAggNode, :1300-1304). A task with arcs into more than one marked
 *     aggregator, or twice into the same one, is KS_E_INVALID (a task has one job), the
 *     error names the task. With explicit ids a task with no aggregator arc is legal and
 *     moves no capacity. With unsched_ids == NULL an aggregator that has lost its arc into
 *     the sink is invisible, so a task with no arc into a recognised aggregator is
 *     KS_E_INVALID with a message that asks for the ids: the call never silently leaves a
 *     capacity one short. After a pinned commit or ks_complete_tasks may have drained an
 *     aggregator to 0, pass the ids. A context with other than one sink refuses any call in
 *     which an aggregator gains a unit (KS_E_INVALID). unsched_sink_cost beyond ±2^40:
 *     KS_E_RANGE. An aggregator id that is no live node: KS_E_INVALID.
 *   - flags must be 0 (reserved); anything else is KS_E_INVALID.
 * Needs no previous solve and no residual CSR (no BFS runs: arrivals change no resource
 * capacity). k == 0 does nothing and keeps the solution. Success with k > 0 invalidates the
 * solution and the mapping, exactly as ks_apply_deltas does; a node beyond the built CSR or a
 * full segment takes the store's rebuild path (ks_store_stats.rebuilds). Every refusal is
 * found before anything changes on the device, and the host's node table is rolled back. A
 * device failure after the records were emitted leaves the store unusable until the next
 * ks_load_graph; the host's node table is rolled back. stats may be NULL; records == tasks +
 * arcs_added + unsched_updates + unsched_added. */
int ks_add_tasks(ks_ctx* ctx, int32_t flags,
                 const uint64_t* tasks, size_t k,
                 const uint64_t* arc_off /* k + 1 */, const ks_task_arc* arcs,
                 const uint64_t* unsched_ids, size_t nu, int64_t unsched_sink_cost,
                 ks_add_stats* stats /* may be NULL */);

typedef struct ks_res_node {          /* 32 B: one new resource node                        */
    uint64_t id;              /* caller-allocated NodeID (id reuse is the caller's, as in ks_add_tasks) */
    int32_t  type;            /* KS_NODE_PU, _MACHINE, _INTERMEDIATE or _OTHER (a rack)     */
    int32_t  _pad;
    uint64_t slots;           /* PU: capacity of its arc into the sink (MaxTasksPerPu), >= 1; others: 0 */
    int64_t  sink_cost;       /* PU: cost of that arc (LeafResourceNodeToSinkCost); others: 0 */
} ks_res_node;

#define KS_RES_TREE  0   /* the ParentId edge: each child has at most one; slots sum up along it */
#define KS_RES_EXTRA 1   /* any other arc into a node of the call (an equivalence class or cluster
                            aggregator -> machine): gets the head's capacity, sums nothing      */
#define KS_RES_MAX_DEPTH 32   /* KS_RES_TREE edges between a new PU and the topology's root, at most */
typedef struct ks_res_arc {           /* 32 B */
    uint64_t parent, child;
    int64_t  cost;            /* ResourceNodeToResourceNodeCost; used when the arc is created */
    int32_t  kind;            /* KS_RES_TREE / KS_RES_EXTRA */
    int32_t  _pad;
} ks_res_arc;

typedef struct ks_grow_stats {        /* 96 B */
    int64_t nodes, pus, slots;        /* ADD_NODE records; of those PUs; their slots summed      */
    int64_t sink_arcs;                /* PU -> sink ADD_ARC records (== pus)                     */
    int64_t arcs_added;               /* edge records that are ADD_ARC (new head, or arc not held) */
    int64_t cap_updates;              /* edge records that are UPDATE_ARC (held arc, cap raised)  */
    int64_t arcs_skipped;             /* edges that get no record (no new slot beneath the head)  */
    int64_t records;                  /* nodes + sink_arcs + arcs_added + cap_updates             */
    int64_t reserved[4];
} ks_grow_stats;

/* Machines, racks and PUs join the graph, on device: AddResourceTopology
 * (flowmanager/graph_manager.go:238-251) through addResourceTopologyDFS (:557-630),
 * addResourceNode (:528-551), updateResToSinkArc (:1116-1129) and capacityFromResNodeToParent
 * (:662-667), and updateResourceStatsUpToRoot (:1041-1061) for the arcs above the attach
 * point. The records are generated in device memory and applied as ONE stream with the
 * semantics of ks_apply_deltas (all or nothing, in place, store counters, warm-start
 * bookkeeping, the dirty-cell marks of a partition). The stream's order is fixed, so a host
 * restatement produces the identical stream: n ADD_NODE records at positions 0 … n − 1 in
 * input order; the PU → sink arcs in input order of the PUs; then one record per edge that
 * gets one, in input order. No (src, dst) appears twice: ks_store_stats.superseded stays 0.
 * Only the two 32-byte arrays and the host's node edits cross PCIe; the caller keeps no shadow
 * of the ancestors' capacities and need not know which ancestor arc the store still holds.
 *   - Nodes: each enters with supply 0 and its type. The ids follow the ADD_NODE rule of
 *     ks_apply_deltas, as in ks_add_tasks: in 1 … 2^30 − 1 (KS_E_RANGE), no live node, an id
 *     listed twice is "already present" (KS_E_INVALID); a reused dead id or any id beyond the
 *     highest in use is legal. A type of task or sink, or an unknown one: KS_E_INVALID. A PU
 *     with slots == 0, or another node with slots or sink_cost other than 0: KS_E_INVALID.
 *     slots > 2^53 or |sink_cost| > 2^40: KS_E_RANGE. The first offending node in input order
 *     is named (on one node: the id, the type, then the values); nothing changes. The new
 *     slots of one call summed beyond 2^53: KS_E_RANGE. Each new PU gets ADD_ARC PU → sink
 *     (low 0, cap slots, cost sink_cost, type 0); a call with a PU needs exactly one sink
 *     (KS_E_INVALID).
 *   - Edges: parent and child must each be a node of this call or a node that was live before
 *     it; the parent no task, no sink and no PU, the child no task and no sink; parent ==
 *     child: KS_E_INVALID. An unknown kind: KS_E_INVALID. A KS_RES_TREE edge from a new parent
 *     to a node that was live before the call: KS_E_INVALID (a live node does not move).
 *     |cost| > 2^40: KS_E_RANGE. A (parent, child) pair listed twice: KS_E_INVALID. A child
 *     named by two KS_RES_TREE edges: KS_E_INVALID, the error names the child (a resource has
 *     one parent). The first offending edge in input order is the one reported, on one edge in
 *     the order of this list; nothing changes. The KS_RES_TREE edges whose child was live
 *     before the call are the chain: the caller lists the ancestors of each attach point up to
 *     the topology's root (rack → machine, root → rack, …; Go's nodeToParentNode has them).
 *   - New slots beneath a node: S(v) = the slots of the new PUs from which v is reached going
 *     up KS_RES_TREE edges, a new PU counting itself. A PU whose walk has not ended after
 *     KS_RES_MAX_DEPTH edges (a cycle, or a topology too deep): KS_E_INVALID, the first such PU
 *     in input order is named; nothing changes.
 *   - Capacities: a function of the edge's head v only, for both kinds. New resources run
 *     nothing, so slots − running (ks_commit_schedule's rule) and slots (ks_commit_preemptive's)
 *     both rise by exactly S(v): one rule serves both, which is why flags is reserved.
 *       S(v) == 0                      no record (arcs_skipped): a capacity of 0 is an absent
 *                                      arc. An empty rack's arc is created by the later call
 *                                      that attaches beneath it and lists the edge as chain.
 *       v new, S(v) > 0                ADD_ARC (low 0, cap S(v), the edge's cost, type 0)
 *       v live, the store holds        UPDATE_ARC: low, cost and type kept, cap = old + S(v)
 *         parent → v                   (beyond 2^53: KS_E_RANGE, nothing changes)
 *       v live, the store does not     ADD_ARC (low 0, cap S(v), the edge's cost, type 0): the
 *         hold it                      capacity had fallen to 0 (a full machine under the
 *                                      pinned rule), which removed the arc
 *     The store's (src, dst) index tells the last two apart; the pinned recipe of
 *     ks_complete_tasks is not needed here.
 *   - What the device cannot check: that the chain reaches the root, and that every arc into
 *     a chain node is listed. A chain cut short leaves the arcs above it one subtree short, an
 *     unlisted KS_RES_EXTRA arc into a chain node likewise. ks_complete_tasks(k = 0,
 *     KS_COMPLETE_RESOURCE_CAPS[ | KS_COMPLETE_PREEMPTIVE]) repairs both (arcs that fell to 0
 *     first re-created by the pinned recipe).
 *   - A held capacity that was not the rule's value is raised all the same. The capacity rule
 *     of the commits, ks_remove_resources and ks_complete_tasks treats a type-0 head (a rack)
 *     as a resource only while slots_below[v] > 0: once the last machine beneath a rack has
 *     left (or, under slots − running, the rack's only machine with a free slot has), the arc
 *     into the rack KEEPS the capacity it had, which no flow can use. A machine that later
 *     joins beneath that rack with the chain listed gets old + S(v) on that arc, S(v) being
 *     the right value. The surplus admits no flow (the arcs beneath carry S(v)), but the
 *     capacity is not the rule's any more: a round that adds resources beneath racks that may
 *     have been emptied or filled follows ks_add_resources with the same refresh,
 *     ks_complete_tasks(k = 0, KS_COMPLETE_RESOURCE_CAPS[ | KS_COMPLETE_PREEMPTIVE]), which
 *     sets it (tests/round_ref.py does so after every call with an edge).
 *   - flags must be 0 (reserved); anything else is KS_E_INVALID.
 * Needs no previous solve, no residual CSR and no BFS. n == 0 && m == 0 does nothing and
 * keeps the solution, as does a call that generates no record. Success with a record
 * invalidates the solution and the mapping, exactly as ks_apply_deltas does; a node beyond the
 * built CSR or a full segment takes the store's rebuild path (ks_store_stats.rebuilds). Every
 * refusal is found before anything changes on the device, and the host's node table is rolled
 * back. A device failure after the records were emitted leaves the store unusable until the
 * next ks_load_graph; the host's node table is rolled back. stats may be NULL. On a batch:
 * ks_batch_add_resources.
 * UpdateResourceTopology (:217-236, a live resource's slots change): ks_update_nodes with the
 * PU → sink arc listed at its new slot count, then ks_complete_tasks(k = 0,
 * KS_COMPLETE_RESOURCE_CAPS [| KS_COMPLETE_PREEMPTIVE]) for the capacities above it. */
int ks_add_resources(ks_ctx* ctx, int32_t flags /* must be 0 */,
                     const ks_res_node* nodes, size_t n,
                     const ks_res_arc* arcs, size_t m,
                     ks_grow_stats* stats /* may be NULL */);

#define KS_UPDATE_KEEP_UNLISTED 1   /* no arc is deleted: additions and cost changes only */

typedef struct ks_update_stats {      /* 96 B */
    int64_t tasks;            /* tasks listed                                              */
    int64_t arcs_added;       /* listed arcs the store did not hold (ADD_ARC)              */
    int64_t cost_updates;     /* held arcs whose cost changed (UPDATE_ARC)                 */
    int64_t arcs_unchanged;   /* listed, held, same cost: no record                        */
    int64_t running_kept;     /* listed heads whose held arc is a running arc: no record   */
    int64_t arcs_removed;     /* held, unlisted, deleted (UPDATE_ARC 0/0)                  */
    int64_t unsched_updates;  /* aggregator → sink arcs whose capacity rose (UPDATE_ARC)   */
    int64_t unsched_added;    /* aggregator → sink arcs re-created (ADD_ARC)               */
    int64_t records;          /* arcs_added + cost_updates + arcs_removed + the two above  */
    int64_t reserved[3];
} ks_update_stats;

/* Live tasks' arcs follow the cost model, on device: UpdateTimeDependentCosts =
 * AddOrUpdateJobNodes (flowmanager/graph_manager.go:211-213, :166-208), which for a task that
 * already has its node runs updateTaskNode (:1183-1192) with its three arc writers,
 * updateTaskToUnscheduledAggArc (:1270-1285), updateTaskToEquivArcs (:1197-1226) and
 * updateTaskToResArcs (:1229-1264). Each adds the arc the graph does not hold or calls
 * ChangeArcCost, which logs a record only when the cost differs (graph_change_manager.go:171-182),
 * and then removeInvalidECPrefArcs / removeInvalidPrefResArcs (:732-790) delete the arcs that are
 * no longer preferred; updateRunningTaskNode (:1140-1158) does the same for a running task under
 * preemption. The caller lists, per task, the non-running out-arcs the task should have; the
 * device diffs each list against the arcs the store holds, so the caller keeps no shadow of the
 * tasks' arcs and costs (which ks_update_unsched_costs and the commits change on the device
 * alone). The records are generated in device memory and applied as ONE stream with the
 * semantics of ks_apply_deltas (all or nothing, in place, store counters, warm-start bookkeeping,
 * the dirty-cell marks of a partition). The stream's order is fixed, so a host restatement
 * produces the identical stream: the records on held arcs (cost changes and deletions) in
 * ascending arc-slot order, the order in which ks_get_graph lists arcs; the ADD_ARC records of
 * the listed arcs the store did not hold, in input order; then one record per aggregator that
 * gains a unit, in ascending aggregator id. No (src, dst) appears twice
 * (ks_store_stats.superseded stays 0). Only the ids, the offsets and the 16-byte arcs cross PCIe.
 *   - Task ids: every id must be a live task node. The first id that is 0, beyond the graph,
 *     dead, of another type or listed a second time: KS_E_INVALID, the error names the id,
 *     nothing changes (two lists for one task have no meaning: a repeat is refused, not
 *     merged). No node is added or removed; the host's node table is only read.
 *   - Listed arcs: task i's list is arcs[arc_off[i] .. arc_off[i + 1]), the offsets as in
 *     ks_add_tasks (arc_off[0] == 0, never decreasing, else KS_E_INVALID); an empty list is
 *     legal. Every head must be a live node that is no task: a head that is 0, beyond the
 *     graph, dead or a task is KS_E_INVALID, the error names the task and the head.
 *     |cost| > 2^40: KS_E_RANGE. A head listed twice for one task: KS_E_INVALID (the diff needs
 *     a set; in ks_add_tasks a repeat is an upsert). The first offending arc in input order is
 *     the one reported; on one arc the head comes before the repeat and the repeat before the
 *     cost. Nothing changes. Per listed arc (t, h):
 *       the store does not hold it     ADD_ARC (low 0, cap 1, the listed cost, type 0)
 *       held, type 0, another cost     UPDATE_ARC: low, cap and type kept, the listed cost,
 *                                      old_cost the cost it had
 *       held, type 0, the same cost    no record (ChangeArcCost logs nothing then)
 *       held as a running arc (type 1) no record and its cost stays (:1250-1255): that cost
 *                                      belongs to ks_update_unsched_costs and the commits
 *   - Held arcs of a listed task that its list does not name: a running arc is kept. This is a
 *     deliberate deviation: the reference's removeInvalidPrefResArcs deletes a running arc
 *     whose PU left the preferences and then panics at the next updateRunningTaskNode. An arc
 *     into a marked aggregator is kept with its cost (the reference never deletes it, and
 *     ks_update_unsched_costs may have aged the cost on the device). Every other arc is deleted
 *     (UPDATE_ARC with low == cap == 0). With KS_UPDATE_KEEP_UNLISTED nothing is deleted.
 *   - Aggregators: unsched_ids, nu of them; NULL: every type-0 node with an arc into the
 *     sink, as in the commits. On its arc into the sink an aggregator gains one unit of
 *     capacity per listed task whose listed arc into it the store did not hold: the mirror of
 *     ks_complete_tasks' loss rule, and the +1 of a task evicted after a pinned commit (after a
 *     preemptive commit the task still has the arc, only its cost moves and nothing is gained).
 *     The record is that of ks_add_tasks: if the store holds aggregator → sink, one UPDATE_ARC,
 *     low, cost and type kept, cap raised; if not, one ADD_ARC with low 0, cap = the count, cost
 *     unsched_sink_cost, type 0 (:1300-1304). A task that would end with arcs into two marked
 *     aggregators, listed, held or one of each: KS_E_INVALID, the error names the task (a task
 *     does not change its job). With unsched_ids == NULL a drained aggregator is invisible, so
 *     a task without a device-kept binding that would end with no arc into a recognised
 *     aggregator is KS_E_INVALID with a message that asks for the ids: the call never silently
 *     leaves a capacity one short. A bound task may have none (a pinned running task has no
 *     aggregator arc). A context with other than one sink refuses any call in which an
 *     aggregator gains a unit (KS_E_INVALID). unsched_sink_cost beyond ±2^40: KS_E_RANGE. An
 *     aggregator id that is no live node: KS_E_INVALID.
 *   - flags: KS_UPDATE_KEEP_UNLISTED or 0; any other bit is KS_E_INVALID.
 * Needs no previous solve. Without the flag the tasks' segments of the residual CSR are walked
 * (a pending rebuild runs first, as in ks_complete_tasks); with it only the node store, the arc
 * table and the (src, dst) index are read, as in ks_add_tasks. k == 0 does nothing and keeps the
 * solution, as does a call that generates no record (the solution and the mapping stay valid);
 * a call that generates any record invalidates them, exactly as ks_apply_deltas does. A full
 * segment takes the store's rebuild path (ks_store_stats.rebuilds). Every refusal is found before
 * anything changes on the device. A device failure after the records were emitted leaves the
 * store unusable until the next ks_load_graph. stats may be NULL; records == arcs_added +
 * cost_updates + arcs_removed + unsched_updates + unsched_added.
 * The class and resource nodes' arcs are ks_update_nodes; UpdateResourceTopology (:217-236) is
 * ks_update_nodes on the PU → sink arc, then ks_complete_tasks(k = 0, KS_COMPLETE_RESOURCE_CAPS
 * [| KS_COMPLETE_PREEMPTIVE]). */
int ks_update_tasks(ks_ctx* ctx, int32_t flags,
                    const uint64_t* tasks, size_t k,
                    const uint64_t* arc_off /* k + 1 */, const ks_task_arc* arcs,
                    const uint64_t* unsched_ids, size_t nu, int64_t unsched_sink_cost,
                    ks_update_stats* stats /* may be NULL */);

#define KS_CAP_KEEP UINT64_MAX        /* listed arc: keep the held arc's capacity (ChangeArcCost) */
#define KS_NODES_KEEP_UNLISTED 1      /* no arc is deleted for being unlisted */

typedef struct ks_node_arc { uint64_t dst; int64_t cost; uint64_t cap; } ks_node_arc;   /* 24 B */

typedef struct ks_node_stats {        /* 96 B */
    int64_t nodes;           /* tails listed                                                  */
    int64_t arcs_added;      /* listed, not held, cap > 0 (ADD_ARC)                           */
    int64_t arcs_updated;    /* listed, held, cost or capacity differs (UPDATE_ARC)           */
    int64_t arcs_unchanged;  /* listed, held, same cost and capacity: no record               */
    int64_t arcs_skipped;    /* listed, not held, cap == 0: no record                         */
    int64_t arcs_zeroed;     /* listed, held, cap == 0: deleted (UPDATE_ARC 0/0)              */
    int64_t arcs_removed;    /* held, unlisted, deleted (UPDATE_ARC 0/0)                      */
    int64_t records;         /* arcs_added + arcs_updated + arcs_zeroed + arcs_removed        */
    int64_t reserved[4];
} ks_node_stats;

/* Class and resource arcs follow the cost model, on device: the part of AddOrUpdateJobNodes →
 * updateFlowGraph (flowmanager/graph_manager.go:1012-1033) that ks_update_tasks leaves out. The
 * sweep walks on from the task nodes through every equivalence-class node and every resource
 * node it reaches. updateEquivClassNode (:931-1010): per class, EquivClassToEquivClass and
 * EquivClassToResourceNode each give a cost AND a capacity; an absent arc gets AddArc(0, cap,
 * cost), a held one ChangeArc(low kept, cap, cost), and removeInvalidECPrefArcs /
 * removeInvalidPrefResArcs (:732-790) drop what is no longer preferred. updateResourceNode →
 * updateResOutgoingArcs (:1094-1111): ChangeArcCost on every resource → resource arc, and
 * updateResToSinkArc (:1116-1129) on PU → sink. The caller lists, per tail, the out-arcs it
 * should have with their costs and capacities; the device diffs each list against the arcs the
 * store holds, so the caller keeps no shadow of those arcs (which the commits,
 * ks_remove_resources, ks_complete_tasks and ks_add_resources rewrite or delete on the device
 * alone). The records are generated in device memory and applied as ONE stream with the
 * semantics of ks_apply_deltas (all or nothing, in place, store counters, warm-start bookkeeping,
 * the dirty-cell marks of a partition). The stream's order is that of ks_update_tasks, so a host
 * restatement produces the identical stream: the records on held arcs in ascending arc-slot
 * order, the order in which ks_get_graph lists arcs; then the ADD_ARC records in input order.
 * No (src, dst) appears twice (ks_store_stats.superseded stays 0). Only the ids, the offsets and
 * the 24-byte arcs cross PCIe.
 *   - Tails: every nodes[i] must be a live node of type 0, a machine, an intermediate node or a
 *     PU. The first id in input order that is 0, beyond the graph, dead, a task, a sink or
 *     listed a second time: KS_E_INVALID, the error names the id, nothing changes. No node is
 *     added or removed; the host's node table is only read.
 *   - Listed arcs: tail i's list is arcs[arc_off[i] .. arc_off[i + 1]), the offsets as in
 *     ks_add_tasks (arc_off[0] == 0, never decreasing, else KS_E_INVALID); an empty list is
 *     legal. The head must be a live node that is no task and not the tail itself; a PU's only
 *     legal head is a sink, and a sink head is legal only from a PU or a type-0 tail: else
 *     KS_E_INVALID, the error names the tail and the head. A head listed twice for one tail:
 *     KS_E_INVALID. |cost| > 2^40: KS_E_RANGE. A cap other than KS_CAP_KEEP above 2^53:
 *     KS_E_RANGE. The first offending arc in input order is the one reported; on one arc the
 *     head comes before the repeat, the repeat before the cost, the cost before the capacity.
 *     Only when every arc passes these is the store consulted, and again the first offending
 *     arc in input order is reported (the two cases below that refuse). Per listed arc (u, h):
 *       the store does not hold it, cap > 0         ADD_ARC (low 0, cap, the listed cost, type 0)
 *       the store does not hold it, cap == 0        no record (arcs_skipped): a capacity of 0 is
 *                                                   an absent arc, as everywhere in this library
 *       the store does not hold it, KS_CAP_KEEP     KS_E_INVALID naming tail and head (there is
 *                                                   nothing to keep)
 *       held; c = cap, or under KS_CAP_KEEP the held capacity:
 *         c == 0 and the held lower bound is 0      UPDATE_ARC 0/0, a deletion (arcs_zeroed)
 *         c below the held lower bound              KS_E_VERIFY, nothing changes, as in the commits
 *         cost and capacity both unchanged          no record (ChangeArc logs nothing then)
 *         otherwise                                 UPDATE_ARC: low and type kept, cap c, the
 *                                                   listed cost, old_cost the cost it had
 *   - Held arcs of a listed tail that its list does not name: a type-0 tail's are deleted
 *     (UPDATE_ARC with low == cap == 0), except an arc into a sink, which stays: removeInvalid*
 *     never looks at the sink, and an unscheduled aggregator's arc into the sink belongs to the
 *     unit accounting of the task calls. So an empty list is "no preferences" (:942-945,
 *     :980-983) and drops every non-sink arc of the class. A machine, an intermediate node or a
 *     PU never loses an arc: updateResOutgoingArcs deletes nothing. With KS_NODES_KEEP_UNLISTED
 *     nothing at all is deleted for being unlisted.
 *   - flags: KS_NODES_KEEP_UNLISTED or 0; any other bit is KS_E_INVALID.
 * Needs no previous solve. Without the flag the type-0 tails' segments of the residual CSR are
 * walked (a pending rebuild runs first, as in ks_update_tasks); with it only the node store, the
 * arc table and the (src, dst) index are read. k == 0 does nothing and keeps the solution, as
 * does a call that generates no record (the solution and the mapping stay valid); a call that
 * generates any record invalidates them, exactly as ks_apply_deltas does. A full segment takes
 * the store's rebuild path (ks_store_stats.rebuilds). Every refusal is found before anything
 * changes on the device. A device failure after the records were emitted leaves the store
 * unusable until the next ks_load_graph. stats may be NULL. On a batch: ks_batch_update_nodes.
 * What the call does not do:
 *   - It does not purge a class that lost its last in-arc: the reference declares
 *     PurgeUnconnectedEquivClassNodes (:347-357) and never calls it. ks_remove_resources with
 *     the class as a root removes one.
 *   - A capacity written here is overwritten by any later call that runs the capacity rule
 *     (KS_COMMIT_RESOURCE_CAPS, KS_REMOVE_RESOURCE_CAPS, KS_COMPLETE_RESOURCE_CAPS) on an arc
 *     that rule counts as a resource arc: the caveat the commits already carry.
 *   - UpdateResourceTopology (:217-236): list PU → sink with the new slot count here, then run
 *     ks_complete_tasks(k = 0, KS_COMPLETE_RESOURCE_CAPS [| KS_COMPLETE_PREEMPTIVE]), which
 *     carries the new slots up the chain. Under the pinned rule (slots − running) a PU that
 *     was FULL has no arc from its machine, and neither has any ancestor that was full with it:
 *     the refresh writes only arcs that exist, so the new slot would stay cut off. List those
 *     chain arcs (machine → PU and upwards as far as the heads were full) in the same call with
 *     any positive capacity: they are ADD_ARC, and the refresh sets them. It is the parent-chain
 *     recipe of ks_complete_tasks, through this call.
 * What a caller without a shadow can list (tests/round_ref.py plays it over whole rounds):
 *   - KS_CAP_KEEP only on an arc it knows the store to hold. The capacity rule deletes every arc
 *     into a head with no room (pinned: a full PU, a machine or rack of full PUs) and counts a
 *     class → machine arc as a resource arc, so after a pinned commit a class has no arc into a
 *     full machine and KS_CAP_KEEP on it is refused. Class arcs are therefore listed with an
 *     explicit capacity (the machine's room, or less): 0 while the machine is full (skipped or
 *     zeroed), positive once a completion freed a slot (ADD_ARC: the arc comes back here, not
 *     with the completion's parent-chain upserts, which name the resource tree only).
 *   - The arc into a rack with no slot beneath it is the one whose presence cannot be known
 *     (the rule leaves it as it was, absent or stale): list it with capacity 0.
 *     ks_add_resources re-creates it when a machine joins. */
int ks_update_nodes(ks_ctx* ctx, int32_t flags,
                    const uint64_t* nodes, size_t k,
                    const uint64_t* arc_off /* k + 1 */, const ks_node_arc* arcs,
                    ks_node_stats* stats /* may be NULL */);

/* pu[i] = the PU task[i] is bound to on the device (ks_set_bindings, the commits), 0 =
 * unbound: for the pinned recipe above and for checkpoints. A task id that is not a live
 * task: KS_E_INVALID. */
int ks_get_bindings(ks_ctx* ctx, const uint64_t* task, uint64_t* pu, size_t k);

/* ---- config 5: independent graphs sharded over GPUs (SURVEY §7 step 6, §8 row e) --
 * No reference counterpart (ksched solves one graph per round,
 * flowscheduler/scheduler.go:350); this is the north star's multi-GPU mode: cluster
 * cells / what-if graphs, graph g on global rank g mod world, each device solving
 * the disjoint union of its graphs, then ONE collective — every rank's per-graph
 * rows to rank 0 over RCCL (ncclSend/ncclRecv in a group), inside the library. */
typedef struct ks_batch ks_batch;
#define KS_UNIQUE_ID_BYTES 128

/* One process driving several devices (ncclCommInitAll over devices[0..ndev)). */
ks_batch*   ks_batch_create(const int* devices, int ndev, const ks_opts* opts);
/* One process per GPU (e.g. under torch.distributed.run): rank 0 makes the id with
 * ks_batch_unique_id and shares it out of band; every rank then calls this. */
int         ks_batch_unique_id(uint8_t* id /* KS_UNIQUE_ID_BYTES */);
ks_batch*   ks_batch_create_rank(int device, int nranks, int rank, const uint8_t* id, const ks_opts* opts);
void        ks_batch_destroy(ks_batch* b);
const char* ks_batch_last_error(ks_batch* b);
/* Every rank passes ALL ngraphs graphs (arrays as for ks_load_graph); each device
 * uploads the ones it owns. */
int ks_batch_load(ks_batch* b, size_t ngraphs, const ks_node* const* nodes, const size_t* n,
                  const ks_arc* const* arcs, const size_t* m);
/* Solve every local device's union concurrently; results[i] (may be NULL) for the
 * i-th local device. */
int ks_batch_solve(ks_batch* b, ks_result* results);
/* Collective (all ranks call it): per graph its cost, flow value and the PU node id
 * (local to the graph, 0 = unscheduled) of each of its task nodes in id order,
 * gathered to global rank 0, whose pu[g·max_tasks ..], cost[g], flow[g] receive
 * them (other ranks may pass NULL). A rank that fails to pack its rows still
 * enters the collective; every rank then returns that failure. */
int ks_batch_gather(ks_batch* b, size_t max_tasks, uint64_t* pu, int64_t* cost, int64_t* flow);

/* Layout of the gather (host-only, no device or RCCL: the packing and unpacking
 * of ks_batch_gather use exactly these). Graph g is owned by global rank
 * g mod world as its (g div world)-th graph; each rank sends one block of
 * ks_batch_block_len elements: [status][slots rows of 2 + max_tasks: cost, flow
 * value, PU per task]. ks_batch_unpack turns the world blocks rank 0 received (in
 * rank order) into graph order; it returns a rank's non-zero status word. */
size_t      ks_batch_slots(size_t ngraphs, int world);
int         ks_batch_owner(size_t g, int world, int* rank, size_t* slot);
size_t      ks_batch_block_len(size_t ngraphs, int world, size_t max_tasks);
int         ks_batch_unpack(const int64_t* gathered, size_t ngraphs, int world, size_t max_tasks, uint64_t* pu,
                            int64_t* cost, int64_t* flow);

/* ---- batch rounds: deltas, a re-solve of the changed cells, commits ------
 * A batch goes through scheduling rounds as a single context does: the union stays
 * resident, every graph keeps its own id range in it, and a warm re-solve
 * (ks_opts.warm_start >= 1) launches only the cells some record touched since their
 * last solve (ks_result.cells_run; DESIGN §3.5 "which cells run").
 *
 * Layout (host-only, no device: ks_batch_load and ks_batch_apply_deltas use exactly
 * these). Graph i of a device's union owns the node ids (off[i], off[i+1]], where
 * off[i+1] = off[i] + maxid[i] + spare: ks_batch_node_offsets writes the k + 1 offsets.
 * ks_batch_translate_deltas moves a stream from graph-local ids into the range
 * (lo, hi]: lo is added to id, src and dst of every record (each kind's unused id
 * fields stay as they are; a record of an unknown kind is copied unchanged, for
 * ks_apply_deltas to refuse). A used id that is 0 or greater than hi − lo: KS_E_RANGE
 * and nothing is written. out == in works. */
int ks_batch_node_offsets(const uint64_t* maxid, size_t k, size_t spare, int64_t* off /* k + 1 */);
int ks_batch_translate_deltas(int64_t lo, int64_t hi, const ks_delta* in, size_t k, ks_delta* out);

/* Node ids every graph may grow by after the load (new tasks beyond its highest id).
 * Takes effect at the next ks_batch_load; 0 (the default) packs the graphs tightly, as
 * before the batch had rounds. With spare_ids > 0 the load also builds the residual CSR with the
 * slack of an incrementally edited graph, so the first delta stream lands in place. */
int ks_batch_reserve(ks_batch* b, size_t spare_ids);

/* Every rank passes all ngraphs streams (graph-local ids; deltas[g] == NULL or
 * k[g] == 0: graph g untouched). Each local device translates the streams of the
 * graphs it owns and applies them, in graph order, as ONE stream with the semantics of
 * ks_apply_deltas (all or nothing per device). An id outside its graph's range — a new
 * node beyond the reserved ids, an arc into another cell — is KS_E_RANGE: the error
 * names the graph and the id, and that device is unchanged. With ks_opts.auto_sink a
 * graph with exactly one sink then gets that sink's supply set to −Σ of its other
 * nodes' supplies (a SET_EXCESS record at the end of the stream). No collective: a
 * rank returns its own failure. */
int ks_batch_apply_deltas(ks_batch* b, size_t ngraphs, const ks_delta* const* deltas, const size_t* k);

/* Graph g as it stands, in graph-local ids (ks_get_graph of its part of the union).
 * KS_E_INVALID on a rank that does not own g. Call with caps of 0 to size. */
int ks_batch_get_graph(ks_batch* b, size_t g, ks_node* nodes, size_t ncap, size_t* n, ks_arc* arcs, size_t acap,
                       size_t* m);

/* ks_set_bindings for graph g, in graph-local ids (KS_E_INVALID when g is not local). */
int ks_batch_set_bindings(ks_batch* b, size_t g, const uint64_t* task, const uint64_t* pu, size_t k);

typedef struct ks_batch_delta {
    int32_t  type;             /* KS_DELTA_*                                             */
    int32_t  graph;            /* the graph the task belongs to                          */
    uint64_t task;             /* graph-local ids, as in ks_sched_delta                  */
    uint64_t pu;
} ks_batch_delta;

/* ks_commit_schedule / ks_commit_preemptive on every local device's union. The
 * unscheduled aggregators are every type-0 node with an arc into a sink (the NULL rule
 * of the single-graph calls). The deltas cover the calling process's graphs, grouped by
 * graph in ascending order and within a graph in the order of ks_scheduling_deltas.
 * out == NULL: *count only, nothing changes; cap < count: KS_E_INVALID, nothing changes.
 * KS_COMMIT_RESOURCE_CAPS seeds the topology BFS with every live sink (one per graph).
 * The records the commit generates mark their cells for the next solve, on the device.
 * stats (may be NULL) are summed over the local devices. No collective. */
int ks_batch_commit_schedule(ks_batch* b, int32_t flags, int64_t continuation_cost,
                             ks_batch_delta* out, size_t cap, size_t* count, ks_commit_stats* stats);
int ks_batch_commit_preemptive(ks_batch* b, int32_t flags, int64_t continuation_cost, int64_t preemption_cost,
                               ks_batch_delta* out, size_t cap, size_t* count, ks_preempt_stats* stats);

/* ---- batch rounds, the task side: arrivals, completions, refreshes --------
 * The twins of ks_add_tasks, ks_complete_tasks, ks_update_tasks, ks_get_bindings and
 * ks_update_unsched_costs on a batch. Every rank passes one list per graph (ngraphs ==
 * the loaded graphs, else KS_E_INVALID) and applies those of the graphs it owns; every id
 * in a list is in its graph's OWN numbering. Each call has the semantics of its lone twin
 * applied to every listed graph, as ONE device call per local device: the lists of a
 * device's graphs go up back to back, the heads are range-checked and moved into the
 * union's ids by one kernel, the record stream is generated on the device, is all or
 * nothing there and marks its cells for the next solve. An aggregator's capacity record
 * ends at the sink of the aggregator's own cell (a per-cell sink table, rebuilt per
 * call); a cell without exactly one sink refuses a gaining aggregator.
 *
 * Refused before any device changes: a null array where k > 0 (KS_E_INVALID), offsets
 * that do not start at 0 or fall (KS_E_INVALID), and any id outside 1..span of its graph,
 * a task, a head or an aggregator (KS_E_RANGE; span = the graph's highest id at the load
 * plus the reserved ids). The device's refusals keep the lone call's status code. Every
 * message names the graph and the graph-local id. unsched_ids is one mode per call:
 * either every listed graph passes its aggregators or none does (the NULL rule), else
 * KS_E_INVALID.
 *
 * With ks_opts.auto_sink, after ks_batch_add_tasks and ks_batch_complete_tasks every
 * touched graph with exactly one sink has that sink's supply at −Σ of its other nodes'
 * supplies, as after ks_batch_apply_deltas. stats (may be NULL) are summed over the local
 * devices. No collective: a rank returns its own failure. The resource side of a round
 * (ks_batch_remove_resources, ks_batch_add_resources) follows the same contract, below. */
typedef struct ks_batch_task_list {   /* one graph's part of a call, in the graph's OWN ids */
    const uint64_t*    tasks;       size_t k;     /* k == 0: the graph is untouched          */
    const uint64_t*    arc_off;                   /* k + 1, as ks_add_tasks (unused by complete) */
    const ks_task_arc* arcs;
    const uint64_t*    unsched_ids; size_t nu;    /* NULL: the NULL rule of the lone call    */
} ks_batch_task_list;

/* ks_add_tasks per listed graph: AddOrUpdateJobNodes (flowmanager/graph_manager.go:166-208)
 * → addTaskNode (:632-648), updateUnscheduledAggNode(+1) (:194, :1291-1305), updateTaskNode
 * (:1183-1192). flags is reserved: pass 0. */
int ks_batch_add_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                       int64_t unsched_sink_cost, ks_add_stats* stats);
/* ks_complete_tasks per listed graph: HandleTaskCompletion (flowscheduler/scheduler.go:106-132)
 * → TaskCompleted (flowmanager/graph_manager.go:389-405) → removeTaskNode (:803-813). flags:
 * KS_COMPLETE_*. left (may be NULL): left[g] (may be NULL) receives, for a graph this rank
 * owns, the k bindings read before anything changed, graph-local, 0 = unbound; an id listed
 * twice gets the same value twice. With every k == 0 and KS_COMPLETE_RESOURCE_CAPS the call is
 * the lone call's plain capacity refresh (k == 0) on every local device's union, under the NULL
 * rule: what a round runs after ks_batch_add_resources. */
int ks_batch_complete_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                            uint64_t* const* left, ks_complete_stats* stats);
/* ks_update_tasks per listed graph: UpdateTimeDependentCosts (flowmanager/graph_manager.go:211-213)
 * → updateTaskNode (:1183-1192) with removeInvalidECPrefArcs / removeInvalidPrefResArcs
 * (:732-790). flags: KS_UPDATE_*. */
int ks_batch_update_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                          int64_t unsched_sink_cost, ks_update_stats* stats);
/* ks_get_bindings for graph g, graph-local ids both ways (the mirror of
 * ks_batch_set_bindings; KS_E_INVALID when g is not local). */
int ks_batch_get_bindings(ks_batch* b, size_t g, const uint64_t* task, uint64_t* pu, size_t k);
/* ks_update_unsched_costs: UpdateAllCostsToUnscheduledAggs (flowmanager/graph_manager.go:462-475).
 * lists == NULL: every aggregator of every local graph (the NULL rule). Else only
 * unsched_ids / nu of each entry are read: the aggregators whose tasks are re-costed (a
 * graph with nu == 0 is untouched). *changed (may be NULL): summed over the local devices. */
int ks_batch_update_unsched_costs(ks_batch* b, size_t ngraphs, const ks_batch_task_list* lists, int32_t mode,
                                  int64_t cost, int64_t continuation_cost, size_t* changed);

/* ---- batch rounds, the resource side: machines and racks leave and join ----
 * The twins of ks_remove_resources and ks_add_resources on a batch, under the contract
 * written above ks_batch_task_list: one list per loaded graph on every rank (else
 * KS_E_INVALID), every id in its graph's OWN numbering, ONE device call per local device on
 * its union with one record stream that is all or nothing there and marks its cells for the
 * next solve, stats (may be NULL) summed over the local devices, no collective, and every
 * message names the graph and the graph-local id. No supply changes, so no sink's demand
 * moves, and evicted tasks stay task nodes: the rows of ks_batch_gather keep their length.
 * A live resource's slot count changing (UpdateResourceTopology) is, on a batch,
 * ks_batch_update_nodes on the PU → sink arc followed by ks_batch_complete_tasks with every
 * k == 0 and KS_COMPLETE_RESOURCE_CAPS [| KS_COMPLETE_PREEMPTIVE]: the lone recipe of
 * ks_update_nodes, call for call. */
typedef struct ks_batch_res_list {   /* one graph's part of a call, in the graph's OWN ids */
    const uint64_t*    roots; size_t k;     /* ks_batch_remove_resources; k == 0: untouched        */
    const ks_res_node* nodes; size_t n;     /* ks_batch_add_resources; n == 0 && m == 0: untouched */
    const ks_res_arc*  arcs;  size_t m;
} ks_batch_res_list;

/* ks_remove_resources per listed graph (only roots / k of each entry are read). flags:
 * KS_REMOVE_* with the lone call's rules; the capacity BFS starts from every cell's sink,
 * as in the batch commits. A root that is 0 or beyond 1..span of its graph is KS_E_RANGE
 * before any device is asked; a root that is dead, a task or a sink keeps the lone call's
 * KS_E_INVALID. removed receives graph-local ids grouped by graph in ascending graph order
 * and ascending within a graph; removed_off (ngraphs + 1 entries, may be NULL) delimits
 * them: removed_off[g] .. removed_off[g + 1] is graph g's part, empty for a graph this rank
 * does not own. evicted receives one KS_DELTA_PREEMPT per evicted task (graph, graph-local
 * task, the graph-local PU it leaves), grouped by graph and in task order within a graph.
 * removed == NULL && evicted == NULL: a probe, the counts only and nothing changes. With
 * several local devices every device is probed first, so a buffer that is too small
 * (KS_E_INVALID, both counts written) or a root that any device refuses changes no device. */
int ks_batch_remove_resources(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_res_list* lists,
                              uint64_t* removed, size_t rcap, size_t* nremoved,
                              size_t* removed_off /* ngraphs + 1, may be NULL */,
                              ks_batch_delta* evicted, size_t ecap, size_t* nevicted,
                              ks_remove_stats* stats);
/* ks_add_resources per listed graph (only nodes / n and arcs / m of each entry are read).
 * flags is reserved: pass 0. The two 32-byte arrays go up back to back in graph order, as
 * the caller wrote them; one kernel range-checks every node id and both endpoints of every
 * edge against 1..span of the record's graph and moves them into the union's ids, so an edge
 * between two cells cannot be written. The first record in input order (nodes, then edges)
 * with an id outside its graph is KS_E_RANGE naming the graph, what the id was (node, parent
 * or child) and the id. A repeated (parent, child) pair is a repeat within one graph only.
 * Every new PU's arc ends at the sink of the PU's own cell (the per-cell sink table of the
 * task calls); a PU whose cell has no sink or several is KS_E_INVALID naming the graph, and
 * nothing changes. A new id may be any dead id of 1..span: a reserved one or a freed one.
 * After a growth with an edge, refresh the capacities as after ks_add_resources:
 * ks_batch_complete_tasks with every k == 0 and KS_COMPLETE_RESOURCE_CAPS. */
int ks_batch_add_resources(ks_batch* b, int32_t flags /* 0 */, size_t ngraphs, const ks_batch_res_list* lists,
                           ks_grow_stats* stats);

/* ---- batch rounds, class and resource arcs: the cost model's sweep ----------
 * The twin of ks_update_nodes on a batch, under the contract written above
 * ks_batch_task_list: one list per loaded graph on every rank (else KS_E_INVALID), every id
 * in its graph's OWN numbering, ONE device call per local device on its union with one record
 * stream that is all or nothing there and marks its cells for the next solve, stats (may be
 * NULL) summed over the local devices, no collective, and every message names the graph and
 * the graph-local id. With it the ten calls of a round (commit, remove, complete, add
 * resources, refresh, add tasks, update tasks, update nodes, costs, solve) all run on a batch,
 * and a caller whose class, rack or PU → sink costs move, or whose PUs change their slot
 * count, keeps no shadow of any cell's arcs.
 *
 * Refused on the host before any device is asked: a list count other than the loaded graphs,
 * an unknown flag bit, a null array where k > 0, arc_off[0] != 0, falling offsets, a null
 * arcs with arc_off[k] > 0 (all KS_E_INVALID); more than INT32_MAX / 4 tails or arcs per
 * graph or per device (KS_E_RANGE); and any tail outside 1..span of its graph (KS_E_RANGE),
 * which is checked for every local device first.
 *
 * The tails go into the union's ids on the host (O(k)). The 24-byte arcs go up as the caller
 * wrote them: one kernel range-checks every head against 1..span of the arc's graph and moves
 * it into the union's ids in place, so an arc from one cell into another cannot be written.
 * The first head in input order outside its graph is KS_E_RANGE naming the graph, the tail,
 * the head and the span; it is reported before the device's other refusals, as in
 * ks_batch_update_tasks, and nothing changes. Every other refusal (a dead tail, a task or
 * sink tail, a tail listed twice, an illegal head, a repeated head for one tail, a cost or a
 * capacity out of range, KS_CAP_KEEP on an arc the store does not hold, a capacity below a
 * lower bound) keeps the lone call's status code and the lone call's order within a device.
 * A tail listed twice is twice within one graph: the same local id in two graphs is two tails.
 *
 * With several local devices the call is all or nothing PER DEVICE, as in
 * ks_batch_update_tasks: the devices are asked in order, and a later device's refusal does
 * not undo the stream an earlier device has applied. No supply moves, so no auto-sink record
 * follows and the rows of ks_batch_gather keep their length. A call whose lists are all empty,
 * or that generates no record on a device, keeps that device's solution and mapping and marks
 * no cell. */
typedef struct ks_batch_node_list {   /* one graph's part of the call, in the graph's OWN ids */
    const uint64_t*    nodes;  size_t k;    /* the tails; k == 0: the graph is untouched */
    const uint64_t*    arc_off;             /* k + 1, as ks_update_nodes                 */
    const ks_node_arc* arcs;
} ks_batch_node_list;

int ks_batch_update_nodes(ks_batch* b, int32_t flags /* KS_NODES_KEEP_UNLISTED or 0 */,
                          size_t ngraphs, const ks_batch_node_list* lists, ks_node_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSMCMF_H */
