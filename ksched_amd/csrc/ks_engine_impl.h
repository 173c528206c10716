// ks_engine_impl.h — what the engine's translation units share (internal: included
// only by ks_engine.hip, ks_engine_build.hip, ks_engine_io.hip and ks_engine_sched.hip).
// The constants, the control block, the device view of the graph (DG), the owning
// device buffer (DBuf) and the engine's whole host state (EngineImpl). Kernels and
// the device helpers only they use live in the source that launches them.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ks_cell.h"
#include "ks_engine.h"
#include "ks_sched.h"

namespace ks {
namespace impl {

constexpr int BLK = 256;
constexpr int WAVE = 64;
constexpr int WPB = BLK / WAVE;
constexpr int NGC = 6;             // group classes: 4, 8, 16, 32, 64 lanes; 64 lanes × several chunks
constexpr int HEAVY_MIN = 4096;    // degree > 4096: hub, chunked over workgroups
constexpr int CHUNK = 1024;        // heavy hubs: 1024 residual arcs per workgroup
constexpr int PER_T = CHUNK / 256; // arcs per thread in a hub chunk
constexpr int HSPLIT = 4;          // Bellman-Ford: workgroups per hub chunk (one arc per thread at 4)
constexpr int BF_PER_T = PER_T / HSPLIT;
static_assert(PER_T % HSPLIT == 0, "a hub chunk splits into whole arcs per thread");
#ifndef KS_WPW
#define KS_WPW 2
#endif
constexpr int WPW = KS_WPW;        // windows per wave in sparse (grid-stride) passes (-DKS_WPW: tuning builds)
constexpr int SHARDS = 16;         // inbox shards per heavy hub
constexpr int MAXB = 64;           // max sweeps per cycle
constexpr int HUB_LDS = 16;        // hubs whose Bellman-Ford minima are reduced in LDS
constexpr int CYC_SLOTS = 2;       // control snapshots / timing events rotate over two cycles
constexpr int NCTR = 10;
constexpr int CTR_SHARDS = 64;
constexpr long long INF64 = 0x3fffffffffffffffLL;
constexpr long long LEN_CAP = 1LL << 40;   // global-update arc length clamp
constexpr double kSolveWallLimitS = 120.0; // host-side guard against a non-converging solve
constexpr double kCellLimitS = 20.0;       // the cell solver's in-kernel wall-clock limit (every workgroup exits)

enum { C_SCAN = 0, C_VISIT = 1, C_PUSH = 2, C_RELABEL = 3, C_GUSCAN = 4, C_BFROUND = 5, C_AUGWALK = 6, C_AUGHOP = 7,
       C_FSSCAN = 8, C_GULEAF = 9 };
constexpr int AUG_KMAX = 4096;     // most excess nodes a tail's walkers start from (ks_opts.tail_nodes)
constexpr int BX_CAP = 64;         // global updates with at most this many excess nodes are bounded
// Forward tail update: a node's search key (in its record's dist slot) packs the
// distance from the excess nodes above the position of the arc that set it.
constexpr int FS_PB = 26;
constexpr long long FS_NONE = (1LL << FS_PB) - 1;    // no parent (an excess node)
constexpr long long FS_DMAX = 1LL << 36;             // distances beyond are not searched
constexpr int FDEF_CAP = 64;       // deficits one forward update traces paths to
constexpr int FS_LIST_BLOCKS = 128;
constexpr int FWD_UPD = 4;         // forward updates per cycle once a search finished within its rounds (2: ~1 ms slower on config 4)

struct Ctl {
    long long eps;
    double inv;            // 1.0 / eps, computed on the host (ks_len.h); every writer of eps sets inv and lim too
    long long gu_L;        // max finite distance of the current global update
    long long gu_X;        // max distance of a node holding excess (−1: none)
    int infeasible;
    int bf_done;           // Bellman-Ford frontier drained (update converged)
    int verify_bad;
    int cp_bad;            // k_pack_pos: a value the 16-B record cannot hold (the solve reads Pos)
    int cyc_done;          // cycle-cancelling refinement: cycles cancelled
    int cyc_rej;           //   marked nodes k_cyc_check found with other than one member pointing at them
    int bf_count;          // Bellman-Ford rounds that did work (whole solve)
    int bfa[3];            // Bellman-Ford flag buffer k holds at least one flag
    int apply_act;         // the global-update apply seeded a non-empty frontier
    int sweep_act[MAXB];   // sweep pos left a non-empty frontier
    int gu_pending;        // the last cycle's update did not converge: the next cycle continues it
    int n_exc;             // nodes the last apply found holding excess
    int bf_r0;             // bf_count when the running update started
    int bf_seq0;           // sequence number of the running update's first (dense) round
    int aug_reached;       // walks of this cycle that reached a deficit / stopped short
    int aug_short;
    int n_xl2;             // nodes fed by this cycle's hub distribution
    int dbg_x[4];          // diagnostics (KS_CYCLE_LOG): the first listed excess nodes, their excess at the apply
    int dbg_e[4];
    int n_bx;              // excess nodes k_gu_init listed for the distance bound (> BX_CAP: no bound)
    long long bf_bound;    // Bellman-Ford prune bound: max tentative distance of the listed excess nodes
    long long gu_B;        // the converged bounded update's cap: max distance of the listed excess nodes
    // forward tail update (k_fs_*): a search from the excess nodes
    long long fs_D;        // least distance of a deficit found by the running search (INF64: none yet)
    int fs_cnt[3];         // frontier list lengths (rotating like the flag buffers)
    int fs_done;           // the search's frontier drained
    int fs_fail;           // list overflow or no deficit in range: the next cycle is a backward update
    int fs_pending;        // a search is running: the next init continues it (set by its first round)
    int fs_rounds;         // rounds of the running search that had a frontier
    int n_fdef;            // deficits at distance D listed for the trace
    int fs_moved;          // units the trace moved
    long long u_exc;       // excess units the last apply (backward) / init (forward) found
    int fs_maxcnt;         // the running search's widest frontier (nodes; hubs count 1024 each)
    int n_exc_rep;         // excess nodes / units the last completed forward update's init found
    long long u_exc_rep;
    int fs_completed;      // forward updates completed (whole solve)
    int fs_moved_cyc;      // units the traces of this cycle moved
    // device-clock timing (s_memrealtime, 100 MHz) where a HIP event between two
    // kernels would cost a ~5.7 µs gap of its own (profiles/r06_*_gaps):
    unsigned long long t_sw0;       // the cycle's first sweep started
    unsigned long long t_end;       // k_cycle_end started (= the last sweep ended)
    unsigned long long t_srch;      // the finish's running parent-graph search started (0: none)
    unsigned long long srch_ticks;  // the finish's searches so far (subtracted from its batches' spans)
    long long lim;         // (1 << 60) / eps: distances ε multiplies without overflowing a price (the applies)
};

struct HItem {
    int node, hid, begin, end;
};

__host__ __device__ constexpr int class_lanes(int c) { return c < 4 ? (4 << c) : 64; }
__host__ __device__ inline int degree_class(int d) {
    return d <= 4 ? 0 : d <= 8 ? 1 : d <= 16 ? 2 : d <= 32 ? 3 : d <= 64 ? 4 : d <= HEAVY_MIN ? 5 : NGC;
}
constexpr int CCLS = 5;            // chunked class: Bellman-Ford splits its nodes into 64-arc waves

struct CItem {                     // one 64-arc chunk of a chunked-class node
    int node, begin, end, lead;    // lead = 1 for the node's first chunk
};
// A wave owns one window: win_batches(c) batches of 64/G consecutive node ids.
// classes below 4 (≤ 16 lanes per node) own two batches per window, the rest one
__host__ __device__ constexpr int win_batches(int c) { return c < 4 ? 2 : 1; }
static_assert(NGC == 6, "KS_BY_CLASS dispatches six classes");
__host__ __device__ constexpr int win_slots(int c) { return win_batches(c) * (64 / class_lanes(c)); }

// One frontier buffer: a flag byte per (non-hub) node, a flag per hub.
struct Front {
    unsigned char* flag;   // [hub_base]
    int* hub;              // [nheavy]
};

struct DG {
    int n;                 // internal node ids: [0, hub_base) grouped nodes, then hubs
    int m;                 // always 0, read by no kernel (kept: dropping it moves every kernel's arguments)
    int hub_base;
    int expand;            // Bellman-Ford: relax low-degree targets two hops per round
    const int* first;
    Pos* pos;              // residual positions: cost, rcap, ucap = rcap(a) + rcap(rev a), head, rev
    CPos* cp;              // compact solve: 16-B copies of the positions (nullptr: the solve reads pos)
    int* crev;             // compact solve: reverse position of each position
    long long* excess;
    long long* p0;         // node records (stride 4, index with ni()): p0 at +0, dist at +1, p1 at +2
    long long* p1;
    long long* dist;
    long long* inbox;
    int wbeg[NGC + 1];     // windows of class c: [wbeg[c], wbeg[c+1])
    int obeg[NGC + 1];     // first node id of class c
    int oend[NGC];         // one past the last real node of class c
    const HItem* hitems;
    int nhitems;
    int nheavy;
    const CItem* citems;   // chunks of the chunked class
    int ncitems;
    int ncls_c;            // nodes of the chunked class
    int sw_clsb;           // sweep blocks striding the class windows (after the hub blocks)
    const int* hnchunks;
    int* xl;               // excess nodes listed by the last apply (the first aug_k)
    int aug_k;             // a phase's tail: ≤ aug_k excess nodes (ks_opts.tail_nodes)
    int* xl2;              // nodes fed by k_aug_hub (the first AUG_K2)
    int* bx;               // excess nodes of the running update (the first BX_CAP; k_gu_init)
    int* fl;               // forward search: 3 rotating frontier lists of fl_cap node ids
    int fl_cap;
    int fs_wide;           // a forward frontier wider than this fails its search as wide
    int npos;              // residual positions (m2cap)
    int* fdef;             // forward search: deficits at the found distance (FDEF_CAP)
    int bound;             // 1: prune Bellman-Ford offers at ctl->bf_bound (ks_opts.bf_bound >= 0)
    long long* aug_req;    // per hub: excess claimed by its k_aug_hub chunks
    long long* q_req;      // claim slots: hubs [0, nheavy), then chunked nodes
    long long* q_taken;
    long long* q_min;
    int* q_unsat;
    int* q_arrive;
    Front sf[3];   // sweep frontiers
    Front bf[3];   // Bellman-Ford frontiers
    Ctl* ctl;
    unsigned long long* ctr;
};

// Node records: p0, dist, p1 and the node's segment bounds (first[x], first[x+1]
// packed) share one 32-B record, so a Bellman-Ford tail gather (price, distance,
// and a leaf's segment) or a sweep's node load (price, segment) is one cache line.
__host__ __device__ __forceinline__ size_t ni(long long x) { return 4 * (size_t)x; }
constexpr int ND_SEG = 3;   // record slot of the packed segment bounds

// (the one atomic the build's and the outputs' kernels use too; the rest are the solve's)
__device__ __forceinline__ void atom_add(long long* p, long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================ host helpers ===
inline int grid_for(long long n, int cap = 4096) {
    long long b = (n + BLK - 1) / BLK;
    if (b < 1) b = 1;
    return (int)std::min<long long>(b, cap);
}

template <typename T>
struct DBuf {   // an owning device allocation (freed with its owner)
    T* p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { release(); }
    hipError_t ensure(size_t k) {
        if (k <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        size_t want = std::max<size_t>(k, 1);
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    // grow to ≥ k elements keeping the first `keep` ones; new tail bytes = fill
    hipError_t grow(size_t k, size_t keep, int fill, hipStream_t st) {
        if (k <= n && p) return hipSuccess;
        const size_t want = std::max<size_t>(k, 1);
        T* q = nullptr;
        hipError_t e = hipMalloc(&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        keep = std::min(keep, n);
        if (keep && p) e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(q + keep, fill, (want - keep) * sizeof(T), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (p) (void)hipFree(p);
        p = q;
        n = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

}  // namespace impl
using namespace impl;

struct EngineImpl {
    int device = 0;
    ks_opts opts{};
    hipStream_t stream = nullptr;
    // [0] solve start, [1] build / reset done, [2] phase start, [3] saturate done,
    // [4] phase end, [5]/[6] around a refinement and around verification
    hipEvent_t ev[7] = {};
    hipEvent_t kev[4] = {};   // kernel-batch timing (price refinement)
    hipEvent_t fin_ev[4] = {};      // the finish's pipelined batches: [3] its start, [b % 3] batch b's end
    // per-cycle timing: [0] before the first Bellman-Ford round, [1] after the last (the
    // sweeps: device clock); forward cycles: [2u]/[2u+1] around update u's search rounds (fev)
    hipEvent_t cev[CYC_SLOTS][2] = {};
    hipEvent_t fev[CYC_SLOTS][8] = {};
    hipEvent_t cdone[CYC_SLOTS] = {};   // a cycle's control snapshot has landed (timed: cycle end)
    Ctl* h_cyc[CYC_SLOTS] = {};         // pinned control snapshots of the cycles in flight
    Ctl* d_cyc[CYC_SLOTS] = {};         // their device-side addresses (written by k_cycle_end)

    // ---- node store (by slot = id − 1)
    int64_t nstore = 0;       // allocated slots
    int64_t nslots = 0;       // slots in use (max id)
    DBuf<long long> n_supply;
    DBuf<unsigned char> n_type, n_alive, n_fresh;
    DBuf<unsigned long long> n_cshift;   // per slot: cost rise on a flow-carrying out-arc (warm start)
    DBuf<int> n_lastrm;
    DBuf<int> n_hint;         // per slot: segment capacity of the last build
    DBuf<unsigned char> n_grow;
    DBuf<unsigned long long> n_bind;   // per slot: bound PU (scheduling deltas)
    // ---- arc table (by slot) and its hash index
    int64_t acap = 0;
    DBuf<int> a_src, a_dst, fwd, free_stack;
    DBuf<long long> a_low, a_cap, a_cost;
    DBuf<unsigned char> a_alive, a_type;
    int64_t hcap = 0;
    DBuf<unsigned long long> hkey;
    DBuf<int> hval, hlast;
    DBuf<StoreCtl> sctl;
    StoreCtl* h_sctl = nullptr;   // pinned mirror
    DBuf<ks_delta> d_recs;
    DBuf<NodeEdit> d_edits;
    DBuf<int> rec_ent;
    // ---- residual CSR built from the table (internal ids)
    bool csr_valid = false;   // CSR matches the table (deltas applied in place)
    bool incremental = false; // deltas seen since the load: rebuild with slack
    int64_t rebuilds = 0;     // CSR builds since the load
    int64_t ncap = 0;         // node slots covered by the build
    long long mult = 1;       // cost multiplier (ncap + 1)
    int64_t m2cap = 0;        // residual positions (Σ segment capacities)
    DBuf<int> first, ent, used, scur, perm, iperm;
    DBuf<Pos> pos;
    DBuf<CPos> cpos;               // the compact solve's 16-B positions (k_pack_pos)
    DBuf<int> crev;
    DBuf<int> cyc;                 // cycle-cancelling refinement: parents, doubling buffers, marks, arcs
    DBuf<long long> cyc64;         //   and per-group cost sums and bottlenecks
    DBuf<long long> excess;
    DBuf<long long> nd;            // node records [p0, dist, p1, pad] × nn
    DBuf<unsigned> keys_in, keys_out;
    DBuf<int> vals_in, vals_out, pos_of, deg, capv, capi, rs;
    DBuf<unsigned char> sort_tmp, cls;
    DBuf<int> nsel;
    DBuf<int> cls_list[NGC + 1];   // node slots of each degree class; [NGC] = heavy hubs
    DBuf<unsigned char> sel_tmp;
    DBuf<HItem> hitems;
    DBuf<CItem> citems;
    DBuf<int> hnchunks, q_unsat, q_arrive;
    DBuf<long long> q_req, q_taken, q_min, inbox, part, flows;
    DBuf<long long> vbal;               // verification: per-node balance of the arc flows (input slots)
    DBuf<unsigned char> flags;   // 6 frontier buffers × hub_base
    DBuf<int> hubflags;          // 6 × nheavy
    DBuf<unsigned long long> ctr;
    DBuf<int> xl, xl2;                 // walker start nodes (k_augment)
    DBuf<int> bx;                      // excess nodes of the running update (distance bound)
    DBuf<int> fl, fdef;                // forward tail update: frontier lists, traced deficits
    DBuf<long long> aug_req;           // per hub claim counter (k_aug_hub)
    DBuf<Ctl> ctl;
    Ctl* h_ctl = nullptr;        // pinned host mirror
    int ncls[NGC + 1] = {0};
    int nheavy = 0, nhitems = 0, ncitems = 0;
    int hub_base = 0, nn = 0;    // grouped node ids [0, hub_base), hubs after: nn ids
    int obeg[NGC + 1] = {0}, oend[NGC] = {0}, wbeg[NGC + 1] = {0};
    // ---- solution
    bool solved = false;         // flows/prices of the current graph are optimal
    bool has_prev = false;       // a solution exists in place (warm start possible)
    DBuf<long long> saved_flows, p_slot;
    DBuf<long long> map_outv, map_inv, map_outs, map_ins;
    DBuf<int> map_rank, map_is_task, flow_sel, flow_cnt;
    DBuf<unsigned char> map_itype, map_tmp;
    DBuf<uint64_t> map_scratch;  // device vector behind ks_get_task_mapping
    DBuf<ks_flow> flow_recs;
    // ---- cell solver (ks_cell.h): one workgroup per small graph
    bool cell_layout = false;           // the CSR was built cell-major (the cell solver's node order)
    std::vector<int64_t> cell_off;      // node-id partition into independent cells (ks_batch); empty: one
    std::vector<CellDesc> h_cells;      // per cell: its class bounds in internal ids
    int cell_max = 0;                   // largest cell (node slots)
    DBuf<CellDesc> cells;
    DBuf<int> cl_lists, cl_rln;
    DBuf<long long> cl_rlp;
    DBuf<CellOut> cl_out;
    DBuf<CellPos> cl_pos;               // compact positions (k_cell_pack / k_cell_unpack)
    DBuf<int> cl_bad;
    bool cell_refused = false;          // the cell solver handed this graph to the engine: engine until a reload,
    bool cell_refused_values = false;   //   or, when a value did not fit the compact record, until arcs change
    size_t lds_limit = 0;               // the device's opt-in LDS per workgroup (sizes the cells)
    bool fb_active = false;             // a per-cell fallback solve is running (engine order, failing cells cold)
    std::vector<int> fb_cells;          // the cells it re-solves
    DBuf<long long> fb_rng;             // their node-slot ranges on the device
    DBuf<unsigned long long> fb_cnt;    // arc + node slots k_fb_reset restarted cold
    std::vector<CellOut> h_cell_out;
    // which cells run: one flag per cell of a partition, set on the device over
    // every record stream that reaches store_apply and cleared by a successful solve
    std::vector<int> h_cell_first;      // the cells' first node slots (k + 1: the last one ends the partition)
    bool cell_first_valid = false;      // cell_first / cell_dirty hold the current partition
    DBuf<int> cell_first, cell_dirty;
    DBuf<int> cell_sink;                // a union's sink per cell (sched_cell_sinks), rebuilt by every call that reads it
    DBuf<int> cell_list;                // the cells of a partial launch
    std::vector<int> h_cell_dirty, h_cell_list;
    bool cells_kept = false;            // the last solve ended OK on the cell path and no build ran since:
                                        //   a cell no record touched still holds its optimum
    // ---- scheduler-side sweeps (ks_sched.hip)
    DBuf<int> sched_i;                  // int scratch
    DBuf<unsigned long long> sched_u;   // u64 scratch
    DBuf<unsigned char> sched_b;        // byte scratch
    DBuf<ks_sched_delta> sched_d;
    DBuf<int> cm_i;                     // ks_commit_schedule: places, chunk items, arc flags and their scans
    DBuf<unsigned long long> cm_u;      //   per node slot: aggregator / PU counts, slots and running below
    DBuf<unsigned char> cm_b;           //   per node slot: aggregator / placed flags
    DBuf<CommitCtl> cm_ctl;
    DBuf<RemoveCtl> rm_ctl;             // ks_remove_resources: its counters (the scratch is the commit's)
    DBuf<AddCtl> add_ctl;               // ks_add_tasks: its counters (the scratch is the commit's)
    DBuf<GrowCtl> grow_ctl;             // ks_add_resources: its counters (the scratch is the commit's)
    DBuf<UpdCtl> upd_ctl;               // ks_update_tasks: its counters (the scratch is the commit's)
    DBuf<NodCtl> nod_ctl;               // ks_update_nodes: its counters (the scratch is the commit's)

    SchedDev schd() const {
        SchedDev d{};
        d.ncap = (int)ncap;
        d.nstore = nstore;
        d.perm = perm.p;
        d.iperm = iperm.p;
        d.n_alive = n_alive.p;
        d.n_type = n_type.p;
        d.n_bind = n_bind.p;
        d.hi = h_sctl ? h_sctl->hi : 0;
        d.a_alive = a_alive.p;
        d.a_type = a_type.p;
        d.a_src = a_src.p;
        d.a_dst = a_dst.p;
        d.a_low = a_low.p;
        d.a_cap = a_cap.p;
        d.a_cost = a_cost.p;
        d.fwd = fwd.p;
        d.first = first.p;
        d.used = used.p;
        d.pos = pos.p;
        d.ent = ent.p;
        d.mult = mult;
        d.csr_valid = csr_valid ? 1 : 0;
        return d;
    }

    ~EngineImpl() {   // (the device buffers free themselves after this: the stream was synchronised)
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
        }
        if (h_ctl) (void)hipHostFree(h_ctl);
        for (auto* h : h_cyc)
            if (h) (void)hipHostFree(h);
        for (auto& c : cev)
            for (auto& e : c)
                if (e) (void)hipEventDestroy(e);
        for (auto& c : fev)
            for (auto& e : c)
                if (e) (void)hipEventDestroy(e);
        for (auto& e : cdone)
            if (e) (void)hipEventDestroy(e);
        if (h_sctl) (void)hipHostFree(h_sctl);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : kev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : fin_ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    StoreDev sd() const {
        StoreDev d{};
        d.ncap = (int)ncap;
        d.n_supply = n_supply.p;
        d.n_type = n_type.p;
        d.n_alive = n_alive.p;
        d.n_fresh = n_fresh.p;
        d.n_cshift = n_cshift.p;
        d.n_lastrm = n_lastrm.p;
        d.n_grow = n_grow.p;
        d.n_bind = n_bind.p;
        d.perm = perm.p;
        d.acap = (int)acap;
        d.a_src = a_src.p;
        d.a_dst = a_dst.p;
        d.a_low = a_low.p;
        d.a_cap = a_cap.p;
        d.a_cost = a_cost.p;
        d.a_type = a_type.p;
        d.a_alive = a_alive.p;
        d.fwd = fwd.p;
        d.free_stack = free_stack.p;
        d.hmask = (int)(hcap - 1);
        d.hkey = hkey.p;
        d.hval = hval.p;
        d.hlast = hlast.p;
        d.nn = nn;
        d.first = first.p;
        d.used = used.p;
        d.scur = scur.p;
        d.pos = pos.p;
        d.ent = ent.p;
        d.excess = excess.p;
        d.mult = mult;
        d.csr_valid = csr_valid ? 1 : 0;
        d.ctl = sctl.p;
        return d;
    }

    DG dg() const {
        DG g{};
        g.n = nn;
        g.m = 0;
        g.hub_base = hub_base;
        g.first = first.p;
        g.pos = pos.p;
        g.excess = excess.p;
        g.p0 = nd.p;
        g.p1 = nd.p ? nd.p + 2 : nullptr;
        g.dist = nd.p ? nd.p + 1 : nullptr;
        g.inbox = inbox.p;
        for (int c = 0; c <= NGC; ++c) {
            g.obeg[c] = obeg[c];
            g.wbeg[c] = wbeg[c];
        }
        for (int c = 0; c < NGC; ++c) g.oend[c] = oend[c];
        g.hitems = hitems.p;
        g.nhitems = nhitems;
        g.citems = citems.p;
        g.ncitems = ncitems;
        g.ncls_c = ncls[CCLS];
        g.sw_clsb = sweep_cls_blocks();
        g.nheavy = nheavy;
        g.hnchunks = hnchunks.p;
        g.xl = xl.p;
        g.xl2 = xl2.p;
        g.bx = bx.p;
        g.fl = fl.p;
        g.fl_cap = (int)(fl.n / 3);
        g.fdef = fdef.p;
        g.npos = (int)m2cap;
        g.aug_req = aug_req.p;
        g.q_req = q_req.p;
        g.q_taken = q_taken.p;
        g.q_min = q_min.p;
        g.q_unsat = q_unsat.p;
        g.q_arrive = q_arrive.p;
        const int hs = std::max(1, nheavy);
        const size_t fs = std::max(1, hub_base);
        for (int k = 0; k < 6; ++k) {
            Front f{flags.p + k * fs, hubflags.p + (size_t)k * hs};
            if (k < 3) g.sf[k] = f;
            else g.bf[k - 3] = f;
        }
        g.ctl = ctl.p;
        g.ctr = ctr.p;
        return g;
    }
    int window_grid() const { return nhitems + std::max(1, (wbeg[NGC] + WPB - 1) / WPB); }
    // Bellman-Ford rounds: HSPLIT workgroups per hub chunk, then the windows / chunk items
    int dense_grid() const { return nhitems * HSPLIT + std::max(1, (wbeg[CCLS] + ncitems + WPB - 1) / WPB); }
    int sweep_cls_blocks() const { return std::max(1, (wbeg[CCLS] + WPW * WPB - 1) / (WPW * WPB)); }
    // sweeps: hub chunks, class-window blocks, one wave per chunked-class node
    int sweep_grid() const {
        return nhitems + sweep_cls_blocks() + ncls[CCLS];
    }
    int sparse_grid() const {
        return nhitems * HSPLIT + std::max(1, (wbeg[CCLS] + ncitems + WPW * WPB - 1) / (WPW * WPB));
    }
    int hi() const { return h_sctl->hi; }
};

namespace impl {

// ks_engine_build.hip
int build(EngineImpl& s, std::string& err);        // the residual CSR from the arc table
int cold_reset(EngineImpl& s, std::string& err);   // zero flow, supplies with the lower-bound transform, zero prices
// ks_engine_io.hip: store glue the build and the scheduler's commit share
int ensure_nodes(EngineImpl& s, int64_t need, std::string& err);
int read_sctl(EngineImpl& s, std::string& err);
int ensure_arcs(EngineImpl& s, int64_t need, std::string& err);
int ensure_hash(EngineImpl& s, int64_t extra, std::string& err);
int applied(EngineImpl& s, std::string& err);
// cell_first / cell_dirty of the current partition on the device (a partition must exist)
int ensure_cell_first(EngineImpl& s, std::string& err);
// the cells a record stream (device memory) touches, before it reaches store_apply
int mark_cells(EngineImpl& s, const ks_delta* recs, size_t k, const NodeEdit* edits, size_t ne, std::string& err);
// the tail of a record stream generated on the device: room for nrec records in
// d_recs / rec_ent and nedits node edits in d_edits; then, the records emitted, the stream's way
// into the store
int size_stream(EngineImpl& s, int64_t nrec, size_t nedits, std::string& err);
int apply_stream(EngineImpl& s, int64_t nrec, const std::vector<NodeEdit>& edits, bool arc_recs, std::string& err,
                 hipEvent_t applied_ev = nullptr);

inline double ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.0;
    return ms;
}

}  // namespace impl

#define KS_CHECK(expr)                                                   \
    do {                                                                 \
        hipError_t _e = (expr);                                          \
        if (_e != hipSuccess) {                                          \
            err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            return KS_E_DEVICE;                                          \
        }                                                                \
    } while (0)

}  // namespace ks
