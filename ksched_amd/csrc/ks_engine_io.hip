// ks_engine_io.hip — the engine's store glue (load, deltas, node edits: ks_store.h)
// and its outputs with their kernels: the task → PU mapping, flows, arcs, per-cell
// sums, downloads.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ks_engine_impl.h"

namespace ks {
namespace {

// ================================================ task → PU mapping ===
// Path decomposition of the solved flow on device (replaces parseFlowToMapping,
// placement/solver.go:183-269). Flow units are numbered per node: the units
// leaving x are numbered along x's forward arcs in segment order (out prefix), the
// units entering y along y's reverse arcs (in prefix); unit k entering y leaves
// on y's k-th outgoing unit. A task's single unit is followed until it reaches a
// node without outflow (the sink); the last PU on the way is its placement.
__global__ void k_unit_vals(long long m2cap, const int* __restrict__ ent, const long long* __restrict__ flows,
                            long long* __restrict__ outv, long long* __restrict__ inv) {
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2cap; p += (long long)gridDim.x * BLK) {
        const int e = ent[p];
        const long long f = e >= 0 ? flows[e >> 1] : 0;
        outv[p] = (e >= 0 && !(e & 1)) ? f : 0;
        inv[p] = (e >= 0 && (e & 1)) ? f : 0;
    }
}

__global__ void k_node_meta(int ncap, const int* __restrict__ perm, const unsigned char* __restrict__ type,
                            const unsigned char* __restrict__ alive, unsigned char* __restrict__ itype,
                            int* __restrict__ is_task) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        const unsigned char t = alive[v] ? type[v] : 0;
        itype[perm[v]] = t;
        is_task[v] = t == KS_NODE_TASK ? 1 : 0;
    }
}

// smallest position p in [lo, hi) with pre[p] + val[p] > k (pre is the inclusive-
// exclusive pair of a scan: pre[p] = units before p within the segment)
__device__ __forceinline__ int find_unit(const long long* __restrict__ scan, const long long* __restrict__ val,
                                         int lo, int hi, long long base, long long k) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (scan[mid] - base + val[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void k_task_paths(int ncap, int nn, const int* __restrict__ perm, const int* __restrict__ first,
                             const Pos* __restrict__ pos,
                             const long long* __restrict__ outv, const long long* __restrict__ outs,
                             const long long* __restrict__ inv, const long long* __restrict__ ins,
                             const int* __restrict__ iperm, const unsigned char* __restrict__ itype,
                             const int* __restrict__ rank, const int* __restrict__ is_task, long long cap,
                             unsigned long long* __restrict__ out) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        if (!is_task[v]) continue;
        int x = perm[v];
        long long k = 0;   // unit index among x's outgoing units
        int last_pu = -1;
        for (int step = 0; step <= nn; ++step) {
            const int lo = first[x], hi = first[x + 1];
            if (lo >= hi) break;
            const long long obase = outs[lo];
            const long long otot = outs[hi - 1] + outv[hi - 1] - obase;
            if (k >= otot) break;   // absorbed here (no outflow left)
            const int p = find_unit(outs, outv, lo, hi, obase, k);
            const long long off = k - (outs[p] - obase);
            const int y = pos[p].head;
            if (itype[y] == KS_NODE_PU) last_pu = y;
            const int q = pos[p].rev;
            k = ins[q] - ins[first[y]] + off;
            x = y;
        }
        if (rank[v] < cap) out[rank[v]] = last_pu >= 0 ? (unsigned long long)iperm[last_pu] + 1 : 0ULL;
    }
}

// Per-partition cost and flow value of a disjoint union (k ≤ 1024 parts; one LDS
// accumulator per part and block, one atomic per part and block).
constexpr int MAX_CELLS = 1024;
__global__ void k_cell_sums(int hi, int k, const long long* __restrict__ off, const unsigned char* __restrict__ alive,
                            const int* __restrict__ src, const int* __restrict__ dst,
                            const long long* __restrict__ supply, const long long* __restrict__ cost,
                            const long long* __restrict__ flows, long long* __restrict__ out_cost,
                            long long* __restrict__ out_flow) {
    __shared__ long long sc[MAX_CELLS], sf[MAX_CELLS];
    for (int i = threadIdx.x; i < k; i += BLK) sc[i] = sf[i] = 0;
    __syncthreads();
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK) {
        if (!alive[s]) continue;
        const long long f = flows[s];
        if (!f) continue;
        const long long id = (long long)src[s] + 1;
        int lo = 0, hh = k;   // the part j with off[j] < id <= off[j+1]
        while (hh - lo > 1) {
            const int mid = (lo + hh) >> 1;
            if (off[mid] < id) lo = mid; else hh = mid;
        }
        __hip_atomic_fetch_add(&sc[lo], f * cost[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        long long fv = 0;
        if (supply[dst[s]] < 0) fv += f;
        if (supply[src[s]] < 0) fv -= f;
        if (fv) __hip_atomic_fetch_add(&sf[lo], fv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += BLK) {
        if (sc[i]) atom_add(&out_cost[i], sc[i]);
        if (sf[i]) atom_add(&out_flow[i], sf[i]);
    }
}

struct SlotAlive {
    const unsigned char* alive;
    __host__ __device__ bool operator()(const int& s) const { return alive[s] != 0; }
};

__global__ void k_arc_records(int cnt, const int* __restrict__ sel, const int* __restrict__ src,
                              const int* __restrict__ dst, const long long* __restrict__ low,
                              const long long* __restrict__ cap, const long long* __restrict__ cost,
                              const unsigned char* __restrict__ type, ks_arc* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < cnt; i += (long long)gridDim.x * BLK) {
        const int s = sel[i];
        ks_arc a;
        a.src = (uint64_t)src[s] + 1;
        a.dst = (uint64_t)dst[s] + 1;
        a.low = (uint64_t)low[s];
        a.cap = (uint64_t)cap[s];
        a.cost = cost[s];
        a.type = type[s];
        a._pad = 0;
        out[i] = a;
    }
}

// positive-flow arcs of the last solve as "f" records (ks_flow), slot order
struct FlowPositive {
    const unsigned char* alive;
    const long long* flows;
    __host__ __device__ bool operator()(const int& s) const { return alive[s] && flows[s] > 0; }
};

__global__ void k_flow_records(int cnt, const int* __restrict__ sel, const int* __restrict__ src,
                               const int* __restrict__ dst, const long long* __restrict__ flows,
                               ks_flow* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < cnt; i += (long long)gridDim.x * BLK) {
        const int s = sel[i];
        out[i] = ks_flow{(uint64_t)src[s] + 1, (uint64_t)dst[s] + 1, flows[s]};
    }
}

// One flag per cell of a partition, set for every cell a record stream touches (DESIGN
// §3.5 "which cells run"). A record's node — an arc's tail: no arc crosses two cells — is
// bisected over the cells' first slots, as k_cell_pack bisects heads. The lanes of a
// wave then agree on their distinct cells and ONE lane per cell issues the atomic: a
// stream is grouped by graph, so a wave sets one or two words instead of sending 64
// atomics to the same one. Slots outside the partition (the store's spare
// slots) belong to no cell.
__global__ void k_mark_cells(const ks_delta* __restrict__ recs, int k, const NodeEdit* __restrict__ edits, int ne,
                             const int* __restrict__ first, int ncells, int* __restrict__ dirty) {
    const long long total = (long long)k + ne;
    const int lane = threadIdx.x & (WAVE - 1);
    // (i − lane is the wave's first index: the trip count is wave-uniform)
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i - lane < total; i += (long long)gridDim.x * BLK) {
        int cell = -1;
        if (i < total) {
            long long slot;
            if (i < k) {
                const bool arc = recs[i].kind == KS_ADD_ARC || recs[i].kind == KS_UPDATE_ARC;
                slot = (long long)(arc ? recs[i].src : recs[i].id) - 1;
            } else {
                slot = edits[i - k].slot;
            }
            if (slot >= first[0] && slot < first[ncells]) {
                int lo = 0, hi = ncells;   // the last cell with first[cell] <= slot
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (first[mid] <= slot) lo = mid;
                    else hi = mid;
                }
                cell = lo;
            }
        }
        for (;;) {
            const unsigned long long m = __ballot(cell >= 0);
            if (!m) break;
            const int leader = __ffsll((long long)m) - 1;
            const int c = __shfl(cell, leader);
            if (lane == leader) atomicOr(&dirty[c], 1);
            if (cell == c) cell = -1;
        }
    }
}

}  // namespace

// The partition's first slots and its cleared dirty flags reach the device once per partition.
int impl::ensure_cell_first(EngineImpl& s, std::string& err) {
    if (s.cell_first_valid) return KS_OK;
    hipStream_t st = s.stream;
    const int ncells = (int)s.cell_off.size() - 1;
    s.h_cell_first.assign(s.cell_off.begin(), s.cell_off.end());   // cell i: slots [off[i], off[i+1])
    KS_CHECK(s.cell_first.ensure(ncells + 1));
    KS_CHECK(s.cell_dirty.ensure(ncells));
    KS_CHECK(hipMemcpyAsync(s.cell_first.p, s.h_cell_first.data(), (ncells + 1) * sizeof(int), hipMemcpyHostToDevice,
                            st));
    KS_CHECK(hipMemsetAsync(s.cell_dirty.p, 0, ncells * sizeof(int), st));
    KS_CHECK(hipStreamSynchronize(st));
    s.cell_first_valid = true;
    return KS_OK;
}

// The flags of k_mark_cells for a stream in device memory (the host's, uploaded by
// run_apply, or a commit's, generated there). Without a partition there is nothing to mark.
int impl::mark_cells(EngineImpl& s, const ks_delta* recs, size_t k, const NodeEdit* edits, size_t ne,
                     std::string& err) {
    if (s.cell_off.size() < 2 || k + ne == 0) return KS_OK;
    hipStream_t st = s.stream;
    const int ncells = (int)s.cell_off.size() - 1;
    if (int rc = ensure_cell_first(s, err)) return rc;
    hipLaunchKernelGGL(k_mark_cells, dim3(grid_for((long long)(k + ne), 1024)), dim3(BLK), 0, st, recs, (int)k, edits,
                       (int)ne, (const int*)s.cell_first.p, ncells, s.cell_dirty.p);
    KS_CHECK(hipGetLastError());
    return KS_OK;
}

// ------------------------------------------------------------------ store ---
int impl::read_sctl(EngineImpl& s, std::string& err) {
    KS_CHECK(hipMemcpyAsync(s.h_sctl, s.sctl.p, sizeof(StoreCtl), hipMemcpyDeviceToHost, s.stream));
    KS_CHECK(hipStreamSynchronize(s.stream));
    return KS_OK;
}

// Node store covers slots [0, need).
int impl::ensure_nodes(EngineImpl& s, int64_t need, std::string& err) {
    if (need <= s.nstore) return KS_OK;
    const int64_t cap = std::max<int64_t>(need + need / 8 + 64, 1024);
    hipStream_t st = s.stream;
    KS_CHECK(s.n_supply.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_type.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_alive.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_fresh.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_cshift.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_lastrm.grow(cap, s.nstore, 0xff, st));
    KS_CHECK(s.n_hint.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_grow.grow(cap, s.nstore, 0, st));
    KS_CHECK(s.n_bind.grow(cap, s.nstore, 0, st));
    s.nstore = cap;
    return KS_OK;
}

// Arc table holds slots [0, need).
int impl::ensure_arcs(EngineImpl& s, int64_t need, std::string& err) {
    if (need <= s.acap) return KS_OK;
    if (need >= (1LL << 30)) {
        err = "arc table beyond 2^30 slots";
        return KS_E_RANGE;
    }
    const int64_t cap = std::max<int64_t>(need + need / 4 + 64, 4096);
    hipStream_t st = s.stream;
    const int64_t keep = s.acap;
    KS_CHECK(s.a_src.grow(cap, keep, 0, st));
    KS_CHECK(s.a_dst.grow(cap, keep, 0, st));
    KS_CHECK(s.a_low.grow(cap, keep, 0, st));
    KS_CHECK(s.a_cap.grow(cap, keep, 0, st));
    KS_CHECK(s.a_cost.grow(cap, keep, 0, st));
    KS_CHECK(s.a_alive.grow(cap, keep, 0, st));
    KS_CHECK(s.a_type.grow(cap, keep, 0, st));
    KS_CHECK(s.fwd.grow(cap, keep, 0xff, st));
    KS_CHECK(s.free_stack.grow(cap, keep, 0, st));
    KS_CHECK(s.flows.grow(cap, keep, 0, st));
    s.acap = cap;
    return KS_OK;
}

// Hash index with room for `extra` more keys at load ≤ 1/2 (tombstones count).
int impl::ensure_hash(EngineImpl& s, int64_t extra, std::string& err) {
    const int64_t live = s.h_sctl->live, tombs = s.h_sctl->tombs;
    if (s.hcap && 2 * (live + tombs + extra) <= s.hcap) return KS_OK;
    int64_t cap = s.hcap ? s.hcap : 1024;
    while (cap < 4 * (live + extra) + 1024) cap <<= 1;
    if (cap > (1LL << 31)) {
        err = "hash index beyond 2^31 entries";
        return KS_E_RANGE;
    }
    KS_CHECK(s.hkey.ensure(cap));
    KS_CHECK(s.hval.ensure(cap));
    KS_CHECK(s.hlast.ensure(cap));
    s.hcap = cap;
    KS_CHECK(store_rehash(s.sd(), s.stream));
    return read_sctl(s, err);
}

// After store_apply and read_sctl: the store's overflow word.
int impl::applied(EngineImpl& s, std::string& err) {
    if (s.h_sctl->overflow & 12) {
        err = "store index or table exhausted";
        return KS_E_DEVICE;
    }
    if (s.h_sctl->overflow) {   // a full segment or a node beyond the build: rebuild from the table
        s.csr_valid = false;
        KS_CHECK(hipMemsetAsync(&s.sctl.p->overflow, 0, sizeof(int), s.stream));
        s.h_sctl->overflow = 0;
    }
    return KS_OK;
}

// Room for a stream generated on the device: nrec records and nedits node edits (no buffer
// below one element: store_apply takes the pointers of an empty stream too).
int impl::size_stream(EngineImpl& s, int64_t nrec, size_t nedits, std::string& err) {
    KS_CHECK(s.d_recs.ensure(std::max<size_t>(nrec, 1)));
    KS_CHECK(s.rec_ent.ensure(std::max<size_t>(nrec, 1)));
    KS_CHECK(s.d_edits.ensure(std::max<size_t>(nedits, 1)));
    return KS_OK;
}

// The nrec records a scheduler call emitted into d_recs reach the store: the host's node edits
// go up, the stream's cells are marked on the device (the records exist only there), store_apply
// runs, and ONE sync brings the store's counters. A failure in here leaves the device state
// unknown. arc_recs: the stream held arc records (costs or capacities changed, as in run_apply).
// applied_ev: recorded behind store_apply, before the sync (the commit's device span).
int impl::apply_stream(EngineImpl& s, int64_t nrec, const std::vector<NodeEdit>& edits, bool arc_recs,
                       std::string& err, hipEvent_t applied_ev) {
    hipStream_t st = s.stream;
    if (!edits.empty())
        KS_CHECK(hipMemcpyAsync(s.d_edits.p, edits.data(), edits.size() * sizeof(NodeEdit), hipMemcpyHostToDevice, st));
    int rc = mark_cells(s, s.d_recs.p, (size_t)nrec, s.d_edits.p, edits.size(), err);
    if (rc) return rc;
    KS_CHECK(store_apply(s.sd(), s.d_recs.p, (int)nrec, s.rec_ent.p, s.d_edits.p, (int)edits.size(), st));
    if (applied_ev) KS_CHECK(hipEventRecord(applied_ev, st));
    rc = read_sctl(s, err);
    if (rc == KS_OK) rc = applied(s, err);
    if (rc) return rc;
    s.incremental = true;
    s.solved = false;
    if (arc_recs && s.cell_refused_values) s.cell_refused = s.cell_refused_values = false;   // (as run_apply)
    return KS_OK;
}

static int run_apply(EngineImpl& s, const NodeEdit* edits, size_t ne, const ks_delta* recs, size_t k,
                     std::string& err) {
    hipStream_t st = s.stream;
    size_t narc = 0;
    for (size_t i = 0; i < k; ++i) narc += recs[i].kind == KS_ADD_ARC || recs[i].kind == KS_UPDATE_ARC;
    int rc = ensure_arcs(s, (int64_t)s.hi() + (int64_t)narc, err);
    if (rc == KS_OK) rc = ensure_hash(s, (int64_t)narc, err);
    if (rc) return rc;
    KS_CHECK(s.d_recs.ensure(std::max<size_t>(k, 1)));
    KS_CHECK(s.rec_ent.ensure(std::max<size_t>(k, 1)));
    KS_CHECK(s.d_edits.ensure(std::max<size_t>(ne, 1)));
    const auto t0 = std::chrono::steady_clock::now();
    if (k) KS_CHECK(hipMemcpyAsync(s.d_recs.p, recs, k * sizeof(ks_delta), hipMemcpyHostToDevice, st));
    if (ne) KS_CHECK(hipMemcpyAsync(s.d_edits.p, edits, ne * sizeof(NodeEdit), hipMemcpyHostToDevice, st));
    const auto t1 = std::chrono::steady_clock::now();
    rc = mark_cells(s, s.d_recs.p, k, s.d_edits.p, ne, err);
    if (rc) return rc;
    KS_CHECK(store_apply(s.sd(), s.d_recs.p, (int)k, s.rec_ent.p, s.d_edits.p, (int)ne, st));
    rc = read_sctl(s, err);
    if (rc) return rc;
    if (s.opts.log_cycles) {
        const auto t2 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "apply: upload call %.3f ms (%.1f MB), store kernels + wait %.3f ms\n",
                     std::chrono::duration<double, std::milli>(t1 - t0).count(),
                     1e-6 * (double)(k * sizeof(ks_delta) + ne * sizeof(NodeEdit)),
                     std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    rc = applied(s, err);
    if (rc) return rc;
    if (k || ne) s.solved = false;
    // costs or capacities changed: values that sent the cell solver's graph to the engine may
    // fit its record again (the next solve tries, and falls back once more if they do not)
    if (narc && s.cell_refused_values) s.cell_refused = s.cell_refused_values = false;
    return KS_OK;
}

int Engine::load(int64_t nslots, const int64_t* supply, const uint8_t* type, const uint8_t* alive, const ks_arc* arcs,
                 size_t m, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    if (nslots >= (1LL << 30) || m >= (1ULL << 29)) {
        err = "graph too large for 32-bit CSR indices";
        return KS_E_RANGE;
    }
    int rc = ensure_nodes(s, std::max<int64_t>(nslots, 1), err);
    if (rc) return rc;
    s.nslots = nslots;
    // empty store
    KS_CHECK(hipMemsetAsync(s.n_alive.p, 0, s.nstore, st));
    KS_CHECK(hipMemsetAsync(s.n_supply.p, 0, s.nstore * sizeof(long long), st));
    KS_CHECK(hipMemsetAsync(s.n_type.p, 0, s.nstore, st));
    KS_CHECK(hipMemsetAsync(s.n_fresh.p, 0, s.nstore, st));
    KS_CHECK(hipMemsetAsync(s.n_cshift.p, 0, s.nstore * sizeof(unsigned long long), st));
    KS_CHECK(hipMemsetAsync(s.n_hint.p, 0, s.nstore * sizeof(int), st));
    KS_CHECK(hipMemsetAsync(s.n_grow.p, 0, s.nstore, st));
    KS_CHECK(hipMemsetAsync(s.n_bind.p, 0, s.nstore * sizeof(unsigned long long), st));
    if (nslots) {
        KS_CHECK(hipMemcpyAsync(s.n_supply.p, supply, nslots * sizeof(long long), hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(s.n_type.p, type, nslots, hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(s.n_alive.p, alive, nslots, hipMemcpyHostToDevice, st));
    }
    if (s.acap) {
        KS_CHECK(hipMemsetAsync(s.a_alive.p, 0, s.acap, st));
        KS_CHECK(hipMemsetAsync(s.fwd.p, 0xff, s.acap * sizeof(int), st));
        KS_CHECK(hipMemsetAsync(s.a_low.p, 0, s.acap * sizeof(long long), st));
    }
    KS_CHECK(hipMemsetAsync(s.sctl.p, 0, sizeof(StoreCtl), st));
    std::memset(s.h_sctl, 0, sizeof(StoreCtl));
    s.csr_valid = false;
    s.incremental = false;
    s.rebuilds = 0;
    s.solved = false;
    s.has_prev = false;
    s.cells_kept = false;
    s.cell_refused = s.cell_refused_values = false;
    rc = ensure_arcs(s, (int64_t)m, err);
    if (rc) return rc;
    if (s.hcap) {   // clear the index (keeps its size)
        KS_CHECK(hipMemsetAsync(s.hkey.p, 0, s.hcap * sizeof(unsigned long long), st));
        KS_CHECK(hipMemsetAsync(s.hval.p, 0xff, s.hcap * sizeof(int), st));
        KS_CHECK(hipMemsetAsync(s.hlast.p, 0xff, s.hcap * sizeof(int), st));
    }
    // the arcs enter as ADD_ARC records of one stream (duplicates: the last wins)
    std::vector<ks_delta> recs(m);
    for (size_t i = 0; i < m; ++i) {
        ks_delta& d = recs[i];
        std::memset(&d, 0, sizeof(d));
        d.kind = KS_ADD_ARC;
        d.type = arcs[i].type;
        d.src = arcs[i].src;
        d.dst = arcs[i].dst;
        d.low = arcs[i].low;
        d.cap = arcs[i].cap;
        d.cost = arcs[i].cost;
    }
    return run_apply(s, nullptr, 0, recs.data(), m, err);
}

int Engine::apply(const NodeEdit* edits, size_t ne, const ks_delta* recs, size_t k, int64_t nslots,
                  std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    int rc = ensure_nodes(s, std::max<int64_t>(nslots, 1), err);
    if (rc) return rc;
    s.nslots = std::max(s.nslots, nslots);
    s.incremental = true;
    return run_apply(s, edits, ne, recs, k, err);
}

int64_t Engine::live_arcs() const { return p_->h_sctl ? p_->h_sctl->live : 0; }
bool Engine::solved() const { return p_->solved; }

void Engine::store_stats(ks_store_stats* o) const {
    const EngineImpl& s = *p_;
    std::memset(o, 0, sizeof(*o));
    if (!s.h_sctl) return;
    o->live_arcs = s.h_sctl->live;
    o->inserted = s.h_sctl->inserted;
    o->updated = s.h_sctl->updated;
    o->killed = s.h_sctl->killed;
    o->superseded = s.h_sctl->superseded;
    o->rebuilds = s.rebuilds;
    o->residual_slots = s.m2cap;
}

int Engine::set_nodes(const NodeEdit* edits, size_t ne, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    return run_apply(s, edits, ne, nullptr, 0, err);
}

int Engine::task_pu(uint64_t* dev_out, size_t cap, size_t* count, int64_t n_tasks, std::string& err) {
    EngineImpl& s = *p_;
    if (!s.solved) {
        err = "no successful solve";
        return KS_E_INVALID;
    }
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    *count = (size_t)n_tasks;
    if (!dev_out || cap < (size_t)n_tasks || n_tasks == 0) {
        if (dev_out && cap < (size_t)n_tasks) {
            err = "output buffer smaller than the task count";
            return KS_E_INVALID;
        }
        return KS_OK;
    }
    const int64_t m2 = std::max<int64_t>(s.m2cap, 1), ncap = s.ncap;
    const int nn = s.nn;
    KS_CHECK(s.map_outv.ensure(m2));
    KS_CHECK(s.map_inv.ensure(m2));
    KS_CHECK(s.map_outs.ensure(m2));
    KS_CHECK(s.map_ins.ensure(m2));
    KS_CHECK(s.map_itype.ensure(nn + 1));
    KS_CHECK(s.map_rank.ensure(ncap + 1));
    KS_CHECK(s.map_is_task.ensure(ncap + 1));
    KS_CHECK(hipMemsetAsync(s.map_itype.p, 0, nn + 1, st));
    if (s.m2cap)
        hipLaunchKernelGGL(k_unit_vals, dim3(grid_for(s.m2cap)), dim3(BLK), 0, st, (long long)s.m2cap,
                           (const int*)s.ent.p, (const long long*)s.flows.p, s.map_outv.p, s.map_inv.p);
    hipLaunchKernelGGL(k_node_meta, dim3(grid_for(ncap)), dim3(BLK), 0, st, (int)ncap, (const int*)s.perm.p,
                       (const unsigned char*)s.n_type.p, (const unsigned char*)s.n_alive.p, s.map_itype.p,
                       s.map_is_task.p);
    size_t t1 = 0, t2 = 0;
    if (s.m2cap) KS_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, s.map_outv.p, s.map_outs.p, (int)s.m2cap, st));
    KS_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, s.map_is_task.p, s.map_rank.p, (int)ncap, st));
    KS_CHECK(s.map_tmp.ensure(std::max(t1, t2)));
    size_t tt = s.map_tmp.n;
    if (s.m2cap) {
        KS_CHECK(hipcub::DeviceScan::ExclusiveSum(s.map_tmp.p, tt, s.map_outv.p, s.map_outs.p, (int)s.m2cap, st));
        tt = s.map_tmp.n;
        KS_CHECK(hipcub::DeviceScan::ExclusiveSum(s.map_tmp.p, tt, s.map_inv.p, s.map_ins.p, (int)s.m2cap, st));
    }
    tt = s.map_tmp.n;
    KS_CHECK(hipcub::DeviceScan::ExclusiveSum(s.map_tmp.p, tt, s.map_is_task.p, s.map_rank.p, (int)ncap, st));
    hipLaunchKernelGGL(k_task_paths, dim3(grid_for(ncap)), dim3(BLK), 0, st, (int)ncap, nn, (const int*)s.perm.p,
                       (const int*)s.first.p, (const Pos*)s.pos.p,
                       (const long long*)s.map_outv.p, (const long long*)s.map_outs.p,
                       (const long long*)s.map_inv.p, (const long long*)s.map_ins.p, (const int*)s.iperm.p,
                       (const unsigned char*)s.map_itype.p, (const int*)s.map_rank.p,
                       (const int*)s.map_is_task.p, (long long)cap, (unsigned long long*)dev_out);
    KS_CHECK(hipGetLastError());
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

int Engine::download(void* host_dst, const void* dev_src, size_t bytes, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    if (bytes) {
        KS_CHECK(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s.stream));
        KS_CHECK(hipStreamSynchronize(s.stream));
    }
    return KS_OK;
}

int Engine::scratch(uint64_t** dev, size_t n, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    KS_CHECK(s.map_scratch.ensure(std::max<size_t>(1, n)));
    *dev = s.map_scratch.p;
    return KS_OK;
}

int Engine::flows(std::vector<ks_flow>& out, std::string& err) {
    EngineImpl& s = *p_;
    if (!s.solved) {
        err = "no successful solve";
        return KS_E_INVALID;
    }
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const int hi = s.hi();
    out.clear();
    if (!hi) return KS_OK;
    KS_CHECK(s.flow_sel.ensure(hi));
    KS_CHECK(s.flow_cnt.ensure(1));
    hipcub::CountingInputIterator<int> it(0);
    FlowPositive pred{s.a_alive.p, s.flows.p};
    size_t t = 0;
    KS_CHECK(hipcub::DeviceSelect::If(nullptr, t, it, s.flow_sel.p, s.flow_cnt.p, hi, pred, st));
    KS_CHECK(s.map_tmp.ensure(std::max(t, s.map_tmp.n)));
    t = s.map_tmp.n;
    KS_CHECK(hipcub::DeviceSelect::If(s.map_tmp.p, t, it, s.flow_sel.p, s.flow_cnt.p, hi, pred, st));
    int cnt = 0;
    KS_CHECK(hipMemcpyAsync(&cnt, s.flow_cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    if (!cnt) return KS_OK;
    KS_CHECK(s.flow_recs.ensure(cnt));
    hipLaunchKernelGGL(k_flow_records, dim3(grid_for(cnt)), dim3(BLK), 0, st, cnt, (const int*)s.flow_sel.p,
                       (const int*)s.a_src.p, (const int*)s.a_dst.p, (const long long*)s.flows.p, s.flow_recs.p);
    out.resize(cnt);
    KS_CHECK(hipMemcpyAsync(out.data(), s.flow_recs.p, cnt * sizeof(ks_flow), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

int Engine::arcs(std::vector<ks_arc>& out, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const int hi = s.hi();
    out.clear();
    if (!hi) return KS_OK;
    KS_CHECK(s.flow_sel.ensure(hi));
    KS_CHECK(s.flow_cnt.ensure(1));
    hipcub::CountingInputIterator<int> it(0);
    SlotAlive pred{s.a_alive.p};
    size_t t = 0;
    KS_CHECK(hipcub::DeviceSelect::If(nullptr, t, it, s.flow_sel.p, s.flow_cnt.p, hi, pred, st));
    KS_CHECK(s.map_tmp.ensure(std::max(t, s.map_tmp.n)));
    t = s.map_tmp.n;
    KS_CHECK(hipcub::DeviceSelect::If(s.map_tmp.p, t, it, s.flow_sel.p, s.flow_cnt.p, hi, pred, st));
    int cnt = 0;
    KS_CHECK(hipMemcpyAsync(&cnt, s.flow_cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    if (!cnt) return KS_OK;
    ks_arc* d = nullptr;
    KS_CHECK(hipMalloc(&d, cnt * sizeof(ks_arc)));
    hipLaunchKernelGGL(k_arc_records, dim3(grid_for(cnt)), dim3(BLK), 0, st, cnt, (const int*)s.flow_sel.p,
                       (const int*)s.a_src.p, (const int*)s.a_dst.p, (const long long*)s.a_low.p,
                       (const long long*)s.a_cap.p, (const long long*)s.a_cost.p, (const unsigned char*)s.a_type.p, d);
    out.resize(cnt);
    hipError_t e = hipMemcpyAsync(out.data(), d, cnt * sizeof(ks_arc), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    KS_CHECK(e);
    return KS_OK;
}

hipStream_t Engine::stream() const { return p_->stream; }

int Engine::cell_sums(const int64_t* off, size_t k, int64_t* dev_cost, int64_t* dev_flow, std::string& err) {
    EngineImpl& s = *p_;
    if (!s.solved) {
        err = "no successful solve";
        return KS_E_INVALID;
    }
    if (k > (size_t)MAX_CELLS) {
        err = "more than 1024 graphs in one union";
        return KS_E_INVALID;
    }
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const int hi = s.hi();
    KS_CHECK(s.sched_u.ensure(k + 1));
    KS_CHECK(hipMemcpyAsync(s.sched_u.p, off, (k + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    KS_CHECK(hipMemsetAsync(dev_cost, 0, k * sizeof(int64_t), st));
    KS_CHECK(hipMemsetAsync(dev_flow, 0, k * sizeof(int64_t), st));
    if (hi && k)
        hipLaunchKernelGGL(k_cell_sums, dim3(grid_for(hi, 1024)), dim3(BLK), 0, st, hi, (int)k,
                           (const long long*)s.sched_u.p, (const unsigned char*)s.a_alive.p, (const int*)s.a_src.p,
                           (const int*)s.a_dst.p, (const long long*)s.n_supply.p, (const long long*)s.a_cost.p,
                           (const long long*)s.flows.p, (long long*)dev_cost, (long long*)dev_flow);
    KS_CHECK(hipGetLastError());
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

}  // namespace ks
