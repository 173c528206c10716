// ks_engine.hip — gfx950 ε-scaling push-relabel min-cost flow engine: the solve
// (Engine::solve → SolveRun) and every kernel it launches. The engine's other sources:
// ks_engine_build.hip (the residual CSR and the cold reset), ks_engine_io.hip (store
// glue, the task → PU mapping and the other outputs), ks_engine_sched.hip (scheduler
// glue); what they share is in ks_engine_impl.h.
//
// Replaces the Flowlessly solve behind ksched's placement.Solver
// (scheduling/flow/placement/solver.go:30-34, 60-90). Algorithm and data
// layout: DESIGN.md §3-§4. Summary:
//
//   build      Nodes are RENUMBERED internally: classed by residual degree into
//              lane GROUPS of 4/8/16/32/64 lanes per node (one residual arc per
//              lane: a node costs one short dependent chain, not a serial arc
//              loop), each class a contiguous id range padded to whole 64-node
//              blocks, heavy hubs (degree > 4096; cluster aggregator, sink) last.
//              The residual CSR over the new ids comes from a radix sort of the
//              2m (tail, slot) keys (hipcub over rocPRIM). Every arc also keeps
//              its pair capacity ucap = rcap(a) + rcap(rev a), so the reverse
//              residual is ucap − rcap (no gather) and a push is two stores.
//   phases     ε ← ε/α: saturate every residual arc with negative reduced cost,
//              then alternate a GLOBAL PRICE UPDATE (Bellman-Ford from the
//              deficits) with a short burst of push/relabel SWEEPS until no node
//              holds excess. Once ε is below a small fraction of a cost unit the
//              flow is tested by PRICE REFINEMENT at ε = 1 (Bellman-Ford on the
//              difference constraints of 1-optimality); success proves the flow
//              optimal and ends the solve early.
//   finish     (default) the final phase is replaced: the phase before it drains,
//              then the refinement's Bellman-Ford records each node's parent arc
//              (packed keys) and every 8 rounds the parent graph is searched by
//              pointer doubling; its negative cycles are cancelled in parallel
//              until the refinement certifies (k_cyc_*). A near-optimal
//              flow (config 4's churn rounds) takes the finish a phase earlier.
//   layout     the solve's hot kernels read 16-B compact positions (CPos + a
//              reverse array) when the graph's values fit 32 bits (PL<CP>).
//   frontier   sweeps and Bellman-Ford rounds only touch the ACTIVE frontier:
//              one flag byte per node (three rotating buffers) plus per-hub
//              flags. Producers store 1 (idempotent: no counters, no returning
//              atomics); a wave owns a window of one or two lane-group batches,
//              ballots its flags, clears what it reads and hands the active
//              nodes to its groups. Dense passes take every node.
//   sweep      every frontier node discharges once against a price SNAPSHOT
//              (double-buffered prices: read P[ni(q)], write P[ni(q^1)]); a node
//              relabels only if it saturated all of its own admissible arcs, and
//              the relabel also covers arcs that may gain residual capacity from
//              concurrent pushes in the same sweep (reduced cost in (0, ε]) —
//              ε-optimality without locks.
//   control    the host enqueues one CYCLE per round trip: [global-update init]
//              [k Bellman-Ford rounds] [max] [apply] [g sweeps]; kernels read
//              device-side flags and exit early once their stage is finished,
//              so a cycle costs one host synchronisation.
//   heavy hubs pushes into a hub are wave-aggregated into a 16-way sharded
//              inbox; hub chunks claim excess with a CAS and the last-arriving
//              chunk finalises the relabel. Bellman-Ford relaxations into a hub
//              are min-reduced in LDS per workgroup.
//   tail       once an update leaves ≤ 64 nodes with excess, each sends its
//              units down the update's distances (k_augment walks; k_aug_hub
//              hands a hub's excess on in parallel) instead of one hop per
//              sweep over dozens of cycles; the update itself is bounded at the
//              excess nodes' largest distance. In a coarse phase the tail runs
//              FORWARD updates instead (k_fs_*): a search from the excess nodes
//              to the nearest deficit, the successive-shortest-path dual step,
//              and one unit per deficit pushed back along the search's parent
//              arcs — no global recompute.
//   verify     on-device: conservation, capacity, and 1-optimality of the final
//              prices in scaled units (costs × (n+1), so 1-optimal ⇒ optimal);
//              the total cost is reduced in int64.
//
// All in-kernel cross-workgroup communication uses device-scope RMW atomics or
// idempotent flag stores; everything else is handed over at kernel boundaries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ks_engine_impl.h"
#include "ks_len.h"

namespace ks {
namespace {

__device__ __forceinline__ void seg_of(const long long* nd, int x, int& b0, int& b1) {
    const unsigned long long w = (unsigned long long)nd[ni(x) + ND_SEG];
    b0 = (int)(unsigned)(w & 0xffffffffULL);
    b1 = (int)(unsigned)(w >> 32);
}

// ---------------------------------------------------------------- atomics ---
__device__ __forceinline__ long long atom_add_ret(long long* p, long long v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ long long atom_exch(long long* p, long long v) {
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int atom_exch_i(int* p, int v) {
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ long long atom_min_ret(long long* p, long long v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void atom_min(long long* p, long long v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// excess and dist are only ever changed by atomics (performed beyond the issuing
// XCD's L2). Every load of them that hands data across workgroups or kernels is
// an agent-scope load: a plain load can hit a stale copy in another XCD's L2
// when a node's owner moves to a different XCD between launches (observed when
// several solves share the GPU: over-pushes, lost distance updates).
__device__ __forceinline__ long long atom_load(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int atom_load_i(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A wave-uniform 64-bit value that came from a vector load (one address for the
// whole wave), moved to scalar registers.
__device__ __forceinline__ long long uniform64(long long x) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)x & 0xffffffffULL));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void drain_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// One residual position (ks_pos.h) in two 16-byte loads issued together.
__device__ __forceinline__ Pos ld_pos(const Pos* p) {
    const longlong2 a = reinterpret_cast<const longlong2*>(p)[0];   // cost, rcap
    const longlong2 b = reinterpret_cast<const longlong2*>(p)[1];   // ucap, head | rev << 32
    Pos r;
    r.cost = a.x;
    r.rcap = a.y;
    r.ucap = b.x;
    r.head = (int)(unsigned)((unsigned long long)b.y & 0xffffffffULL);
    r.rev = (int)(unsigned)((unsigned long long)b.y >> 32);
    return r;
}

// Position access of the solve's hot kernels, by record layout:
// PL<false> reads the 32-B Pos records, PL<true> the 16-B CPos copies (32-bit
// residual, pair capacity, scaled cost, head) plus the separate reverse array.
// Every hot kernel is instantiated for both; the host launches the compact one when
// the graph's scaled costs and capacities fit 32 bits (ks_opts.compact_pos).
template <bool CP>
struct PL;
template <>
struct PL<false> {
    static __device__ __forceinline__ Pos ld(const DG& g, int a) { return ld_pos(g.pos + a); }
    // the record without its reverse position (Bellman-Ford): the same loads here
    static __device__ __forceinline__ Pos ld_nr(const DG& g, int a) { return ld_pos(g.pos + a); }
    static __device__ __forceinline__ void set_rc(const DG& g, int a, long long v) { g.pos[a].rcap = v; }
    static __device__ __forceinline__ long long rc_atomic(const DG& g, int a) { return atom_load(&g.pos[a].rcap); }
    static __device__ __forceinline__ bool cas_rc(const DG& g, int a, long long& exp, long long v) {
        return __hip_atomic_compare_exchange_strong(&g.pos[a].rcap, &exp, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void add_rc(const DG& g, int a, long long v) { atom_add(&g.pos[a].rcap, v); }
    static __device__ __forceinline__ int head(const DG& g, int a) { return g.pos[a].head; }
    static __device__ __forceinline__ int rev(const DG& g, int a) { return g.pos[a].rev; }
};
template <>
struct PL<true> {
    static __device__ __forceinline__ Pos ld(const DG& g, int a) {
        const int4 w = reinterpret_cast<const int4*>(g.cp)[a];
        const int rv = g.crev[a];   // issued with the record (independent address)
        Pos r;
        r.rcap = w.x;
        r.ucap = w.y;
        r.cost = w.z;   // CPOS_DEAD for inert positions: never residual, reduced cost > ε
        r.head = w.w;
        r.rev = rv;
        return r;
    }
    static __device__ __forceinline__ Pos ld_nr(const DG& g, int a) {
        const int4 w = reinterpret_cast<const int4*>(g.cp)[a];
        Pos r;
        r.rcap = w.x;
        r.ucap = w.y;
        r.cost = w.z;
        r.head = w.w;
        r.rev = -1;
        return r;
    }
    static __device__ __forceinline__ void set_rc(const DG& g, int a, long long v) { g.cp[a].rcap = (int)v; }
    static __device__ __forceinline__ long long rc_atomic(const DG& g, int a) {
        return __hip_atomic_load(&g.cp[a].rcap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ bool cas_rc(const DG& g, int a, long long& exp, long long v) {
        int e = (int)exp;
        const bool ok = __hip_atomic_compare_exchange_strong(&g.cp[a].rcap, &e, (int)v, __ATOMIC_RELAXED,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        exp = e;
        return ok;
    }
    static __device__ __forceinline__ void add_rc(const DG& g, int a, long long v) {
        __hip_atomic_fetch_add(&g.cp[a].rcap, (int)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ int head(const DG& g, int a) { return g.cp[a].head; }
    static __device__ __forceinline__ int rev(const DG& g, int a) { return g.crev[a]; }
};

// ------------------------------------------------------------ wave helpers ---
__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ long long wave_min(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (long long)__shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ long long wave_max(long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (long long)__shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ long long wave_incl_scan(long long x, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}
// Lane-group (G lanes, aligned) collectives.
template <int G>
__device__ __forceinline__ long long g_incl_scan(long long x) {
    const int l = lane_id() & (G - 1);
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        long long y = __shfl_up(x, o, G);
        if (l >= o) x += y;
    }
    return x;
}
template <int G>
__device__ __forceinline__ long long g_min(long long x) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) x = min(x, (long long)__shfl_xor(x, o, G));
    return x;
}
template <int G>
__device__ __forceinline__ long long g_sum(long long x) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, G);
    return x;
}

// Mark node w active in frontier f (idempotent plain stores).
__device__ __forceinline__ void mark(const DG& g, const Front& f, int w, int& out) {
    if (w >= g.hub_base) f.hub[w - g.hub_base] = 1;
    else f.flag[w] = 1;
    out = 1;
}

// Per-lane pending hub push: wave-aggregated into the hub's sharded inbox.
struct Pend {
    int key;
    long long val;
};

struct Cnt {
    long long scan = 0, visit = 0, push = 0, relabel = 0;
};

__device__ __forceinline__ void flush_counters(const DG& g, const Cnt& c) {
    const long long s = wave_sum(c.scan), v = wave_sum(c.visit), p = wave_sum(c.push),
                    r = wave_sum(c.relabel);
    if (lane_id() == 0 && (s | v | p | r)) {
        const int sh = ((blockIdx.x * WPB) + (threadIdx.x >> 6)) & (CTR_SHARDS - 1);
        unsigned long long* c0 = g.ctr + sh * NCTR;
        if (s) atomicAdd(c0 + C_SCAN, (unsigned long long)s);
        if (v) atomicAdd(c0 + C_VISIT, (unsigned long long)v);
        if (p) atomicAdd(c0 + C_PUSH, (unsigned long long)p);
        if (r) atomicAdd(c0 + C_RELABEL, (unsigned long long)r);
    }
}

// Push d units along arc a (v → w): residuals are two plain stores (only v's
// discharge writes the pair this sweep), the excess a fire-and-forget atomic.
// Non-hub heads are marked in nf (when given); hub pushes are buffered in pd
// and flagged once per wave in flush_pending.
// rv / uc: the arc's reverse position and pair capacity when the caller loaded
// them with the arc (rv < 0: load them here, one more dependent step).
template <bool CP>
__device__ __forceinline__ void push_arc(const DG& g, const Front* nf, int a, int w, long long r, long long d,
                                         Pend& pd, int& out, int rv, long long uc) {
    PL<CP>::set_rc(g, a, r - d);
    PL<CP>::set_rc(g, rv, uc - (r - d));
    if (w < g.hub_base) {
        atom_add(&g.excess[w], d);
        if (nf) {
            nf->flag[w] = 1;
            out = 1;
        }
        return;
    }
    const int h = w - g.hub_base;
    if (pd.key == h) {
        pd.val += d;
    } else if (pd.key < 0) {
        pd.key = h;
        pd.val = d;
    } else {
        atom_add(&g.inbox[h * SHARDS + (blockIdx.x & (SHARDS - 1))], d);
        if (nf) {
            nf->hub[h] = 1;
            out = 1;
        }
    }
}

// Must be called by all 64 lanes of a wave at a converged point.
__device__ __forceinline__ void flush_pending(const DG& g, const Front* nf, Pend& pd, int& out) {
    const int lane = lane_id();
    for (;;) {
        const unsigned long long msk = __ballot(pd.key >= 0);
        if (!msk) break;
        const int leader = __ffsll((long long)msk) - 1;
        const int k = __shfl(pd.key, leader);
        const long long s = wave_sum(pd.key == k ? pd.val : 0);
        if (lane == leader) {
            atom_add(&g.inbox[k * SHARDS + (blockIdx.x & (SHARDS - 1))], s);
            if (nf) {
                nf->hub[k] = 1;
                out = 1;
            }
        }
        if (pd.key == k) pd.key = -1;
    }
}

// Drain a hub's inbox shards into its excess. Returns the drained amount.
__device__ __forceinline__ long long drain_inbox(const DG& g, int h) {
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SHARDS; ++k) s += atom_exch(&g.inbox[h * SHARDS + k], 0LL);
    if (s) atom_add(&g.excess[g.hub_base + h], s);
    return s;
}

// ------------------------------------------------------------ block helpers ---
__device__ __forceinline__ long long block_sum(long long x, long long* sh) {
    x = wave_sum(x);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 0) sh[w] = x;
    __syncthreads();
    long long t = 0;
#pragma unroll
    for (int i = 0; i < WPB; ++i) t += sh[i];
    return t;
}
__device__ __forceinline__ long long block_min(long long x, long long* sh) {
    x = wave_min(x);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 0) sh[w] = x;
    __syncthreads();
    long long t = INF64;
#pragma unroll
    for (int i = 0; i < WPB; ++i) t = min(t, sh[i]);
    return t;
}
// exclusive scan across the block; returns exclusive prefix, *total = block total
__device__ __forceinline__ long long block_excl_scan(long long x, long long* sh, long long* total) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const long long incl = wave_incl_scan(x, lane);
    __syncthreads();
    if (lane == WAVE - 1) sh[w] = incl;
    __syncthreads();
    long long off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WPB; ++i) {
        if (i < w) off += sh[i];
        tot += sh[i];
    }
    *total = tot;
    return off + incl - x;
}

// --------------------------------------------------- frontier traversal ---
// A wave owns one window of class C. It ballots the window's flags (clearing
// what it reads; dense passes take every real node) and hands the active nodes
// to its G-lane groups one batch at a time. The loop trip count is wave-uniform,
// so the group code may use wave collectives.
#define KS_WINDOW(C, ARGS, W, ...)                                                   \
    {                                                                                \
        constexpr int G_ = class_lanes(C);                                           \
        constexpr int PER_ = 64 / G_;                                                \
        constexpr int WS_ = win_slots(C);                                            \
        const int base_ = g.obeg[C] + ((W) - g.wbeg[C]) * WS_;                       \
        const int ln_ = lane_id();                                                   \
        bool on_ = false;                                                            \
        if (ln_ < WS_) {                                                             \
            if ((ARGS).dense) {                                                      \
                on_ = base_ + ln_ < g.oend[C];                                       \
            } else {                                                                 \
                on_ = (ARGS).flags[base_ + ln_] != 0;                                \
                if (on_) (ARGS).flags[base_ + ln_] = 0;                              \
            }                                                                        \
        }                                                                            \
        unsigned long long mask_ = __ballot(on_);                                    \
        const int k_ = ln_ / G_;                                                     \
        while (mask_) {                                                              \
            unsigned long long mm_ = mask_;                                          \
            for (int j_ = 0; j_ < k_; ++j_) mm_ &= mm_ - 1;                          \
            const int v = mm_ ? base_ + __ffsll((long long)mm_) - 1 : -1;            \
            __VA_ARGS__;                                                             \
            for (int j_ = 0; j_ < PER_; ++j_) mask_ &= mask_ - 1;                    \
        }                                                                            \
    }
// Dispatch on the (wave-uniform) class of window IDX.
#define KS_BY_CLASS(IDX, ARGS, CALLT)                                                \
    {                                                                                \
        const int i_ = (IDX);                                                        \
        if (i_ < g.wbeg[1]) KS_WINDOW(0, ARGS, i_, CALLT(0))                         \
        else if (i_ < g.wbeg[2]) KS_WINDOW(1, ARGS, i_, CALLT(1))                    \
        else if (i_ < g.wbeg[3]) KS_WINDOW(2, ARGS, i_, CALLT(2))                    \
        else if (i_ < g.wbeg[4]) KS_WINDOW(3, ARGS, i_, CALLT(3))                    \
        else if (i_ < g.wbeg[5]) KS_WINDOW(4, ARGS, i_, CALLT(4))                    \
        else if (i_ < g.wbeg[6]) KS_WINDOW(5, ARGS, i_, CALLT(5))                    \
    }
struct Scan {
    unsigned char* flags;   // frontier flags to consume (sparse pass)
    int dense;              // 1: every node, flags ignored
};

__device__ __forceinline__ int wave_index_in_grid(int first_block) {
    return __builtin_amdgcn_readfirstlane(((int)blockIdx.x - first_block) * WPB + ((int)threadIdx.x >> 6));   // wave-uniform: a scalar register
}

// max |cost| over live arcs → *out (the first phase's ε).
__global__ void k_max_cost(int hi, const unsigned char* __restrict__ alive, const long long* __restrict__ cost,
                           long long* __restrict__ out) {
    long long mx = 0;
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK)
        if (alive[s]) mx = max(mx, cost[s] < 0 ? -cost[s] : cost[s]);
    // one atomic per workgroup (per-wave atomics on one address serialise)
    __shared__ long long sh[WPB];
    mx = wave_max(mx);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WPB; ++i) mx = max(mx, sh[i]);
        if (mx) __hip_atomic_fetch_max(out, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The compact solve (ks_opts.compact_pos): every position's 16-B copy
// and its reverse before the phases; a value a 32-bit field cannot hold sets *bad
// and the solve reads the 32-B records instead. The residuals go back before
// verification (k_unpack_pos).
__global__ void k_pack_pos(long long m2, const Pos* __restrict__ pos, CPos* __restrict__ cp, int* __restrict__ crev,
                           int* __restrict__ bad) {
    int b = 0;
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2; p += (long long)gridDim.x * BLK) {
        const Pos q = ld_pos(pos + p);
        const bool dead = q.cost >= DEAD_COST;
        b |= (!dead && (q.cost > CPOS_MAX || q.cost < -CPOS_MAX)) || q.rcap < 0 || q.rcap > CPOS_MAX || q.ucap < 0 ||
             q.ucap > CPOS_MAX;
        int4 w;
        w.x = (int)q.rcap;
        w.y = (int)q.ucap;
        w.z = dead ? CPOS_DEAD : (int)q.cost;
        w.w = q.head;
        reinterpret_cast<int4*>(cp)[p] = w;
        crev[p] = q.rev;
    }
    if (__any(b) && lane_id() == 0) atomicOr(bad, 1);
}
__global__ void k_unpack_pos(long long m2, const CPos* __restrict__ cp, Pos* __restrict__ pos) {
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2; p += (long long)gridDim.x * BLK)
        pos[p].rcap = cp[p].rcap;
}

// ================================================= saturate (phase start) ===
// Push the full residual capacity of every arc with negative reduced cost
// (Goldberg's refine start) over the whole graph; reads the authoritative p0.
template <int G, bool CP>
__device__ __forceinline__ void sat_group(const DG& g, int v, long long thr, Pend& pd, int& out, Cnt& c) {
    const long long* P = g.p0;
    const int lig = lane_id() & (G - 1);
    int b0 = 0, en = 0;
    long long pv = 0;
    if (v >= 0) {
        seg_of(g.p0, v, b0, en);
        pv = P[ni(v)];
    }
    const int iters = G < 64 ? 1 : (en - b0 + 63) / 64;   // G == 64: one node per wave
    long long tot = 0;
    for (int it = 0; it < iters; ++it) {
        const int a = b0 + it * G + lig;
        if (a < en) {
            const Pos q = PL<CP>::ld(g, a);
            const long long r = q.rcap;
            if (r > 0) {
                const int w = q.head;
                if (q.cost + pv - P[ni(w)] < -thr) {
                    push_arc<CP>(g, nullptr, a, w, r, r, pd, out, q.rev, q.ucap);
                    tot += r;
                    c.push++;
                }
            }
        }
        flush_pending(g, nullptr, pd, out);
    }
    tot = g_sum<G>(tot);
    if (v >= 0 && lig == 0 && tot) atom_add(&g.excess[v], -tot);
}

// thr = 0: Goldberg's refine start (every negative reduced cost); thr = ε on a
// warm start: only arcs that violate ε-optimality are saturated.
template <bool CP>
__global__ __launch_bounds__(BLK) void k_saturate(DG g, long long thr) {
    const long long* P = g.p0;
    Pend pd{-1, 0};
    Cnt c;
    int out = 0;
    if ((int)blockIdx.x < g.nhitems) {
        __shared__ long long sh[WPB];
        const HItem it = g.hitems[blockIdx.x];
        const long long px = P[ni(it.node)];
        long long tot = 0;
#pragma unroll
        for (int k = 0; k < PER_T; ++k) {
            const int a = it.begin + threadIdx.x * PER_T + k;
            if (a < it.end) {
                const Pos q = PL<CP>::ld(g, a);
                const long long r = q.rcap;
                if (r > 0) {
                    const int w = q.head;
                    if (q.cost + px - P[ni(w)] < -thr) {
                        push_arc<CP>(g, nullptr, a, w, r, r, pd, out, q.rev, q.ucap);
                        tot += r;
                        c.push++;
                    }
                }
            }
        }
        flush_pending(g, nullptr, pd, out);
        tot = block_sum(tot, sh);
        if (threadIdx.x == 0 && tot) atom_add(&g.excess[it.node], -tot);
        flush_counters(g, c);
        return;
    }
    const Scan sc{nullptr, 1};
#define KS_SAT_CALL(C) sat_group<G_, CP>(g, v, thr, pd, out, c)
    KS_BY_CLASS(wave_index_in_grid(g.nhitems), sc, KS_SAT_CALL)
#undef KS_SAT_CALL
    flush_pending(g, nullptr, pd, out);
    flush_counters(g, c);
}

// =================================================== push/relabel sweep ===
// One node per G-lane group, one residual arc per lane; admissible capacity is
// distributed by an in-group prefix sum, the relabel minimum by a group min.
template <int G, bool CP>
__device__ __forceinline__ void sweep_group(const DG& g, const Front& nf, int v, long long e, long long pv, int b0,
                                            int en, long long* __restrict__ PN, const long long* __restrict__ P,
                                            long long eps, Pend& pd, int& out, Cnt& c) {
    const int lig = lane_id() & (G - 1);
    if (v < 0) e = 0;
    const bool act = e > 0;
    if (!act) en = b0;
    if (act && lig == 0) c.visit++;
    long long rem = e, minc = INF64;
    const int iters = G < 64 ? 1 : (en - b0 + 63) / 64;   // G == 64: one node per wave
    for (int it = 0; it < iters; ++it) {
        const int a = b0 + it * G + lig;
        const bool valid = a < en;
        long long r = 0, cr = 0;
        int w = 0;
        int rv = 0;
        long long uc = 0;
        if (valid) {
            const Pos q = PL<CP>::ld(g, a);   // the whole record: a push needs no further load
            r = q.rcap;
            w = q.head;
            rv = q.rev;
            uc = q.ucap;
            cr = q.cost + pv - P[ni(w)];
            c.scan++;
        }
        const long long adm = (valid && cr < 0 && r > 0) ? r : 0;
        const long long incl = g_incl_scan<G>(adm);
        const long long total = __shfl(incl, G - 1, G);
        long long d = rem - (incl - adm);
        d = d < 0 ? 0 : (d > adm ? adm : d);
        if (d > 0) {
            push_arc<CP>(g, &nf, a, w, r, d, pd, out, rv, uc);
            c.push++;
        }
        if (valid) {
            if (cr < 0) {
                if (r - d > 0) minc = min(minc, cr);
            } else if (r > 0 || cr <= eps) {
                minc = min(minc, cr);
            }
        }
        rem -= total < rem ? total : rem;
        flush_pending(g, &nf, pd, out);
        if (G == 64 && rem == 0) break;
    }
    minc = g_min<G>(minc);
    if (act && lig == 0) {
        const long long pushed = e - rem;
        if (pushed) atom_add(&g.excess[v], -pushed);
        long long np = pv;
        if (rem > 0) {
            if (minc >= INF64) atomicOr(&g.ctl->infeasible, 1);
            else np = pv - (minc + eps);
            c.relabel++;
            nf.flag[v] = 1;   // still active next sweep
            out = 1;
        }
        PN[ni(v)] = np;
    }
}

// -------------------------------------------------- chunked claim protocol ---
// Hubs (one workgroup per 1024-arc chunk) discharge cooperatively. Every chunk reads the node's excess E
// once, requests its admissible capacity Ac with ONE returning atomicAdd on the
// node's request counter (no CAS loop), takes clamp(E − start, 0, Ac), pushes,
// and reports (taken, relabel minimum, unsaturated). The last-arriving chunk
// settles the node: subtracts what was taken, drains the hub inbox, relabels if
// every admissible arc was saturated and excess is left, and marks it active.
// Concurrent inflows only ever add excess, so Σ taken ≤ the excess present.
__device__ __forceinline__ long long claim(const DG& g, int slot, long long E, long long Ac) {
    if (Ac <= 0) return 0;
    const long long start = __hip_atomic_fetch_add(&g.q_req[slot], Ac, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long take = E - start;
    return take < 0 ? 0 : (take > Ac ? Ac : take);
}

// One lane per chunk. Returns nothing; settles the node when it arrives last.
__device__ __forceinline__ void settle(const DG& g, const Front& F, const Front& N, int slot, int x, int nch,
                                       bool hub, long long take, long long Ac, long long minc, long long px,
                                       long long* __restrict__ PN, long long eps, int& out, Cnt& c) {
    if (minc < INF64) atom_min(&g.q_min[slot], minc);
    if (take < Ac) atom_exch_i(&g.q_unsat[slot], 1);
    if (take) atom_add(&g.q_taken[slot], take);
    drain_vm();
    const int old = __hip_atomic_fetch_add(&g.q_arrive[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != nch - 1) return;
    // every returning atomic of the settle issued together (one round trip), then
    // one fetch-add applies the taken units and the drained inbox
    const long long mn = atom_exch(&g.q_min[slot], INF64);
    const int unsat = atom_exch_i(&g.q_unsat[slot], 0);
    const long long taken = atom_exch(&g.q_taken[slot], 0);
    atom_exch(&g.q_req[slot], 0LL);
    long long inflow = 0;
    if (hub) {
        long long* ib = &g.inbox[(x - g.hub_base) * SHARDS];
#pragma unroll
        for (int k = 0; k < SHARDS; ++k) inflow += atom_exch(&ib[k], 0LL);
    }
    const long long delta = inflow - taken;
    const long long now = (delta ? atom_add_ret(&g.excess[x], delta) : atom_load(&g.excess[x])) + delta;
    long long np = px;
    if (!unsat && now > 0) {
        if (mn >= INF64) atomicOr(&g.ctl->infeasible, hub ? 2 : 4);
        else np = px - (mn + eps);
        c.relabel++;
    }
    c.visit++;
    PN[ni(x)] = np;
    if (now > 0) mark(g, N, x, out);
    if (!hub) F.flag[x] = 0;   // every chunk has read it
    atom_exch_i(&g.q_arrive[slot], 0);
}

// Hub chunk: one workgroup, 1024 arcs (four per thread, loads issued together).
// px, E: the hub's price and excess, loaded by the caller with its flag.
template <bool CP>
__device__ void hub_chunk(const DG& g, const Front& F, const Front& N, const HItem& it, long long px, long long E,
                          const long long* __restrict__ P, long long* __restrict__ PN, long long eps, Pend& pd,
                          int& out, Cnt& c) {
    __shared__ long long sh[WPB];
    __shared__ long long s_take;
    const int x = it.node;
    long long r[PER_T], cr[PER_T], adm[PER_T], uc[PER_T];
    int w[PER_T], rv[PER_T];
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < PER_T; ++k) {
        const int a = it.begin + threadIdx.x * PER_T + k;
        r[k] = 0;
        w[k] = 0;
        rv[k] = 0;
        uc[k] = 0;
        cr[k] = 0;
        if (a < it.end) {
            const Pos q = PL<CP>::ld(g, a);
            r[k] = q.rcap;
            w[k] = q.head;
            rv[k] = q.rev;
            uc[k] = q.ucap;
            cr[k] = q.cost;   // + px − P[head], below
        }
    }
#pragma unroll
    for (int k = 0; k < PER_T; ++k) {
        const int a = it.begin + threadIdx.x * PER_T + k;
        if (a < it.end) {
            cr[k] += px - P[ni(w[k])];
            c.scan++;
        }
        adm[k] = (a < it.end && cr[k] < 0 && r[k] > 0) ? r[k] : 0;
        mine += adm[k];
    }
    long long Ac = 0;
    const long long excl = block_excl_scan(mine, sh, &Ac);
    if (threadIdx.x == 0) s_take = claim(g, it.hid, E, Ac);
    __syncthreads();
    const long long take = s_take;
    long long rt = take - excl;
    rt = rt < 0 ? 0 : (rt > mine ? mine : rt);
    long long minc = INF64;
#pragma unroll
    for (int k = 0; k < PER_T; ++k) {
        const int a = it.begin + threadIdx.x * PER_T + k;
        const long long d = adm[k] < rt ? adm[k] : rt;
        rt -= d;
        if (d > 0) {
            push_arc<CP>(g, &N, a, w[k], r[k], d, pd, out, rv[k], uc[k]);
            c.push++;
        }
        if (a < it.end) {
            if (cr[k] < 0) {
                if (r[k] - d > 0) minc = min(minc, cr[k]);
            } else if (r[k] > 0 || cr[k] <= eps) {
                minc = min(minc, cr[k]);
            }
        }
    }
    flush_pending(g, &N, pd, out);
    minc = block_min(minc, sh);
    if (threadIdx.x == 0)
        settle(g, F, N, it.hid, x, g.hnchunks[it.hid], true, take, Ac, minc, px, PN, eps, out, c);
}

// Chunked-class discharge: one wave per 64-arc chunk of node x (flagged in F).

// Whole-node discharge by one wave (chunked class, 65..4096 arcs): the wave of
// the node's lead chunk item loads its arcs NB×64 at a time (all loads of a
// batch issued together, then the price gathers), distributes the excess with
// one wave scan per 64 arcs and relabels like sweep_group. One dependent chain
// per batch instead of the claim/arrive protocol of hubs.
// e, px, b0, en: the node's excess, price and segment, loaded by the caller
// together with its frontier flag (one dependent step fewer).
// Whole-node discharge by one workgroup (chunked class): 512 arcs
// per pass (two per thread, all loads issued together), the excess distributed
// by one block-wide scan. A rack (≈ 440 arcs) is one pass — with one wave per
// node it took two dependent batches, and the chunked node was the last block
// of almost every sweep (round 3's per-launch block stamps).
template <bool CP>
__device__ void node_discharge_blk(const DG& g, const Front& F, const Front& N, int x, long long e, long long px,
                                   int b0, int en, long long* __restrict__ PN, const long long* __restrict__ P,
                                   long long eps, Pend& pd, int& out, Cnt& c) {
    __shared__ long long sh[WPB];
    if (threadIdx.x == 0) F.flag[x] = 0;   // the block consumes the node's flag
    if (e <= 0) return;                    // block-uniform
    if (threadIdx.x == 0) c.visit++;
    long long rem = e, minc = INF64;
    for (int base = b0; base < en; base += 2 * BLK) {   // block-uniform trip count
        long long r[2], cs[2], pw[2], uc[2], adm[2], cr[2];
        int w[2], rv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int a = base + j * BLK + (int)threadIdx.x;
            r[j] = 0;
            cs[j] = 0;
            w[j] = 0;
            rv[j] = 0;
            uc[j] = 0;
            if (a < en) {
                const Pos q = PL<CP>::ld(g, a);
                r[j] = q.rcap;
                w[j] = q.head;
                cs[j] = q.cost;
                rv[j] = q.rev;
                uc[j] = q.ucap;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) pw[j] = (base + j * BLK + (int)threadIdx.x < en) ? P[ni(w[j])] : 0;
        long long mine = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool valid = base + j * BLK + (int)threadIdx.x < en;
            cr[j] = cs[j] + px - pw[j];
            adm[j] = (valid && cr[j] < 0 && r[j] > 0) ? r[j] : 0;
            mine += adm[j];
        }
        long long tot = 0;
        const long long excl = block_excl_scan(mine, sh, &tot);
        long long avail = rem - excl;   // units this thread's arcs may take, in arc order
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int a = base + j * BLK + (int)threadIdx.x;
            long long d = avail < adm[j] ? avail : adm[j];
            d = d < 0 ? 0 : d;
            avail -= d;
            if (d > 0) {
                push_arc<CP>(g, &N, a, w[j], r[j], d, pd, out, rv[j], uc[j]);
                c.push++;
            }
            if (a < en) {
                c.scan++;
                if (cr[j] < 0) {
                    if (r[j] - d > 0) minc = min(minc, cr[j]);
                } else if (r[j] > 0 || cr[j] <= eps) {
                    minc = min(minc, cr[j]);
                }
            }
        }
        flush_pending(g, &N, pd, out);
        rem -= tot < rem ? tot : rem;
        if (rem == 0) break;   // no relabel needed: the rest of the arcs need no scan
    }
    minc = block_min(minc, sh);
    if (threadIdx.x == 0) {
        const long long pushed = e - rem;
        if (pushed) atom_add(&g.excess[x], -pushed);
        long long np = px;
        if (rem > 0) {
            if (minc >= INF64) g.ctl->infeasible = 1;
            else np = px - (minc + eps);
            c.relabel++;
            N.flag[x] = 1;
            out = 1;
        }
        PN[ni(x)] = np;
    }
}

// ------------------------------------------------------ grid-stride windows ---
// Sparse passes use a one-generation grid: each wave owns WPW windows (class
// windows, then chunk items) strided across the grid, ballots all their flags
// first (independent loads), then processes only the active ones.
__device__ __forceinline__ int class_of_window(const DG& g, int w) {
    int c = 0;
#pragma unroll
    for (int k = 1; k < CCLS; ++k) c += (w >= g.wbeg[k]) ? 1 : 0;
    return c;
}

// Window w's frontier flags in two steps, so a launch can issue them before it
// knows whether it has work: window_load reads this lane's flag (class windows:
// one node slot per lane; chunk items: the node's flag on lane 0), window_take
// clears what was set (class windows only; a chunk item's flag is cleared by
// the node's owner) and ballots it — nothing when go is false.
struct WinFlag {
    int slot;        // flag index this lane read (-1: none)
    int raw;         // the flag byte
    long long a;     // class windows: loaded WITH the flag — sweeps: the node's
    long long p;     //   excess and price (read buffer); Bellman-Ford: its distance and p0;
    long long seg;   //   both: its packed segment bounds (one dependent step fewer per launch)
};
// MODE 0: the flag only; 1: sweep (excess, P); 2: Bellman-Ford (dist, p0).
template <int MODE>
__device__ __forceinline__ WinFlag window_load(const DG& g, const unsigned char* flags, int w,
                                               const long long* P = nullptr) {
    w = __builtin_amdgcn_readfirstlane(w);   // wave-uniform: the class selection stays scalar
    WinFlag f{-1, 0, 0, 0, 0};
    const int ln = lane_id();
    if (w < g.wbeg[CCLS]) {
        // class c = the last with wbeg[c] <= w, selected over static fields (kernel
        // arguments: no dependent load before the flag's)
        int ob = g.obeg[0], wb = g.wbeg[0], ws = win_slots(0);
#pragma unroll
        for (int k = 1; k < CCLS; ++k)
            if (w >= g.wbeg[k]) {
                ob = g.obeg[k];
                wb = g.wbeg[k];
                ws = win_slots(k);
            }
        if (ln < ws) f.slot = ob + (w - wb) * ws + ln;
        if (MODE && f.slot >= 0) {
            f.seg = g.p0[ni(f.slot) + ND_SEG];
            if (MODE == 1) {
                f.a = atom_load(&g.excess[f.slot]);
                f.p = P[ni(f.slot)];
            } else {
                f.a = atom_load(&g.dist[ni(f.slot)]);
                f.p = g.p0[ni(f.slot)];
            }
        }
    } else if (w < g.wbeg[CCLS] + g.ncitems) {
        if (ln == 0) f.slot = g.citems[w - g.wbeg[CCLS]].node;
    }
    if (f.slot >= 0) f.raw = flags[f.slot];
    return f;
}
__device__ __forceinline__ unsigned long long window_take(const DG& g, unsigned char* flags, int w, const WinFlag& f,
                                                          bool go) {
    const bool on = go && f.raw != 0;
    if (on && w < g.wbeg[CCLS]) flags[f.slot] = 0;
    return __ballot(on);
}
// The prefetched record of node v (v − base = the lane that loaded it), to every lane.
__device__ __forceinline__ void window_node(const WinFlag& f, int v, int base, long long& a, long long& p, int& b0,
                                            int& en) {
    const int src = v >= 0 ? v - base : 0;
    a = __shfl(f.a, src);
    p = __shfl(f.p, src);
    const unsigned long long sg = (unsigned long long)__shfl(f.seg, src);
    b0 = (int)(unsigned)(sg & 0xffffffffULL);
    en = (int)(unsigned)(sg >> 32);
}

// The control words of a launch pass through an empty asm that also takes the
// launch's first loads as inputs: the words are only tested after every one of
// those loads was issued (one wait for all of them; the compiler would
// otherwise test the words first, or sink the other loads under the test).
#define KS_AFTER_LOADS(c0, c1, ...) asm volatile("" : "+v"(c0), "+v"(c1) : __VA_ARGS__)

template <int C, bool CP>
__device__ __forceinline__ void sweep_win(const DG& g, const Front& N, int w, unsigned long long mask,
                                          const WinFlag& f, const long long* __restrict__ P,
                                          long long* __restrict__ PN, long long eps, Pend& pd, int& out, Cnt& c) {
    constexpr int G = class_lanes(C);
    constexpr int PER = 64 / G;
    constexpr int WS = win_slots(C);
    const int base = g.obeg[C] + (w - g.wbeg[C]) * WS;
    const int k = lane_id() / G;
    while (mask) {
        unsigned long long mm = mask;
        for (int j = 0; j < k; ++j) mm &= mm - 1;
        const int v = mm ? base + __ffsll((long long)mm) - 1 : -1;
        long long e = 0, pv = 0;
        int b0 = 0, en = 0;
        window_node(f, v, base, e, pv, b0, en);
        if (v < 0) e = 0;
        sweep_group<G, CP>(g, N, v, e, pv, b0, en, PN, P, eps, pd, out, c);
        for (int j = 0; j < PER; ++j) mask &= mask - 1;
    }
}


template <bool CP>
__global__ __launch_bounds__(BLK) void k_sweep(DG g, int pos, int seq) {
    if (pos == 0 && blockIdx.x == 0 && threadIdx.x == 0) g.ctl->t_sw0 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0)
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) g.sf[(seq + 2) % 3].hub[h] = 0;
    // The preceding global update was applied (c_done) and the frontier is
    // non-empty (c_act): tested only after each block issued its own first loads
    // (flags, excess, node records; KS_AFTER_LOADS), so the control read is not
    // a dependent step of its own.
    int c_done, c_act;   // read in each branch, after its first loads
    auto ctl_words = [&]() {
        c_done = g.ctl->bf_done;
        c_act = pos == 0 ? g.ctl->apply_act : g.ctl->sweep_act[pos - 1];
    };
    const Front F = g.sf[seq % 3], N = g.sf[(seq + 1) % 3];
    const long long eps = g.ctl->eps;
    const long long* P = (pos & 1) ? g.p1 : g.p0;
    long long* PN = (pos & 1) ? g.p0 : g.p1;
    Pend pd{-1, 0};
    Cnt c;
    int out = 0;
    if ((int)blockIdx.x < g.nhitems) {
        const HItem it = g.hitems[blockIdx.x];
        const int fl = F.hub[it.hid];
        const long long px = P[ni(it.node)];
        const long long E = atom_load(&g.excess[it.node]);
        ctl_words();
        KS_AFTER_LOADS(c_done, c_act, "v"(fl), "v"(px), "v"(E));
        if (c_done && c_act && fl) {
            hub_chunk<CP>(g, F, N, it, px, E, P, PN, eps, pd, out, c);
        }
    } else if ((int)blockIdx.x >= g.nhitems + g.sw_clsb) {
        // chunked class: one workgroup per node (a wave per node made the chunked
        // node the last block of almost every sweep)
        const int i = (int)blockIdx.x - g.nhitems - g.sw_clsb;
        if (i < g.ncls_c) {
            const int x = g.obeg[CCLS] + i;
            // flag, excess and record (price, segment) issued together
            const int fl = F.flag[x];
            const long long e = atom_load(&g.excess[x]);
            const long long px = P[ni(x)];
            const long long sw = g.p0[ni(x) + ND_SEG];
            ctl_words();
            KS_AFTER_LOADS(c_done, c_act, "v"(fl), "v"(e), "v"(px), "v"(sw));
            const int b0 = (int)(unsigned)((unsigned long long)sw & 0xffffffffULL);
            const int en = (int)(unsigned)((unsigned long long)sw >> 32);
            // the flag and the excess may change under the block's feet (pushes into
            // x, the flag cleared by thread 0): thread 0's reading decides for all
            __shared__ long long s_e;
            __shared__ int s_go;
            if (threadIdx.x == 0) {
                s_e = e;
                s_go = c_done && c_act && fl;
            }
            __syncthreads();
            if (s_go) {
                node_discharge_blk<CP>(g, F, N, x, s_e, px, b0, en, PN, P, eps, pd, out, c);
            }
        }
    } else {
        // class windows, WPW per wave strided across the class blocks
        const int tw = g.sw_clsb * WPB;
        const int w0 = wave_index_in_grid(g.nhitems);
        WinFlag wf[WPW];
        int any_raw = 0;
#pragma unroll
        for (int j = 0; j < WPW; ++j) {
            const int w = w0 + j * tw;
            wf[j] = w < g.wbeg[CCLS] ? window_load<1>(g, F.flag, w, P) : WinFlag{-1, 0, 0, 0, 0};
            any_raw |= wf[j].raw;
        }
        ctl_words();
        KS_AFTER_LOADS(c_done, c_act, "v"(any_raw));
        const bool go = c_done && c_act;
        unsigned long long mk[WPW];
#pragma unroll
        for (int j = 0; j < WPW; ++j) mk[j] = window_take(g, F.flag, w0 + j * tw, wf[j], go);
#pragma unroll
        for (int j = 0; j < WPW; ++j) {
            if (!mk[j]) continue;
            const int w = w0 + j * tw;
            switch (class_of_window(g, w)) {
                case 0: sweep_win<0, CP>(g, N, w, mk[j], wf[j], P, PN, eps, pd, out, c); break;
                case 1: sweep_win<1, CP>(g, N, w, mk[j], wf[j], P, PN, eps, pd, out, c); break;
                case 2: sweep_win<2, CP>(g, N, w, mk[j], wf[j], P, PN, eps, pd, out, c); break;
                case 3: sweep_win<3, CP>(g, N, w, mk[j], wf[j], P, PN, eps, pd, out, c); break;
                default: sweep_win<4, CP>(g, N, w, mk[j], wf[j], P, PN, eps, pd, out, c); break;
            }
        }
    }
    if (__any(out) && lane_id() == 0) g.ctl->sweep_act[pos] = 1;
    flush_counters(g, c);
}

// ================================================ Bellman-Ford (GU and PR) ===
// Global price update (GU): distances from the deficit nodes over residual arcs
// of length clamp(floor(rc/ε)+1, 0, LEN_CAP), unreached = INF.
// Price refinement (PR): all distances start at 0, lengths floor(rc/ε)+1 may be
// negative (difference constraints of ε-optimality).
// Push-style: a node whose distance dropped relaxes its IN-arcs (u→v), i.e. the
// reverses of its CSR arcs a = (v→u): residual ucap(a) − rcap(a), cost −cost(a).
// No returning atomics: a plain pre-check filters (a stale distance is only
// larger), atomicMin commits, the flag store marks u for the next round.
//
// PR = 2: price refinement that also finds negative cycles (the
// cycle-cancelling finish). A node's dist slot then packs its distance (biased;
// d ≤ 0 from d ≡ 0) above its parent arc — the position, in the parent's
// segment, of the arc that ends at the node (the parent arc itself is its
// reverse) — so one 64-bit atomicMin keeps each distance and its parent
// consistent, and the parent graph holds the negative cycles that keep the
// refinement from converging.
constexpr int PK_NB = 24;                              // positions below 2^24
constexpr long long PK_NONE = (1LL << PK_NB) - 1;      // no parent (d = 0 from the start)
constexpr long long PK_BIAS = 1LL << 37;
__device__ __forceinline__ long long pk(long long d, long long v) {
    d = d < 1 - PK_BIAS ? 1 - PK_BIAS : (d > PK_BIAS - 1 ? PK_BIAS - 1 : d);
    return ((d + PK_BIAS) << PK_NB) | v;
}
__device__ __forceinline__ long long pk_d(long long key) { return (key >> PK_NB) - PK_BIAS; }
template <int PR>
__device__ __forceinline__ long long dkey(long long raw) { return PR == 2 ? pk_d(raw) : raw; }
// a < b as distances (packed keys: an equal distance through another parent is no improvement)
template <int PR>
__device__ __forceinline__ bool dless(long long a, long long b) { return PR == 2 ? (a >> PK_NB) < (b >> PK_NB) : a < b; }

// ε of the running phase with its reciprocal (Ctl::eps, Ctl::inv): arc lengths
// divide by ε without a division (ks_len.h).
struct EpsR {
    long long eps;
    double inv;
};
template <int PR>
__device__ __forceinline__ long long arc_len(long long pu, long long ca, long long pv, const EpsR& er) {
    long long len = ks_floordiv_inv(pu - ca - pv, er.eps, er.inv) + 1;
    if (!PR) len = len < 0 ? 0 : (len > LEN_CAP ? LEN_CAP : len);
    return len;
}

// Offer distance cand to node u. Returns true when u is a grouped node whose
// distance this call lowered (the caller then owns propagating it).
template <int PR>
__device__ __forceinline__ bool offer(const DG& g, const Front& nf, int u, long long cand, long long du,
                                      long long B, long long* hub_min, int& out) {
    if (cand >= B) return false;   // at or beyond every listed excess node's distance (bounded update)
    if (u >= g.hub_base) {
        const int h = u - g.hub_base;
        if (h < HUB_LDS) {
            __hip_atomic_fetch_min(&hub_min[h], cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (dless<PR>(cand, atom_min_ret(&g.dist[ni(u)], cand))) {
            nf.hub[h] = 1;
            out = 1;
        }
        return false;
    }
    if (!dless<PR>(cand, du)) return false;
    atom_min(&g.dist[ni(u)], cand);
    return true;
}

// Continuation queue (ks_opts.two_hop 2): a lane that lowered a node
// of a lane-group class (16, 32 or 64 lanes: not a leaf, not chunked, not a hub)
// hands it to its own workgroup, which relaxes it behind the main pass of the
// same launch (bf_drain) instead of flagging it for the next one. An entry
// holds what that pass needs without a dependent load; all of it sits in
// registers where the node is lowered (the segment shares the record's line
// with the price). Entries live in LDS and never outlive the launch.
constexpr int TWO_HOP_DEFAULT = 2;   // ks_opts.two_hop 0 (1: two hops, 2: the continuation — measured faster on configs 2, 3 and 4)
constexpr int BF_DEPTH = 1;    // queue levels: 1 = four hops per launch, 2 = six (a drained node's lowerings queue once more; measured, no gain)
constexpr int BFQ_GROUP = 32;  // lanes that relax one queued node (a 64-lane class node in two steps)
// entries per level (32 B each): what the workgroup's groups relax in ONE step. A
// longer queue is drained step after step by the one workgroup that filled it while
// the rest of the grid has retired (config 3, 256 entries: a working launch 16 → 31 µs,
// the solve 3.6 ms slower); what does not fit takes the flags, which spread it over
// the next launch's whole grid.
constexpr int BFQ_CAP = BLK / BFQ_GROUP;
struct QEnt {
    long long pu, d;    // the node's price; the distance it was lowered to (decoded in every mode)
    int b0, b1, u, pad;
};
struct BfQ {
    QEnt* q;     // LDS
    int* n;      // LDS: entries claimed (may run past cap: the drain takes min(n, cap))
    int cap;     // 0: no queue (lowered nodes are flagged)
    int lo, hi;  // queued node ids: [obeg[2], obeg[CCLS])
};
// true: u is queued (the workgroup owns propagating it); false: the caller flags it
__device__ __forceinline__ bool bf_enqueue(const BfQ& Q, int u, unsigned long long seg, long long d, long long pu) {
    if (u < Q.lo || u >= Q.hi) return false;   // (cap 0: lo = hi = 0)
    const unsigned i = (unsigned)atomicAdd(Q.n, 1);
    if (i >= (unsigned)Q.cap) return false;    // full: today's flag path
    QEnt e;
    e.pu = pu;
    e.d = d;
    e.b0 = (int)(unsigned)(seg & 0xffffffffULL);
    e.b1 = (int)(unsigned)(seg >> 32);
    e.u = u;
    e.pad = 0;
    Q.q[i] = e;
    return true;
}

// A leaf's arc records loaded together and held in registers: a task has five
// arcs and a PU two, so five cover the scheduling graphs; a leaf of six to eight
// arcs reads the rest one by one. Eight held 24 more VGPRs across the expansion
// and kept k_bf_round at 4 waves per SIMD. -DKS_LEAF_REGS: tuning builds.
#ifndef KS_LEAF_REGS
#define KS_LEAF_REGS 5
#endif
constexpr int LEAF_REGS = KS_LEAF_REGS;

// Relax the in-arcs of a low-degree node u (≤ 8 arcs: tasks, PUs) right after
// its distance dropped to du: a second hop inside the same round.
template <int PR, bool CP>
__device__ __forceinline__ void expand_leaf(const DG& g, const Front& nf, const BfQ& Q, int u, long long du, long long pu,
                                            int b0, int b1, const EpsR& er, long long B, long long* hub_min, int& out,
                                            int& lscan) {
    lscan += b1 - b0;   // the second hop's in-arc positions examined (ks_result.gu_leaf_scans)
    // the records of the first LEAF_REGS arcs issued together; usually one in-arc
    // carries flow (a task's assignment), so the dependent loads follow for it alone
    unsigned live = 0;
    int hd[LEAF_REGS];
    long long cb[LEAF_REGS];
#pragma unroll
    for (int k = 0; k < LEAF_REGS; ++k) {
        hd[k] = 0;
        cb[k] = 0;
        if (b0 + k < b1) {
            const Pos q = PL<CP>::ld_nr(g, b0 + k);
            hd[k] = q.head;
            cb[k] = q.cost;
            if (q.ucap - q.rcap > 0) live |= 1u << k;
        }
    }
    for (int b = b1 - b0 > LEAF_REGS ? b0 + LEAF_REGS : b1; b < b1; ++b) {   // the arcs beyond the registers, one by one
        const Pos q = PL<CP>::ld_nr(g, b);
        if (q.ucap - q.rcap > 0) {
            const int u2 = q.head;
            const long long pu2 = g.p0[ni(u2)];
            long long cand = du + arc_len<PR>(pu2, q.cost, pu, er);
            if (PR == 2) cand = pk(cand, b);
            if (offer<PR>(g, nf, u2, cand, u2 < g.hub_base ? g.dist[ni(u2)] : INF64, B, hub_min, out) &&
                !bf_enqueue(Q, u2, Q.cap ? (unsigned long long)g.p0[ni(u2) + ND_SEG] : 0ULL, dkey<PR>(cand), pu2)) {
                nf.flag[u2] = 1;
                out = 1;
            }
        }
    }
    while (live) {
        const int k = __builtin_ctz(live);
        live &= live - 1;
        int u2 = 0;
        long long c2 = 0;
#pragma unroll
        for (int j = 0; j < LEAF_REGS; ++j)   // register select (no dynamic indexing into scratch)
            if (j == k) {
                u2 = hd[j];
                c2 = cb[j];
            }
        const long long pu2 = g.p0[ni(u2)];
        const long long du2 = u2 < g.hub_base ? g.dist[ni(u2)] : INF64;
        // (continuation: the segment comes with the record, for the queue entry)
        const unsigned long long sg2 = Q.cap ? (unsigned long long)g.p0[ni(u2) + ND_SEG] : 0ULL;
        long long cand = du + arc_len<PR>(pu2, c2, pu, er);
        if (PR == 2) cand = pk(cand, b0 + k);
        if (offer<PR>(g, nf, u2, cand, du2, B, hub_min, out) && !bf_enqueue(Q, u2, sg2, dkey<PR>(cand), pu2)) {
            nf.flag[u2] = 1;
            out = 1;
        }
    }
}

// Relax in-arc (u→v) = reverse of CSR arc a = (v→u); residual ucap − rcap,
// cost −cost(a). Loads are issued before the residual test (short chain).
// (relax_pos: the position record q of arc a already loaded)
template <int PR, bool CP>
__device__ __forceinline__ void relax_pos(const DG& g, const Front& nf, const BfQ& Q, const Pos& q, int a, long long dv,
                                          long long pv, const EpsR& er, long long B, long long* hub_min, int& out,
                                          int& lscan) {
    const long long rin = q.ucap - q.rcap;
    // an arc that cannot relax reads node 0's (hot) record instead of its head's
    // random line: the loads stay unconditional (no branch join to wait at) and
    // the line is not fetched (config 3: −1…2 ms per solve, interleaved A/B)
    const int u = rin > 0 ? q.head : 0;
    const long long ca = q.cost;
    const long long pu = g.p0[ni(u)];
    const long long du = u < g.hub_base ? g.dist[ni(u)] : INF64;
    const bool leaf = g.expand && u < g.obeg[2];
    // a leaf's segment for its expansion, a queued class's for its queue entry
    unsigned long long sg = 0;
    if (leaf || (u >= Q.lo && u < Q.hi)) sg = (unsigned long long)g.p0[ni(u) + ND_SEG];   // same record line as pu, du
    if (rin <= 0) return;
    const long long cand = dv + arc_len<PR>(pu, ca, pv, er);   // (dv decoded: a distance in every mode)
    const long long key = PR == 2 ? pk(cand, a) : cand;
    if (!offer<PR>(g, nf, u, key, du, B, hub_min, out)) return;
    if (leaf) {
        const int b0 = (int)(unsigned)(sg & 0xffffffffULL), b1 = (int)(unsigned)(sg >> 32);
        expand_leaf<PR, CP>(g, nf, Q, u, cand, pu, b0, b1, er, B, hub_min, out, lscan);   // tasks, PUs: two hops per round
    } else if (!bf_enqueue(Q, u, sg, dkey<PR>(key), pu)) {
        nf.flag[u] = 1;
        out = 1;
    }
}

template <int PR, bool CP>
__device__ __forceinline__ void relax_in(const DG& g, const Front& nf, const BfQ& Q, int v, int a, long long dv, long long pv,
                                         const EpsR& er, long long B, long long* hub_min, int& out, int& lscan) {
    relax_pos<PR, CP>(g, nf, Q, PL<CP>::ld_nr(g, a), a, dv, pv, er, B, hub_min, out, lscan);
}

// The continuation's second pass: the workgroup's 32-lane groups take the queued
// nodes in turn (a 64-lane class node in two steps) and relax their in-arcs from
// the queued distance. The node's current distance is loaded with the positions:
// an entry whose node was lowered further since is skipped — that lowerer owns
// the propagation, through its own entry or its flag. Nodes lowered here go to
// Qn (the next level; cap 0: the frontier flags of the next launch).
template <int PR, bool CP>
__device__ __forceinline__ void bf_drain(const DG& g, const Front& nf, const QEnt* q, int n, const BfQ& Qn, const EpsR& er,
                                         long long B, long long* hub_min, int& out, int& scans, int& lscan) {
    constexpr int QG = BFQ_GROUP;
    const int lig = threadIdx.x & (QG - 1);
    for (int i = threadIdx.x / QG; i < n; i += BLK / QG) {
        const QEnt e = q[i];
        const long long cur = atom_load(&g.dist[ni(e.u)]);
        for (int a = e.b0 + lig; a < e.b1; a += QG) {
            Pos p = PL<CP>::ld_nr(g, a);
            if (dkey<PR>(cur) != e.d) p.rcap = p.ucap;   // stale entry: no residual (a select, the loads stay issued together)
            relax_pos<PR, CP>(g, nf, Qn, p, a, e.d, e.pu, er, B, hub_min, out, lscan);
            scans++;
        }
    }
}

template <int G, int PR, bool CP>
__device__ __forceinline__ void bf_group_pre(const DG& g, const Front& nf, const BfQ& Q, int v, long long dv, long long pv, int b0,
                                             int en, const EpsR& er, long long B, long long* hub_min, int& out, int& scans, int& lscan) {
    const int lig = lane_id() & (G - 1);
    const bool act = v >= 0 && (PR || dv < INF64);
    if (!act) en = b0;
    const int iters = G < 64 ? 1 : (en - b0 + 63) / 64;
    for (int it = 0; it < iters; ++it) {
        const int a = b0 + it * G + lig;
        if (a < en) {
            relax_in<PR, CP>(g, nf, Q, v, a, dkey<PR>(dv), pv, er, B, hub_min, out, lscan);
            scans++;
        }
    }
}

// Sparse Bellman-Ford pass over window w of class C (mask from window_mask).
template <int C, int PR, bool CP>
__device__ __forceinline__ void bf_win(const DG& g, const Front& N, const BfQ& Q, int w, unsigned long long mask, const WinFlag& f,
                                       const EpsR& er, long long B, long long* hub_min, int& out, int& scans, int& lscan) {
    constexpr int G = class_lanes(C);
    constexpr int PER = 64 / G;
    constexpr int WS = win_slots(C);
    const int base = g.obeg[C] + (w - g.wbeg[C]) * WS;
    const int k = lane_id() / G;
    while (mask) {
        unsigned long long mm = mask;
        for (int j = 0; j < k; ++j) mm &= mm - 1;
        const int v = mm ? base + __ffsll((long long)mm) - 1 : -1;
        long long d = INF64, pv = 0;
        int b0 = 0, en = 0;
        window_node(f, v, base, d, pv, b0, en);
        if (v < 0) d = INF64;
        bf_group_pre<G, PR, CP>(g, N, Q, v, d, pv, b0, en, er, B, hub_min, out, scans, lscan);
        for (int j = 0; j < PER; ++j) mask &= mask - 1;
    }
}

// One 64-arc chunk of a chunked-class node (its flag already tested).
template <int PR, bool CP>
__device__ __forceinline__ void bf_chunk(const DG& g, const Front& N, const BfQ& Q, const CItem& ci, const EpsR& er,
                                         long long B, long long* hub_min, int& out, int& scans, int& lscan) {
    const long long dv = atom_load(&g.dist[ni(ci.node)]);
    if (!PR && dv >= INF64) return;
    const int a = ci.begin + lane_id();
    if (a < ci.end) {
        relax_in<PR, CP>(g, N, Q, ci.node, a, dkey<PR>(dv), g.p0[ni(ci.node)], er, B, hub_min, out, lscan);
        scans++;
    }
}

template <int G, int PR, bool CP>
__device__ __forceinline__ void bf_group(const DG& g, const Front& nf, const BfQ& Q, int v, const EpsR& er, long long B, long long* hub_min,
                                         int& out, int& scans, int& lscan) {
    const int lig = lane_id() & (G - 1);
    long long dv = INF64;
    if (v >= 0) dv = atom_load(&g.dist[ni(v)]);
    const bool act = v >= 0 && (PR || dv < INF64);
    long long pv = 0;
    int b0 = 0, en = 0;
    if (act) {
        pv = g.p0[ni(v)];
        seg_of(g.p0, v, b0, en);
    }
    const int iters = G < 64 ? 1 : (en - b0 + 63) / 64;
    for (int it = 0; it < iters; ++it) {
        const int a = b0 + it * G + lig;
        if (a < en) {
            relax_in<PR, CP>(g, nf, Q, v, a, dkey<PR>(dv), pv, er, B, hub_min, out, lscan);
            scans++;
        }
    }
}

// One Bellman-Ford round. dense = 1: every node (first round of an update).
// dense_arg < 0: the round is dense iff it is the running update's first
// (bf_seq0, set by the init kernel); ≥ 0: as given.
template <int PR, bool CP>
__global__ __launch_bounds__(BLK) void k_bf_round(DG g, int seq, int dense_arg) {
    const unsigned long long t_entry = PR == 2 ? __builtin_amdgcn_s_memrealtime() : 0;
    const int dense = __builtin_amdgcn_readfirstlane(dense_arg >= 0 ? dense_arg : (seq == g.ctl->bf_seq0 ? 1 : 0));
    __shared__ long long hub_min[HUB_LDS];
    __shared__ QEnt bfq[BF_DEPTH][BFQ_CAP];   // the continuation queue (g.expand ≥ 2), one level per extra hop pair
    __shared__ int bfq_n[BF_DEPTH];
    if (blockIdx.x == 0) {
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) g.bf[(seq + 2) % 3].hub[h] = 0;
        if (threadIdx.x == 0) g.ctl->bfa[(seq + 2) % 3] = 0;
    }
    const Front F = g.bf[seq % 3], N = g.bf[(seq + 1) % 3];
    if (threadIdx.x < HUB_LDS) hub_min[threadIdx.x] = INF64;
    if (threadIdx.x < BF_DEPTH) bfq_n[threadIdx.x] = 0;
    // g.expand 2: BFQ_CAP entries; 3 (TESTS ONLY, fault_inject bit 9): 2, so almost every enqueue overflows
    const int qcap = g.expand < 2 ? 0 : (g.expand == 2 ? BFQ_CAP : 2);
    const int qlo = qcap ? g.obeg[2] : 0, qhi = qcap ? g.obeg[CCLS] : 0;
    const BfQ Q{bfq[0], &bfq_n[0], qcap, qlo, qhi};
    __syncthreads();   // (waits for outstanding loads: the control words are read after it)
    // The update is still running (!done) and this round's frontier is non-empty
    // (dense || any): read in each branch after its first loads and tested only
    // once they were issued (KS_AFTER_LOADS).
    int done = 0, any = 0;
    auto ctl_words = [&]() {
        done = g.ctl->bf_done;
        any = g.ctl->bfa[seq % 3];
    };
    auto ctl_uniform = [&]() {   // the words are wave-uniform: scalar registers for the rest of the launch
        done = __builtin_amdgcn_readfirstlane(done);
        any = __builtin_amdgcn_readfirstlane(any);
    };
    const EpsR er{uniform64(g.ctl->eps), __longlong_as_double(uniform64(__double_as_longlong(g.ctl->inv)))};
    // bounded update (tail): offers at or above the listed excess nodes' largest
    // tentative distance are dropped (that bound only falls, so a stale copy is safe)
    const long long B = (!PR && g.bound) ? uniform64(atom_load(&g.ctl->bf_bound)) : INF64;
    int out = 0;
    int scans = 0, lscan = 0;   // per lane and launch: 32 bits, widened at the wave sum
    // Hub chunks are split over HSPLIT workgroups: a relaxation is a dependent
    // chain (arc, tail record, leaf expansion, atomic), and a thread that runs
    // several of them in a row made the hub the last block of its round.
    const int nhb = g.nhitems * HSPLIT;
    if ((int)blockIdx.x < nhb) {
        const HItem it = g.hitems[blockIdx.x / HSPLIT];
        const int sub = (int)blockIdx.x % HSPLIT;
        const int fl = F.hub[it.hid];
        const long long dv = atom_load(&g.dist[ni(it.node)]);
        const long long pv = g.p0[ni(it.node)];
        ctl_words();
        KS_AFTER_LOADS(done, any, "v"(fl), "v"(dv), "v"(pv));
        ctl_uniform();
        if (!done && (dense || any) && (dense || fl)) {
            if (PR || dv < INF64) {
#pragma unroll
                for (int k = 0; k < BF_PER_T; ++k) {
                    const int a = it.begin + sub * (CHUNK / HSPLIT) + threadIdx.x * BF_PER_T + k;
                    if (a < it.end) {
                        relax_in<PR, CP>(g, N, Q, it.node, a, dkey<PR>(dv), pv, er, B, hub_min, out, lscan);
                        scans++;
                    }
                }
            }
        }
    } else if (dense) {
        const int w = wave_index_in_grid(nhb);
        ctl_words();
        ctl_uniform();
        if (done) {
            // the update already converged
        } else if (w < g.wbeg[CCLS]) {
            const Scan sc{F.flag, 1};
#define KS_BF_CALL(C) bf_group<G_, PR, CP>(g, N, Q, v, er, B, hub_min, out, scans, lscan)
            KS_BY_CLASS(w, sc, KS_BF_CALL)
#undef KS_BF_CALL
        } else if (w - g.wbeg[CCLS] < g.ncitems) {
            bf_chunk<PR, CP>(g, N, Q, g.citems[w - g.wbeg[CCLS]], er, B, hub_min, out, scans, lscan);
        }
    } else {
        const int tw = ((int)gridDim.x - nhb) * WPB;
        const int w0 = wave_index_in_grid(nhb);
        WinFlag wf[WPW];
        int any_raw = 0;
#pragma unroll
        for (int j = 0; j < WPW; ++j) {
            wf[j] = window_load<2>(g, F.flag, w0 + j * tw);
            any_raw |= wf[j].raw;
        }
        ctl_words();
        KS_AFTER_LOADS(done, any, "v"(any_raw));
        ctl_uniform();
        const bool go = !done && any;
        unsigned long long mk[WPW];
#pragma unroll
        for (int j = 0; j < WPW; ++j) {
            const int w = w0 + j * tw;
            mk[j] = window_take(g, F.flag, w, wf[j], go);
            // chunk items: a node's flag is read by all its chunks; the lead chunk
            // clears it two rounds later (in the buffer read by the previous round)
            if (go && w >= g.wbeg[CCLS] && w - g.wbeg[CCLS] < g.ncitems && lane_id() == 0) {
                const CItem ci = g.citems[w - g.wbeg[CCLS]];
                if (ci.lead) g.bf[(seq + 2) % 3].flag[ci.node] = 0;
            }
        }
#pragma unroll
        for (int j = 0; j < WPW; ++j) {
            if (!mk[j]) continue;
            const int w = w0 + j * tw;
            if (w >= g.wbeg[CCLS]) {
                bf_chunk<PR, CP>(g, N, Q, g.citems[w - g.wbeg[CCLS]], er, B, hub_min, out, scans, lscan);
                continue;
            }
            switch (class_of_window(g, w)) {
                case 0: bf_win<0, PR, CP>(g, N, Q, w, mk[j], wf[j], er, B, hub_min, out, scans, lscan); break;
                case 1: bf_win<1, PR, CP>(g, N, Q, w, mk[j], wf[j], er, B, hub_min, out, scans, lscan); break;
                case 2: bf_win<2, PR, CP>(g, N, Q, w, mk[j], wf[j], er, B, hub_min, out, scans, lscan); break;
                case 3: bf_win<3, PR, CP>(g, N, Q, w, mk[j], wf[j], er, B, hub_min, out, scans, lscan); break;
                default: bf_win<4, PR, CP>(g, N, Q, w, mk[j], wf[j], er, B, hub_min, out, scans, lscan); break;
            }
        }
    }
    __syncthreads();
    // the continuation: nodes this workgroup lowered are relaxed before it retires
    // (an empty queue costs this one LDS read; the count is uniform over the block)
    if (bfq_n[0]) {
#pragma unroll
        for (int l = 0; l < BF_DEPTH; ++l) {
            const int qn = min(bfq_n[l], qcap);
            const BfQ Qn{bfq[l + 1 < BF_DEPTH ? l + 1 : 0], &bfq_n[l + 1 < BF_DEPTH ? l + 1 : 0],
                         l + 1 < BF_DEPTH ? qcap : 0, l + 1 < BF_DEPTH ? qlo : 0, l + 1 < BF_DEPTH ? qhi : 0};
            bf_drain<PR, CP>(g, N, bfq[l], qn, Qn, er, B, hub_min, out, scans, lscan);
            __syncthreads();   // the next level's entries and the hub minima
        }
    }
    if (threadIdx.x < HUB_LDS && (int)threadIdx.x < g.nheavy) {
        const long long val = hub_min[threadIdx.x];
        if (val < INF64) {
            long long* dx = &g.dist[ni(g.hub_base + threadIdx.x)];
            if (dless<PR>(val, atom_load(dx)) && dless<PR>(val, atom_min_ret(dx, val))) {
                N.hub[threadIdx.x] = 1;
                out = 1;
            }
        }
    }
    if (__any(out) && lane_id() == 0) g.ctl->bfa[(seq + 1) % 3] = 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // block 0 is a hub block or a window block: done/any are final here
        if (PR == 2 && g.ctl->t_srch) {   // the finish: the search before this round ended when it started
            g.ctl->srch_ticks += t_entry - g.ctl->t_srch;
            g.ctl->t_srch = 0;
        }
        if (!done && (dense || any)) {
            atomicAdd(g.ctr + C_BFROUND, 1ULL);
            g.ctl->bf_count += 1;
        } else if (!done) {
            g.ctl->bf_done = 1;   // empty frontier: the update converged
        }
    }
    // the next rounds' bound: the largest tentative distance of the listed excess
    // nodes once all of them are reached (every value taken is ≥ the final one)
    if (!PR && g.bound && blockIdx.x == 0 && threadIdx.x < WAVE && !done && (dense || any)) {
        const int nb = g.ctl->n_bx;
        if (nb > 0 && nb <= BX_CAP) {
            long long d = 0;
            if ((int)threadIdx.x < nb) d = atom_load(&g.dist[ni(g.bx[threadIdx.x])]);
            d = wave_max(d);
            if (threadIdx.x == 0 && d < INF64)
                __hip_atomic_fetch_min(&g.ctl->bf_bound, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    scans = wave_sum(scans);
    lscan = wave_sum(lscan);
    if (lane_id() == 0 && (scans | lscan)) {
        const int sh = ((blockIdx.x * WPB) + (threadIdx.x >> 6)) & (CTR_SHARDS - 1);
        if (scans) atomicAdd(g.ctr + sh * NCTR + C_GUSCAN, (unsigned long long)scans);
        if (lscan) atomicAdd(g.ctr + sh * NCTR + C_GULEAF, (unsigned long long)lscan);
    }
}

__device__ __forceinline__ void clear_fronts(const DG& g, const Front* fs) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < g.hub_base; i += (long long)gridDim.x * BLK) {
        fs[0].flag[i] = 0;
        fs[1].flag[i] = 0;
        fs[2].flag[i] = 0;
    }
    if (blockIdx.x == 0)
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) fs[0].hub[h] = fs[1].hub[h] = fs[2].hub[h] = 0;
}

// Wave-aggregated append of the lanes with on set to the bound's excess list.
__device__ __forceinline__ void bx_append(const DG& g, bool on, int v) {
    const unsigned long long m = __ballot(on);
    if (!m) return;
    int base = 0;
    if (lane_id() == 0) base = atomicAdd(&g.ctl->n_bx, (int)__popcll(m));
    base = __shfl(base, 0);
    if (on) {
        const int idx = base + (int)__popcll(m & ((1ULL << lane_id()) - 1));
        if (idx < BX_CAP) g.bx[idx] = v;
    }
}

// GU init: drain hub inboxes, dist = 0 at deficits / INF elsewhere, clean flags.
// A cycle whose predecessor left its update unconverged (gu_pending) continues
// that update instead; seq0 = the sequence number of this cycle's first round.
// The deficits are the first round's frontier (a sparse round: the dense pass
// over every node cost 16–60 µs per update). Each flag is set by the thread that
// cleared it (same grid-stride mapping as clear_fronts; hubs: block 0).
__global__ void k_gu_init(DG g, int seq0, int list) {
    if (g.ctl->gu_pending) return;
    clear_fronts(g, g.bf);
    const Front F0 = g.bf[seq0 % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(&g.ctl->bf_bound, INF64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g.ctl->gu_B = INF64;
        g.ctl->bf_done = 0;
        g.ctl->gu_L = 0;
        g.ctl->gu_X = -1;
        g.ctl->bf_r0 = g.ctl->bf_count;
        g.ctl->bf_seq0 = seq0;
        g.ctl->n_exc = 0;
        g.ctl->u_exc = 0;
        g.ctl->aug_reached = 0;
        g.ctl->aug_short = 0;
        for (int k = 0; k < 3; ++k) g.ctl->bfa[k] = k == seq0 % 3 ? 1 : 0;
    }
    // list: the host expects few excess nodes (the last apply found ≤ BX_CAP) —
    // list them (n_bx, reset by k_gu_max) so the rounds can bound the update
    for (long long v0 = blockIdx.x * (long long)BLK; v0 < g.hub_base; v0 += (long long)gridDim.x * BLK) {
        const long long v = v0 + threadIdx.x;
        long long e = 0;
        if (v < g.hub_base) {
            e = atom_load(&g.excess[v]);
            g.dist[ni(v)] = e < 0 ? 0 : INF64;
            if (e < 0) F0.flag[v] = 1;
        }
        if (list) bx_append(g, e > 0, (int)v);
    }
    if (blockIdx.x == 0)
        for (int h0 = 0; h0 < g.nheavy; h0 += BLK) {
            const int h = h0 + threadIdx.x;
            long long e = 0;
            if (h < g.nheavy) {
                drain_inbox(g, h);
                e = atom_load(&g.excess[g.hub_base + h]);
                g.dist[ni(g.hub_base + h)] = e < 0 ? 0 : INF64;
                if (e < 0) F0.hub[h] = 1;
            }
            if (list) bx_append(g, e > 0, g.hub_base + h);
        }
}

// PR init: dist = 0 everywhere, or dist = p (canonical prices: see k_pr_apply);
// from_p = 2: d = 0 with no parent, packed (the cycle-cancelling refinement).
__global__ void k_pr_init(DG g, int seq0, int from_p) {
    clear_fronts(g, g.bf);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g.ctl->bf_done = 0;
        g.ctl->bf_seq0 = seq0;
        for (int k = 0; k < 3; ++k) g.ctl->bfa[k] = 0;
    }
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK)
        g.dist[ni(v)] = from_p == 2 ? ((PK_BIAS << PK_NB) | PK_NONE) : from_p ? g.p0[ni(v)] : 0;
}

// End of a cycle: an update that has not converged is continued by the next
// cycle; the control block goes straight to pinned host memory (a copy engine
// transfer would drain the queue around it: ~65 µs of idle GPU per cycle).
__global__ void k_cycle_end(DG g, Ctl* host, int fwd) {
    static_assert(sizeof(Ctl) % 4 == 0, "Ctl is copied as words");
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        if (!fwd) g.ctl->gu_pending = g.ctl->bf_done ? 0 : 1;   // (forward: k_fs_end)
        g.ctl->t_end = t;
    }
    __syncthreads();
    const int* src = reinterpret_cast<const int*>(g.ctl);
    int* dst = reinterpret_cast<int*>(host);
    for (int i = threadIdx.x; i < (int)(sizeof(Ctl) / 4); i += blockDim.x)
        __hip_atomic_store(&dst[i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    // a forward init counts excess nodes into n_exc from every block: zero it here
    // (a backward init zeroes it itself; forward updates: k_fs_end)
    if (threadIdx.x == 0) {
        if (!fwd) {
            g.ctl->n_exc = 0;
            g.ctl->u_exc = 0;
        }
        g.ctl->fs_moved_cyc = 0;
    }
    __threadfence_system();
}

// max finite distance (only once the update converged); cleans the sweep
// frontiers and flags the apply step and the sweeps write.
constexpr int SET_FWD = 1;   // k_set_eps: no forward search pending, its counters zeroed
constexpr int SET_CYC = 2;   //            the finish's cycle counters zeroed
__global__ void k_set_eps(DG g, long long eps, double inv, int flags) {
    g.ctl->eps = eps;
    g.ctl->inv = inv;                  // 1 / ε, the host's bits (ks_len.h)
    g.ctl->lim = (1LL << 60) / eps;    // the largest distance ε multiplies without overflowing a price
    if (flags & SET_FWD) {
        g.ctl->fs_pending = 0;
        g.ctl->fs_cnt[0] = g.ctl->fs_cnt[1] = g.ctl->fs_cnt[2] = 0;
        g.ctl->fs_completed = 0;
    }
    if (flags & SET_CYC) {
        g.ctl->cyc_done = 0;
        g.ctl->cyc_rej = 0;
    }
}

// The finish's batch end: closes the running search's time and copies the control
// block into pinned host memory (no copy-engine transfer: that drains the queue).
__global__ void k_prc_snap(DG g, Ctl* host) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && g.ctl->t_srch) {
        g.ctl->srch_ticks += t - g.ctl->t_srch;
        g.ctl->t_srch = 0;
    }
    __syncthreads();
    const int* src = reinterpret_cast<const int*>(g.ctl);
    int* dst = reinterpret_cast<int*>(host);
    for (int i = threadIdx.x; i < (int)(sizeof(Ctl) / 4); i += blockDim.x)
        __hip_atomic_store(&dst[i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
}

__global__ void k_gu_max(DG g) {
    __shared__ long long sh[WPB];
    clear_fronts(g, g.sf);
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < MAXB; k += BLK) g.ctl->sweep_act[k] = 0;
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) {
            g.aug_req[h] = 0;
        }
        if (threadIdx.x == 0) {
            g.ctl->apply_act = 0;
            g.ctl->n_xl2 = 0;
        }
    }
    if (!g.ctl->bf_done) return;
    if (g.bound && blockIdx.x == 0 && threadIdx.x < WAVE) {
        // a bounded update caps the prices at the listed excess nodes' largest
        // distance (exact there; every node at or beyond it gets the cap)
        const int nb = g.ctl->n_bx;
        if (nb > 0 && nb <= BX_CAP) {
            long long d = 0;
            if ((int)threadIdx.x < nb) d = atom_load(&g.dist[ni(g.bx[threadIdx.x])]);
            d = wave_max(d);
            if (threadIdx.x == 0) g.ctl->gu_B = d;
        }
        if (threadIdx.x == 0) g.ctl->n_bx = 0;   // the next update lists afresh
    }
    long long mx = 0;
    long long mxx = -1;   // the farthest node holding excess
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK) {
        const long long d = atom_load(&g.dist[ni(v)]);
        if (d < INF64) mx = max(mx, d);
        if (d < INF64 && atom_load(&g.excess[v]) > 0) mxx = max(mxx, d);
    }
    mx = wave_max(mx);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) sh[w] = mx;
    mxx = wave_max(mxx);
    __shared__ long long shx[WPB];
    if (lane_id() == 0) shx[w] = mxx;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < WPB; ++i) t = max(t, sh[i]);
        if (t) __hip_atomic_fetch_max(&g.ctl->gu_L, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long tx = -1;
        for (int i = 0; i < WPB; ++i) tx = max(tx, shx[i]);
        if (tx >= 0) __hip_atomic_fetch_max(&g.ctl->gu_X, tx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// apply p ← p − ε·min(d, L) and seed the sweep frontier with every excess node
// (L: the largest finite distance, capped at the farthest excess node's).
__global__ void k_gu_apply(DG g, int sseq) {
    if (!g.ctl->bf_done) return;
    const long long eps = g.ctl->eps;
    const long long lim = g.ctl->lim;
    long long L = g.ctl->gu_L;
    L = L < g.ctl->gu_B ? L : g.ctl->gu_B;   // bounded update: the cap
    {   // and at the farthest excess node's distance: min(d, X) keeps the triangle inequality
        // (monotone, 1-Lipschitz), every excess node still gets its full step, and the
        // nodes beyond X — far from the deficits or cut off — stop drifting by ε·L per
        // update (config 4: 34–37 → 29–31 ms per round, config 3 unchanged)
        const long long X = g.ctl->gu_X;
        if (X >= 0) L = L < X ? L : X;
    }
    L = L < lim ? L : lim;
    const Front F = g.sf[sseq % 3];
    int out = 0, xv = -1;
    long long units = 0;
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK) {
        const long long d = atom_load(&g.dist[ni(v)]);
        const long long e = atom_load(&g.excess[v]);
        units += e > 0 ? e : 0;
        if (d >= INF64 && e > 0) atomicOr(&g.ctl->infeasible, 8);
        const long long dd = d < L ? d : L;
        const long long np = g.p0[ni(v)] - eps * dd;
        g.p0[ni(v)] = np;
        g.p1[ni(v)] = np;
        if (e > 0) {
            mark(g, F, (int)v, out);
            xv = (int)v;
        }
    }
    // count the excess nodes (one atomic per wave) and list the first aug_k for the walkers
    const unsigned long long ex = __ballot(out);
    int base = 0;
    if (ex && lane_id() == 0) {
        g.ctl->apply_act = 1;
        base = atomicAdd(&g.ctl->n_exc, (int)__popcll(ex));
    }
    base = __shfl(base, 0);
    units = wave_sum(units);
    if (units && lane_id() == 0) atom_add(&g.ctl->u_exc, units);
    if (out) {
        const int idx = base + (int)__popcll(ex & ((1ULL << lane_id()) - 1));
        if (idx < g.aug_k) g.xl[idx] = xv;
        if (idx < 4) {
            g.ctl->dbg_x[idx] = xv;
            g.ctl->dbg_e[idx] = (int)atom_load(&g.excess[xv]);
        }
    }
}

// ------------------------------------------------------- tail augmentation ---
// When a converged update leaves at most aug_k nodes with excess (the tail of a
// phase: a few units that the sweeps would move one hop per sweep over dozens
// of update cycles), each of them sends its excess straight down the update's
// distances: one wave per excess node walks from u along the residual arc
// (u, w) of least distance d(w), until it reaches a deficit. An arc qualifies
// if d(w) < d(u) (or d(w) = d(u) and it is admissible) and its reduced cost
// under the updated prices is at most slack·ε: the reverse arc a push creates
// then has reduced cost ≥ −slack·ε (slack 1 in a phase that must end
// 1-optimal). Walkers claim residual capacity with a CAS (they may share arcs);
// units that cannot go on (no arc, capacity taken, the hop limit) stay where the
// walk stands, marked for the sweeps that follow; a unit that reaches a hub is
// left there for the hub distribution (k_aug_hub), which hands it on along the
// hub's qualifying arcs in parallel, and a second walker pass starts from the
// nodes it fed. Runs between the apply and the cycle's sweeps.
//
// Measured alternative, not kept: a blocking flow (DFS walkers with
// dead-end marks). On the device's own tail state (a -DKS_DUMP snapshot read by
// tools/proto/tail_dump.c) even a sequential blocking flow needs 21–24 updates
// for config 3's last 68 units — the last ones leave two nodes one unit per
// update through the cluster aggregator — so it saved no cycles and its searches
// cost more than these walks.
constexpr int AUG_K2 = 256;        // walkers from the nodes a hub distribution fed
constexpr int AUG_STEPS = 512;     // hops per walk before its units are left where it stands

// Hub distribution (between the two walker passes): a hub that holds excess
// hands it to its qualifying arcs, one workgroup per chunk claiming its share
// with one returning atomic (as the sweeps' hub chunks do); the fed nodes are
// listed for the second walker pass.
template <bool CP>
__global__ __launch_bounds__(BLK) void k_aug_hub(DG g, int sseq, int slack) {
    __shared__ long long sh[WPB];
    __shared__ long long s_take;
    if (!g.ctl->bf_done) return;
    const int nx = g.ctl->n_exc;
    if (nx == 0 || nx > g.aug_k) return;
    const HItem it = g.hitems[blockIdx.x];
    const int x = it.node;
    const long long E = atom_load(&g.excess[x]);
    if (E <= 0) return;
    const Front F = g.sf[sseq % 3];
    const long long eps = g.ctl->eps;
    const long long dx = atom_load(&g.dist[ni(x)]);
    const long long px = g.p0[ni(x)];
    long long r[PER_T], adm[PER_T], uc[PER_T];
    int w[PER_T], rv[PER_T];
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < PER_T; ++k) {
        const int a = it.begin + threadIdx.x * PER_T + k;
        r[k] = 0;
        w[k] = 0;
        rv[k] = 0;
        uc[k] = 0;
        adm[k] = 0;
        if (a < it.end) {
            const Pos q = PL<CP>::ld(g, a);
            r[k] = PL<CP>::rc_atomic(g, a);   // the first walker pass claimed with atomics
            w[k] = q.head;
            rv[k] = q.rev;
            uc[k] = q.ucap;
            if (r[k] > 0) {
                const long long cr = q.cost + px - g.p0[ni(q.head)];
                const long long dw = atom_load(&g.dist[ni(q.head)]);
                if (cr <= slack * eps && (dw < dx || (dw == dx && cr < 0))) adm[k] = r[k];
            }
        }
        mine += adm[k];
    }
    long long Ac = 0;
    const long long excl = block_excl_scan(mine, sh, &Ac);
    if (threadIdx.x == 0) {
        long long take = 0;
        if (Ac > 0) {
            const long long start = atom_add_ret(&g.aug_req[it.hid], Ac);
            take = E - start;
            take = take < 0 ? 0 : (take > Ac ? Ac : take);
        }
        s_take = take;
        if (take) atom_add(&g.excess[x], -take);
    }
    __syncthreads();
    long long rt = s_take - excl;
    rt = rt < 0 ? 0 : (rt > mine ? mine : rt);
    int dummy = 0;
#pragma unroll
    for (int k = 0; k < PER_T; ++k) {
        const long long d = adm[k] < rt ? adm[k] : rt;
        rt -= d;
        if (d <= 0) continue;
        const int a = it.begin + threadIdx.x * PER_T + k;
        PL<CP>::set_rc(g, a, r[k] - d);   // only this chunk touches the pair in this kernel
        PL<CP>::set_rc(g, rv[k], uc[k] - (r[k] - d));
        const long long now = atom_add_ret(&g.excess[w[k]], d) + d;
        if (now > 0) {
            mark(g, F, w[k], dummy);
            const int idx = atomicAdd(&g.ctl->n_xl2, 1);
            if (idx < AUG_K2) g.xl2[idx] = w[k];
        }
    }
}

// mode 0: from the apply's excess nodes (non-hubs); mode 1: from the nodes a hub
// distribution (k_aug_hub) fed.
template <bool CP>
__global__ __launch_bounds__(WAVE) void k_augment(DG g, int sseq, int mode, int slack) {
    if (!g.ctl->bf_done) return;
    const int nx = g.ctl->n_exc;
    if (nx == 0 || nx > g.aug_k) return;
    const int cnt = mode ? min(g.ctl->n_xl2, AUG_K2) : nx;
    if ((int)blockIdx.x >= cnt) return;
    const int lane = lane_id();
    const Front F = g.sf[sseq % 3];
    const long long eps = g.ctl->eps;
    int u = mode ? g.xl2[blockIdx.x] : g.xl[blockIdx.x];
    if (u < 0 || u >= g.hub_base) return;   // hubs: k_aug_hub
    long long carry = 0;
    if (lane == 0) carry = atom_exch(&g.excess[u], 0LL);
    carry = __shfl(carry, 0);
    if (carry <= 0) {
        if (lane == 0 && carry < 0) atom_add(&g.excess[u], carry);   // (not an excess node any more)
        return;
    }
    long long du = atom_load(&g.dist[ni(u)]);
    long long pu = g.p0[ni(u)];
    int b0, en;
    seg_of(g.p0, u, b0, en);
    // A hop is two dependent levels: [u's records] → [their heads' records: price,
    // distance, segment]; then the claim on the chosen arc, the next node's excess and
    // the next node's first 64 records are all in flight at once (the head's segment
    // came with its record), so the next hop starts from loaded records.
    Pos q0{};
    if (lane < en - b0) q0 = PL<CP>::ld(g, b0 + lane);
    int hops = 0, reached = 0, dummy = 0;
    for (int step = 0; step < AUG_STEPS; ++step) {
        // the qualifying residual arc of least d(w) (ties: lowest position)
        long long bd = INF64, bp = 0, br = 0;
        unsigned long long bseg = 0;
        int ba = -1, bw = 0, brev = 0;
        for (int base = b0; base < en; base += WAVE) {
            const int a = base + lane;
            Pos q{};
            if (base == b0) q = q0;
            else if (a < en) q = PL<CP>::ld(g, a);
            long long key = INF64, pw = 0;
            unsigned long long sg = 0;
            if (a < en) {
                // (the record's residual may be stale under other walkers' claims: the CAS below corrects it)
                pw = g.p0[ni(q.head)];
                const long long dw = atom_load(&g.dist[ni(q.head)]);
                sg = (unsigned long long)g.p0[ni(q.head) + ND_SEG];
                const long long cr = q.cost + pu - pw;
                if (q.rcap > 0 && cr <= slack * eps && (dw < du || (dw == du && cr < 0))) key = dw;
            }
            const long long mn = wave_min(key);
            if (mn < bd) {
                const unsigned long long hit = __ballot(key == mn);
                const int src = __ffsll((long long)hit) - 1;
                bd = mn;
                ba = base + src;
                bw = __shfl(q.head, src);
                brev = __shfl(q.rev, src);
                br = __shfl(q.rcap, src);
                bp = __shfl(pw, src);
                bseg = (unsigned long long)__shfl((long long)sg, src);
            }
        }
        if (ba < 0) break;
        // in flight together: the next node's first records, its excess, the claim
        const int nb0 = (int)(unsigned)(bseg & 0xffffffffULL), nen = (int)(unsigned)(bseg >> 32);
        Pos qn{};
        if (lane < nen - nb0) qn = PL<CP>::ld(g, nb0 + lane);
        long long take = 0, ew = 0;
        if (lane == 0) {
            ew = atom_load(&g.excess[bw]);
            long long r = br;
            for (;;) {   // claim min(carry, residual) on arc ba
                take = r < carry ? r : carry;
                if (take <= 0) {
                    take = 0;
                    break;
                }
                long long exp = r;
                if (PL<CP>::cas_rc(g, ba, exp, r - take)) break;
                r = exp;
            }
            if (take > 0) PL<CP>::add_rc(g, brev, take);
            if (take < carry) {   // the rest stays at u
                atom_add(&g.excess[u], carry - take);
                mark(g, F, u, dummy);
            }
        }
        take = __shfl(take, 0);
        if (take == 0) {
            carry = 0;   // deposited at u above
            break;
        }
        carry = take;
        ++hops;
        u = bw;
        du = bd;
        if (lane == 0 && (ew < 0 || u >= g.hub_base)) {   // a deficit (or a hub: the hub distribution takes over)
            const long long now = atom_add_ret(&g.excess[u], carry) + carry;
            if (now > 0) mark(g, F, u, dummy);
            reached = ew < 0 ? 1 : 0;
            carry = 0;
        }
        carry = __shfl(carry, 0);
        if (carry == 0) break;
        pu = bp;
        b0 = nb0;
        en = nen;
        q0 = qn;
    }
    if (lane == 0) {
        if (carry > 0) {   // hop limit or no qualifying arc: the units stay at u
            atom_add(&g.excess[u], carry);
            mark(g, F, u, dummy);
        }
        const int sh = (int)blockIdx.x & (CTR_SHARDS - 1);
        atomicAdd(reached ? &g.ctl->aug_reached : &g.ctl->aug_short, 1);
        if (reached) atomicAdd(g.ctr + sh * NCTR + C_AUGWALK, 1ULL);
        if (hops) atomicAdd(g.ctr + sh * NCTR + C_AUGHOP, (unsigned long long)hops);
    }
}

// ------------------------------------------------- forward tail update ---
// Once only a few nodes hold excess, a global update (Bellman-Ford from every
// deficit over the whole graph, ~40–60 rounds) moves about one unit per cycle.
// The forward update searches from the excess nodes instead: distances d_f
// over residual arcs of length floor(rc/ε)+1 (≥ 0), stopping at the nearest
// deficit's distance D, then p ← p − ε·max(0, D − d_f) — the dual step of a
// successive-shortest-path solver. Every residual arc keeps length ≥ 0
// (ε-optimality), and each arc of a shortest path from an excess node to a
// deficit at distance D ends with reduced cost in [−ε, 0) (admissible), so one
// unit per such deficit is pushed along the search's parent arcs (k_fs_trace).
// The search touches only the nodes nearer than D (thousands, not the graph).
// A node's key — its record's dist slot — packs d_f above the arc that set it.
__device__ __forceinline__ long long fs_dist(long long key) { return key >> FS_PB; }

// Append the lanes with on set to list l (wave-aggregated); overflow fails the search.
__device__ __forceinline__ void fs_append(const DG& g, int l, bool on, int v) {
    const unsigned long long m = __ballot(on);
    if (!m) return;
    int base = 0;
    if (lane_id() == 0) base = atomicAdd(&g.ctl->fs_cnt[l], (int)__popcll(m));
    base = __shfl(base, 0);
    if (on) {
        const int idx = base + (int)__popcll(m & ((1ULL << lane_id()) - 1));
        if (idx < g.fl_cap) g.fl[(size_t)l * g.fl_cap + idx] = v;
        else g.ctl->fs_fail = 1;
    }
}

// Init: every excess node is a source (d_f 0, no parent), everything else
// unreached; the sources are the first round's frontier. A search still running
// (fs_pending: set by its first round, cleared by k_fs_end once it finished —
// in this cycle's earlier update or the last cycle) is continued instead.
__global__ void k_fs_init(DG g, int seq0) {
    if (g.ctl->fs_pending) return;
    clear_fronts(g, g.bf);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(&g.ctl->fs_D, INF64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g.ctl->fs_done = 0;
        g.ctl->fs_fail = 0;
        g.ctl->fs_rounds = 0;
        g.ctl->n_fdef = 0;
        g.ctl->fs_moved = 0;   // (n_exc was reset by the last cycle's end: this kernel counts into it)
        g.ctl->fs_maxcnt = 0;
    }
    const int l0 = seq0 % 3;
    for (long long v0 = blockIdx.x * (long long)BLK; v0 < g.hub_base; v0 += (long long)gridDim.x * BLK) {
        const long long v = v0 + threadIdx.x;
        long long e = 0;
        if (v < g.hub_base) {
            e = atom_load(&g.excess[v]);
            g.dist[ni(v)] = e > 0 ? FS_NONE : INF64;
        }
        const unsigned long long m = __ballot(e > 0);
        if (m && lane_id() == 0) atomicAdd(&g.ctl->n_exc, (int)__popcll(m));
        const long long units = wave_sum(e > 0 ? e : 0);
        if (units && lane_id() == 0) atom_add(&g.ctl->u_exc, units);
        fs_append(g, l0, e > 0, (int)v);
    }
    if (blockIdx.x == 0)
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) {
            drain_inbox(g, h);
            const long long e = atom_load(&g.excess[g.hub_base + h]);
            g.dist[ni(g.hub_base + h)] = e > 0 ? FS_NONE : INF64;
            if (e > 0) {
                g.bf[l0].hub[h] = 1;
                atomicAdd(&g.ctl->n_exc, 1);
                atom_add(&g.ctl->u_exc, e);
            }
        }
}

// Relax residual out-arc a of u (distance du, price pu). Returns 1 when a
// non-hub, non-deficit head w was lowered and is not yet listed for the next round.
template <bool CP>
__device__ __forceinline__ int fs_relax(const DG& g, const Front& N, int a, long long du, long long pu, long long eps,
                                        double inv, long long B, int& wout) {
    const Pos q = PL<CP>::ld_nr(g, a);
    const int w = q.head;
    const long long pw = g.p0[ni(w)];
    const long long kw = atom_load(&g.dist[ni(w)]);
    const long long ew = atom_load(&g.excess[w]);
    if (q.rcap <= 0) return 0;
    long long len = ks_floordiv_inv(q.cost + pu - pw, eps, inv) + 1;
    len = len < 0 ? 0 : (len > LEN_CAP ? LEN_CAP : len);
    const long long cand = du + len;
    if (cand > B || cand >= FS_DMAX || cand >= fs_dist(kw)) return 0;
    const long long key = (cand << FS_PB) | (long long)a;
    if (key >= atom_min_ret(&g.dist[ni(w)], key)) return 0;
    if (ew < 0) {   // a deficit: the search's bound; paths end here
        __hip_atomic_fetch_min(&g.ctl->fs_D, cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0;
    }
    if (w >= g.hub_base) {
        N.hub[w - g.hub_base] = 1;
        return 0;
    }
    if (N.flag[w]) return 0;
    N.flag[w] = 1;
    wout = w;
    return 1;
}

// One round: the listed nodes (one wave per node, 64 arcs per batch) and the
// flagged hubs (HSPLIT workgroups per 1024-arc chunk) relax their out-arcs.
template <bool CP>
__global__ __launch_bounds__(BLK) void k_fs_round(DG g, int seq) {
    const int lin = seq % 3, lout = (seq + 1) % 3;
    const Front F = g.bf[lin], N = g.bf[lout];
    if (blockIdx.x == 0) {   // the buffers round seq + 1 appends to were read by round seq − 1
        for (int h = threadIdx.x; h < g.nheavy; h += BLK) g.bf[(seq + 2) % 3].hub[h] = 0;
        if (threadIdx.x == 0) g.ctl->fs_cnt[(seq + 2) % 3] = 0;
    }
    const int done = g.ctl->fs_done | g.ctl->fs_fail;
    const int cnt = g.ctl->fs_cnt[lin];
    const long long B = atom_load(&g.ctl->fs_D);
    const long long eps = g.ctl->eps;
    const double inv = g.ctl->inv;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !done) {
        int hub_any = 0;
        for (int h = 0; h < g.nheavy; ++h) hub_any += F.hub[h];
        if (cnt == 0 && !hub_any) g.ctl->fs_done = 1;   // empty frontier: converged
        else {
            g.ctl->fs_pending = 1;   // the next init (this cycle's or the next's) continues it
            g.ctl->fs_rounds += 1;
            atomicAdd(g.ctr + C_BFROUND, 1ULL);
            const int width = cnt + 1024 * hub_any;
            if (width > g.ctl->fs_maxcnt) g.ctl->fs_maxcnt = width;
            // a frontier this wide (a hub's arcs in reach) costs more per unit than
            // the global update it replaces: fail the search as wide
            if (width > g.fs_wide) g.ctl->fs_fail = 2;
        }
    }
    if (done) return;
    const int nhb = g.nhitems * HSPLIT;
    const int lane = lane_id();
    long long scans = 0;   // residual out-arcs examined (the round's units, ks_result.fs_arc_scans)
    auto count = [&]() {
        scans = wave_sum(scans);
        if (lane == 0 && scans) {
            const int sh = ((blockIdx.x * WPB) + (threadIdx.x >> 6)) & (CTR_SHARDS - 1);
            atomicAdd(g.ctr + sh * NCTR + C_FSSCAN, (unsigned long long)scans);
        }
    };
    if ((int)blockIdx.x < nhb) {
        const HItem it = g.hitems[blockIdx.x / HSPLIT];
        if (!F.hub[it.hid]) return;
        const long long du = fs_dist(atom_load(&g.dist[ni(it.node)]));
        const long long pu = g.p0[ni(it.node)];
        const int sub = (int)blockIdx.x % HSPLIT;
        for (int k = 0; k < BF_PER_T; ++k) {
            const int a = it.begin + sub * (CHUNK / HSPLIT) + threadIdx.x * BF_PER_T + k;
            int w = -1;
            const int add = a < it.end ? fs_relax<CP>(g, N, a, du, pu, eps, inv, B, w) : 0;
            scans += a < it.end;
            fs_append(g, lout, add, w);
        }
        count();
        return;
    }
    // listed nodes: one wave each, 64 arcs per pass (eight nodes per wave with eight
    // lanes each was measured slower: a wave then walked its wider nodes — machines —
    // one after another, lengthening the round's chain)
    const int nw = ((int)gridDim.x - nhb) * WPB;
    for (int i = ((int)blockIdx.x - nhb) * WPB + (int)(threadIdx.x >> 6); i < cnt; i += nw) {
        const int v = g.fl[(size_t)lin * g.fl_cap + i];
        const long long key = atom_load(&g.dist[ni(v)]);
        const long long pu = g.p0[ni(v)];
        const long long ev = atom_load(&g.excess[v]);
        int b0, b1;
        seg_of(g.p0, v, b0, b1);
        if (lane == 0) F.flag[v] = 0;
        if (ev < 0) continue;   // a deficit ends its paths
        const long long du = fs_dist(key);
        for (int base = b0; base < b1; base += WAVE) {
            const int a = base + lane;
            int w = -1;
            const int add = a < b1 ? fs_relax<CP>(g, N, a, du, pu, eps, inv, B, w) : 0;
            scans += a < b1;
            fs_append(g, lout, add, w);
        }
    }
    count();
}

// Apply the dual step of a converged search: p ← p − ε·(D − d_f) below D, and
// list the deficits found at distance D for the trace.
__global__ void k_fs_apply(DG g) {
    if (!g.ctl->fs_done || g.ctl->fs_fail) return;
    if (atom_load_i(&g.ctl->n_exc) == 0) return;   // no excess left: nothing to search from
    const long long D = atom_load(&g.ctl->fs_D);
    if (D >= FS_DMAX) {   // no deficit in range: a backward update decides (infeasible or not)
        if (blockIdx.x == 0 && threadIdx.x == 0) g.ctl->fs_fail = 1;
        return;
    }
    const long long eps = g.ctl->eps;
    if (D > g.ctl->lim) {   // ε·D would overflow the prices: a backward update instead
        if (blockIdx.x == 0 && threadIdx.x == 0) g.ctl->fs_fail = 1;
        return;
    }
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK) {
        const long long d = fs_dist(atom_load(&g.dist[ni(v)]));
        if (d < D) {
            const long long np = g.p0[ni(v)] - eps * (D - d);
            g.p0[ni(v)] = np;
            g.p1[ni(v)] = np;
        } else if (d == D && atom_load(&g.excess[v]) < 0) {
            const int idx = atomicAdd(&g.ctl->n_fdef, 1);
            if (idx < FDEF_CAP) g.fdef[idx] = (int)v;
        }
    }
}

// Trace: one unit (or the path's bottleneck) from each listed deficit back along
// the parent arcs to its excess node — one wave per deficit, all in parallel.
// Lane 0 walks the parents (each arc must end at the node it was reached from,
// be residual, and be admissible under the updated prices) into an LDS path;
// the wave then claims the source's excess with a CAS and every arc of the path
// at once (one lane per arc, CAS against the residual); if any arc is short
// (another wave took it) every claim is rolled back and the unit waits for the
// next update. Then the reverse residuals and the deficit are credited.
constexpr int FS_PATH = 512;       // hops a trace may take
template <bool CP>
__global__ __launch_bounds__(WAVE) void k_fs_trace(DG g) {
    __shared__ int path[FS_PATH];
    __shared__ int s_len, s_src;
    __shared__ long long s_amt;
    if (!g.ctl->fs_done || g.ctl->fs_fail) return;
    if ((int)blockIdx.x >= min(g.ctl->n_fdef, FDEF_CAP)) return;
    const int lane = threadIdx.x;
    const int t = g.fdef[blockIdx.x];
    if (lane == 0) {
        long long amt = -atom_load(&g.excess[t]);
        int v = t, src = -1, len = 0;
        while (amt > 0 && len < FS_PATH) {
            const long long key = atom_load(&g.dist[ni(v)]);
            const long long a = key & FS_NONE;
            if (a == FS_NONE) {
                src = v;
                break;
            }
            if (a >= g.npos) break;   // (a key not written by this search)
            const Pos q = PL<CP>::ld(g, (int)a);
            const long long r = PL<CP>::rc_atomic(g, (int)a);
            const int u = PL<CP>::head(g, q.rev);
            if (q.head != v || r <= 0 || q.cost + g.p0[ni(u)] - g.p0[ni(v)] >= 0) break;
            amt = r < amt ? r : amt;
            path[len++] = (int)a;
            v = u;
        }
        if (src >= 0 && src != t) {   // claim the source's excess
            long long e = atom_load(&g.excess[src]);
            for (;;) {
                const long long take = e < amt ? e : amt;
                if (take <= 0) {
                    src = -1;
                    break;
                }
                long long exp = e;
                if (__hip_atomic_compare_exchange_strong(&g.excess[src], &exp, e - take, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    amt = take;
                    break;
                }
                e = exp;
            }
        } else {
            src = -1;
        }
        s_len = len;
        s_src = src;
        s_amt = amt;
    }
    __syncthreads();
    const int len = s_len, src = s_src;
    const long long amt = s_amt;
    if (src < 0) return;
    // claim every arc of the path at once
    bool ok = true;
    unsigned long long mine = 0;   // bit i: this lane holds the claim on path[lane + 64 i]
    for (int i = lane, k = 0; i < len; i += WAVE, ++k) {
        long long r = PL<CP>::rc_atomic(g, path[i]);
        for (;;) {
            if (r < amt) {
                ok = false;
                break;
            }
            long long exp = r;
            if (PL<CP>::cas_rc(g, path[i], exp, r - amt)) {
                mine |= 1ULL << k;
                break;
            }
            r = exp;
        }
    }
    const bool all = __all(ok);
    for (int i = lane, k = 0; i < len; i += WAVE, ++k) {
        if (!(mine >> k & 1)) continue;
        if (all) PL<CP>::add_rc(g, PL<CP>::rev(g, path[i]), amt);
        else PL<CP>::add_rc(g, path[i], amt);   // roll back
    }
    if (lane == 0) {
        if (all) {
            atom_add(&g.excess[t], amt);
            atomicAdd(&g.ctl->fs_moved, 1);
            atomicAdd(&g.ctl->fs_moved_cyc, 1);
        } else {
            atom_add(&g.excess[src], amt);   // the unit stays for the next update
        }
    }
}

// End of a forward update: a finished (or failed) search releases the init and
// reports its excess counts; one still running keeps them (its init is skipped).
__global__ void k_fs_end(DG g) {
    if (threadIdx.x || blockIdx.x) return;
    if (!g.ctl->fs_done && !g.ctl->fs_fail) return;
    g.ctl->fs_pending = 0;
    g.ctl->fs_cnt[0] = g.ctl->fs_cnt[1] = g.ctl->fs_cnt[2] = 0;
    g.ctl->n_exc_rep = atom_load_i(&g.ctl->n_exc);
    g.ctl->u_exc_rep = atom_load(&g.ctl->u_exc);
    g.ctl->n_exc = 0;
    g.ctl->u_exc = 0;
    if (g.ctl->fs_done && !g.ctl->fs_fail) g.ctl->fs_completed += 1;
}

// TESTS ONLY (ks_opts.fault_inject bit 6): move one unit on the first arc that can
// take it without touching any excess word — the flow then violates conservation,
// which only the verifier's balance of the arc flows can see.
__global__ void k_break_conservation(DG g, long long m2) {
    if (threadIdx.x || blockIdx.x) return;
    for (long long p = 0; p < m2; ++p) {
        const Pos q = g.pos[p];
        if (q.rcap > 0 && q.ucap > 0 && q.cost < (1LL << 50)) {
            g.pos[p].rcap = q.rcap - 1;
            g.pos[q.rev].rcap += 1;
            return;
        }
    }
}

// TESTS ONLY (ks_opts.fault_inject bit 1): lower one node's price by delta after
// the solve, so the certificate fails on an optimal flow and must be repaired.
__global__ void k_perturb_price(DG g, int x, long long delta) {
    if (x < g.n) {
        g.p0[ni(x)] -= delta;
        g.p1[ni(x)] -= delta;
    }
}

// PR success: p ← p − ε·d. From d ≡ 0 (d ≤ 0) prices only rise, keeping their
// history. From d = p at ε = 1 the fixpoint is d(u) = p(u) + min(0, min_w dist(u, w))
// over residual paths of length cost + 1 per arc, so p − d = −min(0, min_w dist(u, w)):
// the canonical prices of the flow, the same for any prices it started from
// (warm_canon: the drift of carried prices).
__global__ void k_pr_apply(DG g, int packed) {
    if (!g.ctl->bf_done) return;
    const long long eps = g.ctl->eps;
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK) {
        const long long d = atom_load(&g.dist[ni(v)]);
        const long long np = g.p0[ni(v)] - eps * (packed ? pk_d(d) : d);
        g.p0[ni(v)] = np;
        g.p1[ni(v)] = np;
    }
}

// ------------------------------------------- cycle-cancelling refinement ---
// The finish that replaces the final cost-scaling phase: the flow of
// the last coarse phase is feasible and nearly optimal, and what keeps it from
// optimality is a few negative cycles (CPU prototype tools/proto/cycle_cancel.c:
// 11–13 on config 3, 24–120 arcs of cost −1…−4 each). The refinement's
// Bellman-Ford (PR = 2) records each node's parent; when it has not converged
// after a batch of rounds, the parent graph — one parent per node, so its cycles
// are node-disjoint — is searched: pointer doubling (2^k steps) lands every node
// of a cycle no longer than that, the least id of each window groups a cycle, its
// nodes sum the cost and take the bottleneck with atomics, a group that is not a
// union of cycles (nodes disagreeing on the id, a non-residual arc, a node with
// other than one member pointing at it) is dropped, and every good negative group
// pushes its bottleneck around in parallel; the cycle's nodes rejoin the frontier.
// The refinement then continues; once its frontier drains, every residual arc
// meets d(u) ≤ d(v) + len(u, v): the prices p − d certify the flow optimal.
[[maybe_unused]] constexpr int CYC_WALK = 1 << CYC_LOG;
constexpr int CYC_SHORT = 7;              // a short search's doubling steps
// refinement rounds between parent-graph searches: 4 where the whole
// search is one workgroup's LDS pass (small graphs: a search costs ~3 rounds),
// 8 for the multi-launch search of large graphs (twice the launches for no gain)
constexpr int CYC_EVERY_LDS = 4;
constexpr int CYC_EVERY = 8;
constexpr int CYC_PERIODS = 3;            // rounds + search periods per host check
constexpr long long kPrcUnitsDiv = 4;   // an earlier finish (run_phase prc_early)

// The parent of every node (itself for a root) from its key's position a (the
// parent v is the head of a's reverse); the jump word (node one step ahead, least
// id over the one-node window = its own id); the per-group sums reset.
template <bool CP>
__global__ void k_cyc_par(DG g, int* __restrict__ J0, int2* __restrict__ JM, int* __restrict__ onc,
                          int* __restrict__ R, long long* __restrict__ gsum, long long* __restrict__ gcap,
                          int* __restrict__ gbad, int* __restrict__ indeg) {
    if (g.ctl->bf_done) return;   // the refinement converged: no search
    if (blockIdx.x == 0 && threadIdx.x == 0) g.ctl->t_srch = __builtin_amdgcn_s_memrealtime();
    for (long long u = blockIdx.x * (long long)BLK + threadIdx.x; u < g.n; u += (long long)gridDim.x * BLK) {
        const long long a = atom_load(&g.dist[ni(u)]) & PK_NONE;
        int v = (int)u;
        if (a != PK_NONE) v = PL<CP>::head(g, PL<CP>::rev(g, (int)a));
        J0[u] = v;
        JM[u] = make_int2(v, (int)u);
        R[u] = (int)a;
        onc[u] = 0;
        gsum[u] = 0;
        gcap[u] = INF64;
        gbad[u] = 0;
        indeg[u] = 0;
    }
}
// One jump step: a window of w nodes → F·w (F jumps of the previous step chained;
// F = 4 per launch where the window allows, 2 for an odd power of two: a search
// covers 128 steps in 4 launches, 1,024 in 5, instead of 7 and 10 doublings). The
// jump word packs the node w steps ahead and the least id over the window. On the
// search's last step (mark) every node a window ahead of another is marked — it
// lies on a cycle, or (past the window) on a chain, which the union-of-cycles test
// rejects; roots (their own parent) are skipped.
template <int F>
__global__ void k_cyc_jump(int n, const int* __restrict__ done, const int2* __restrict__ JMi,
                           int2* __restrict__ JMo, int mark, const int* __restrict__ J0, int* __restrict__ onc) {
    if (*done) return;
    for (long long u = blockIdx.x * (long long)BLK + threadIdx.x; u < n; u += (long long)gridDim.x * BLK) {
        int2 c = JMi[u];
        int mn = c.y;
#pragma unroll
        for (int f = 1; f < F; ++f) {
            const int2 x = JMi[c.x];
            mn = min(mn, x.y);
            c.x = x.x;
        }
        JMo[u] = make_int2(c.x, mn);
        if (mark && J0[c.x] != c.x) onc[c.x] = 1;
    }
}
// Each cycle node adds its parent arc (u → v, the reverse of position R[u]) to its
// group — the least id of its window, the cycle's least id when the cycle has at
// most CYC_WALK nodes: cost sum, bottleneck residual. A group whose nodes disagree
// on the group (a longer cycle) or whose arc is not residual is marked bad.
template <bool CP>
__global__ void k_cyc_group(DG g, const int* __restrict__ J0, const int2* __restrict__ MK, const int* __restrict__ onc,
                            const int* __restrict__ R, long long* __restrict__ gsum, long long* __restrict__ gcap,
                            int* __restrict__ gbad, int* __restrict__ indeg) {
    if (g.ctl->bf_done) return;
    for (long long u = blockIdx.x * (long long)BLK + threadIdx.x; u < g.n; u += (long long)gridDim.x * BLK) {
        if (!onc[u] || J0[u] == (int)u) continue;
        const int m = MK[u].y, mn = MK[J0[u]].y;
        // a parent off the group (another group, or unmarked): u's arc leaves the
        // group, which is then no union of cycles. The parent's group is not blamed:
        // it counts only its own members' pointers (a chain of another group that
        // runs into a cycle leaves the cycle's group intact, and cancelling it moves
        // nothing the chain's group owns).
        if (mn != m || !onc[J0[u]]) gbad[m] = 1;
        else atomicAdd(&indeg[J0[u]], 1);
        const Pos q = PL<CP>::ld_nr(g, R[u]);
        const long long res = q.ucap - q.rcap;   // residual of the reverse: the arc u → v
        if (res <= 0) gbad[m] = 1;
        atom_add(&gsum[m], -q.cost);
        __hip_atomic_fetch_min(&gcap[m], res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// A group is a union of cycles only if each of its nodes has exactly one member
// of the group pointing at it (and every member's parent is a member, k_cyc_group):
// each member then has one push out and one push in. A chain longer than the
// doubling window (its nodes marked too) that joins a cycle's group gives the
// junction two, its first node none, and the group is dropped (pushing along a
// chain would break conservation).
// Such nodes are counted (ctl->cyc_rej); apply = 0 (TESTS ONLY, fault_inject bit 8)
// counts them without dropping their groups.
__global__ void k_cyc_check(int n, const int* __restrict__ done, const int* __restrict__ J0,
                            const int2* __restrict__ MK, const int* __restrict__ onc, const int* __restrict__ indeg,
                            int* __restrict__ gbad, int apply, int* __restrict__ rej) {
    if (*done) return;
    int cnt = 0;
    for (long long u = blockIdx.x * (long long)BLK + threadIdx.x; u < n; u += (long long)gridDim.x * BLK)
        if (onc[u] && J0[u] != (int)u && atom_load_i(&indeg[u]) != 1) {
            if (apply) gbad[MK[u].y] = 1;
            ++cnt;
        }
    cnt = (int)wave_sum(cnt);
    if (cnt && lane_id() == 0) atomicAdd(rej, cnt);
}

// Cancel every good negative group: each of its nodes pushes the bottleneck along
// its own parent arc (the arcs of different nodes are different positions), and
// rejoins the frontier the next refinement round reads (buffer seq).
template <bool CP>
__global__ void k_cyc_push(DG g, const int* __restrict__ J0, const int2* __restrict__ MK, const int* __restrict__ onc,
                           const int* __restrict__ R, const long long* __restrict__ gsum,
                           const long long* __restrict__ gcap, const int* __restrict__ gbad, int seq) {
    if (g.ctl->bf_done) return;
    const Front F = g.bf[seq % 3];
    int out = 0, cyc = 0;
    for (long long u = blockIdx.x * (long long)BLK + threadIdx.x; u < g.n; u += (long long)gridDim.x * BLK) {
        if (!onc[u] || J0[u] == (int)u) continue;
        const int m = MK[u].y;
        const long long dl = gcap[m];
        if (gbad[m] || gsum[m] >= 0 || dl <= 0 || dl >= INF64) continue;
        const int a = R[u];
        const Pos q = PL<CP>::ld(g, a);
        PL<CP>::set_rc(g, a, q.rcap + dl);        // the arc u → v is rev(a): its residual falls by dl
        PL<CP>::add_rc(g, q.rev, -dl);
        mark(g, F, (int)u, out);
        cyc += u == m;
    }
    if (__any(out) && lane_id() == 0) g.ctl->bfa[seq % 3] = 1;
    cyc = (int)wave_sum(cyc);
    if (cyc && lane_id() == 0) atomicAdd(&g.ctl->cyc_done, cyc);
}

// The whole search in ONE workgroup with the parent graph in LDS (graphs of at most
// CYC_LDS_K · 1024 internal ids that the LDS holds: config 2's cells). Round 5
// measured a one-workgroup search over global memory slower than the 12 launches;
// here every doubling step, the marks and the in-degrees stay in LDS — three words
// per node: the parent (J0) and the doubling words (jump | least id << CYC_LDS_IDB,
// double-buffered as in the cell solver; the free buffer holds the in-degrees
// afterwards). Each thread owns CYC_LDS_K nodes and issues their loads together
// (the parents' keys, then the reverse positions, then the heads: three dependent
// levels in all, not three per node). Only the marked nodes touch global memory
// after that: their group sums (zeroed by the group's own members) and the pushes.
// Same steps and the same union-of-cycles test as k_cyc_par … k_cyc_push.
constexpr int CYC_LDS_T = 1024;
constexpr int CYC_LDS_K = 14;              // nodes per thread
constexpr int CYC_LDS_IDB = 15;
constexpr int CYC_LDS_IDM = (1 << CYC_LDS_IDB) - 1;
constexpr int CYC_LDS_ON = 1 << 30;
constexpr int CYC_LDS_MAX = CYC_LDS_K * CYC_LDS_T;   // (< 2^15: ids fit the packed word)
static_assert(CYC_LDS_MAX <= CYC_LDS_IDM, "node ids must fit the packed doubling word");
__host__ __device__ constexpr size_t cyc_lds_bytes(int n) { return (size_t)3 * sizeof(int) * (size_t)n; }

template <bool CP>
__global__ __launch_bounds__(CYC_LDS_T) void k_cyc_lds(DG g, int lg, int apply_check, int seq,
                                                      long long* __restrict__ gsum, long long* __restrict__ gcap,
                                                      int* __restrict__ gbad) {
    if (g.ctl->bf_done) return;   // the refinement converged: no search
    if (threadIdx.x == 0) g.ctl->t_srch = __builtin_amdgcn_s_memrealtime();
    extern __shared__ int cyc_sm[];
    const int n = g.n;
    int* J0 = cyc_sm;
    int* Wi = cyc_sm + n;
    int* Wo = Wi + n;
    const int t = threadIdx.x;
    {   // parents: each level's loads for all of this thread's nodes issued together
        long long key[CYC_LDS_K];
        int rv[CYC_LDS_K], hd[CYC_LDS_K];
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) {
            const int u = t + k * CYC_LDS_T;
            key[k] = u < n ? atom_load(&g.dist[ni(u)]) & PK_NONE : PK_NONE;
        }
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) rv[k] = PL<CP>::rev(g, key[k] != PK_NONE ? (int)key[k] : 0);
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) hd[k] = PL<CP>::head(g, rv[k]);
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) {
            const int u = t + k * CYC_LDS_T;
            if (u < n) {
                const int v = key[k] != PK_NONE ? hd[k] : u;
                J0[u] = v;
                Wi[u] = v | (u << CYC_LDS_IDB);
            }
        }
    }
    __syncthreads();
    for (int d = 0; d < lg; ++d) {   // 2^d steps ahead, then 2^d more; the least id over them
        int w[CYC_LDS_K], wx[CYC_LDS_K];
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) {
            const int u = t + k * CYC_LDS_T;
            w[k] = u < n ? Wi[u] : 0;
        }
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) wx[k] = Wi[w[k] & CYC_LDS_IDM];
#pragma unroll
        for (int k = 0; k < CYC_LDS_K; ++k) {
            const int u = t + k * CYC_LDS_T;
            if (u < n)
                Wo[u] = (wx[k] & CYC_LDS_IDM) | (min(w[k] >> CYC_LDS_IDB, wx[k] >> CYC_LDS_IDB) << CYC_LDS_IDB);
        }
        __syncthreads();
        int* tmp = Wi;
        Wi = Wo;
        Wo = tmp;
    }
    // every node a window ahead of another lies on a cycle (or, past the window, on
    // a chain — the test below); roots are skipped. Wo now holds the in-degrees.
    for (int u = t; u < n; u += CYC_LDS_T) {
        const int x = Wi[u] & CYC_LDS_IDM;
        if (J0[x] != x) atomicOr(&Wi[x], CYC_LDS_ON);
        Wo[u] = 0;
    }
    __syncthreads();
    // the marked nodes reset their group's sums (every member writes the same values)
    for (int u = t; u < n; u += CYC_LDS_T) {
        const int w = Wi[u];
        if (!(w & CYC_LDS_ON) || J0[u] == u) continue;
        const int m = (w & ~CYC_LDS_ON) >> CYC_LDS_IDB;
        gsum[m] = 0;
        gcap[m] = INF64;
        gbad[m] = 0;
    }
    __syncthreads();
    for (int u = t; u < n; u += CYC_LDS_T) {
        const int w = Wi[u];
        const int p = J0[u];
        if (!(w & CYC_LDS_ON) || p == u) continue;
        const int m = (w & ~CYC_LDS_ON) >> CYC_LDS_IDB;
        const int wp = Wi[p];
        const int mn = (wp & ~CYC_LDS_ON) >> CYC_LDS_IDB;
        if (mn != m || !(wp & CYC_LDS_ON)) gbad[m] = 1;   // u's arc leaves its group (k_cyc_group)
        else atomicAdd(&Wo[p], 1);
        const int a = (int)(atom_load(&g.dist[ni(u)]) & PK_NONE);
        const Pos q = PL<CP>::ld_nr(g, a);
        const long long res = q.ucap - q.rcap;   // residual of the reverse: the arc u → v
        if (res <= 0) gbad[m] = 1;
        __hip_atomic_fetch_add(&gsum[m], -q.cost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_min(&gcap[m], res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    int rej = 0;
    for (int u = t; u < n; u += CYC_LDS_T) {   // the union-of-cycles test (k_cyc_check)
        const int w = Wi[u];
        if ((w & CYC_LDS_ON) && J0[u] != u && Wo[u] != 1) {
            if (apply_check) gbad[(w & ~CYC_LDS_ON) >> CYC_LDS_IDB] = 1;
            ++rej;
        }
    }
    __syncthreads();
    const Front F = g.bf[seq % 3];
    int out = 0, cyc = 0;
    for (int u = t; u < n; u += CYC_LDS_T) {
        const int w = Wi[u];
        if (!(w & CYC_LDS_ON) || J0[u] == u) continue;
        const int m = (w & ~CYC_LDS_ON) >> CYC_LDS_IDB;
        // (agent-scope loads: the sums were made by atomics in L2, never from a stale L1 line)
        const long long dl = atom_load(&gcap[m]);
        if (atom_load_i(&gbad[m]) || atom_load(&gsum[m]) >= 0 || dl <= 0 || dl >= INF64) continue;
        const int a = (int)(atom_load(&g.dist[ni(u)]) & PK_NONE);
        const Pos q = PL<CP>::ld(g, a);
        PL<CP>::set_rc(g, a, q.rcap + dl);        // the arc u → v is rev(a): its residual falls by dl
        PL<CP>::add_rc(g, q.rev, -dl);
        mark(g, F, u, out);
        cyc += u == m;
    }
    if (__any(out) && lane_id() == 0) g.ctl->bfa[seq % 3] = 1;
    cyc = (int)wave_sum(cyc);
    rej = (int)wave_sum(rej);
    if (lane_id() == 0) {
        if (cyc) atomicAdd(&g.ctl->cyc_done, cyc);
        if (rej) atomicAdd(&g.ctl->cyc_rej, rej);
    }
}

// ================================================================ verify ===
// Conservation, capacity and 1-optimality (scaled units); per-block cost sums.
__global__ void k_drain_all(DG g) {
    const int h = blockIdx.x * BLK + threadIdx.x;
    if (h < g.nheavy) drain_inbox(g, h);
}

constexpr int VERIFY_GRID = 2048;        // most blocks of k_verify_arcs: part holds 2 × 2 × VERIFY_GRID sums (build)
constexpr int VERIFY_COST_RANGE = 8;     // verify_bad: a product flow·cost, or a thread's Σ |flow·cost|, left 64 bits

// Per live arc slot: flow (lower bound included) into flows[s], capacity
// feasibility, the cost sum, and the flow value measured from the resident
// flow: net inflow into the demand nodes (supply < 0).
__global__ void k_verify_arcs(DG g, int hi, const unsigned char* __restrict__ alive, const int* __restrict__ fwd,
                              const int* __restrict__ src, const int* __restrict__ dst,
                              const long long* __restrict__ supply, const long long* __restrict__ low,
                              const long long* __restrict__ cap, const long long* __restrict__ cost,
                              long long* __restrict__ flows, long long* __restrict__ part,
                              long long* __restrict__ partf, long long* __restrict__ bal) {
    __shared__ long long sh[WPB];
    // a hub's balance (the sink, the cluster aggregator: every arc into it adds to
    // one word) is summed in LDS and added once per workgroup — one device atomic
    // per arc on the same word serialised at the memory-side atomic unit (~0.1 ms
    // per config-3 verify)
    __shared__ long long hbal[HUB_LDS];
    __shared__ int hslot[HUB_LDS];
    if (threadIdx.x < HUB_LDS) hbal[threadIdx.x] = 0;
    __syncthreads();
    auto add_bal = [&](int x, int slot, long long v) {
        const int h = x - g.hub_base;
        if (h >= 0 && h < HUB_LDS) {
            __hip_atomic_fetch_add(&hbal[h], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            hslot[h] = slot;   // (every writer stores the same slot)
        } else {
            atom_add(&bal[slot], v);
        }
    };
    long long csum = 0, fsum = 0;
    // Σ |flow·cost| beside the signed sum: below 2^63 no partial sum of the products, in
    // any order, leaves int64, so the total is exact; at or above it the solve reports
    // KS_E_RANGE (include/ksmcmf.h) instead of a wrapped number
    unsigned long long asum = 0;
    int bad = 0, ovf = 0;
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < hi; i += (long long)gridDim.x * BLK) {
        if (!alive[i]) {
            flows[i] = 0;
            continue;
        }
        const int p = fwd[i];
        if (p < 0) {
            bad = 1;
            flows[i] = 0;
            continue;
        }
        const long long cp = cap[i] - low[i];
        const Pos qf = g.pos[p], qr = g.pos[g.pos[p].rev];
        const long long rf = qf.rcap, rr = qr.rcap;
        const long long f = cp - rf;
        if (rf < 0 || rr < 0 || f < 0 || f != rr) bad = 1;
        const long long fl = f + low[i];
        flows[i] = fl;
        if (fl) {   // conservation from the flows themselves (k_verify_balance), not from the excess words
            add_bal(qr.head, src[i], -fl);   // (the reverse position's head is the arc's tail)
            add_bal(qf.head, dst[i], fl);
        }
        long long prod;
        ovf |= __builtin_mul_overflow(fl, cost[i], &prod);
        const unsigned long long mag = prod < 0 ? 0ULL - (unsigned long long)prod : (unsigned long long)prod;
        ovf |= __builtin_add_overflow(asum, mag, &asum);
        csum = (long long)((unsigned long long)csum + (unsigned long long)prod);
        if (supply[dst[i]] < 0) fsum += fl;
        if (supply[src[i]] < 0) fsum -= fl;
    }
    csum = block_sum(csum, sh);
    fsum = block_sum(fsum, sh);
    // the magnitudes in 32-bit halves (a block's sum of either half stays below 2^40)
    const long long ahi = block_sum((long long)(asum >> 32), sh);
    const long long alo = block_sum((long long)(asum & 0xffffffffULL), sh);
    __syncthreads();
    if (threadIdx.x < HUB_LDS && hbal[threadIdx.x]) atom_add(&bal[hslot[threadIdx.x]], hbal[threadIdx.x]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = csum;
        partf[blockIdx.x] = fsum;
        part[gridDim.x + blockIdx.x] = ahi;
        partf[gridDim.x + blockIdx.x] = alo;
    }
    if (__any(bad) && lane_id() == 0) atomicOr(&g.ctl->verify_bad, 1);
    if (__any(ovf) && lane_id() == 0) atomicOr(&g.ctl->verify_bad, VERIFY_COST_RANGE);
}

// Every live node's net inflow plus its supply is zero (the sink's supply is the
// demand set for this solve): conservation of the flow the caller downloads,
// independent of the solver's own excess bookkeeping.
__global__ void k_verify_balance(DG g, int ncap, const unsigned char* __restrict__ alive,
                                 const long long* __restrict__ supply, const long long* __restrict__ bal) {
    int bad = 0;
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK)
        if (alive[v] && atom_load(&bal[v]) + supply[v] != 0) bad = 1;
    if (__any(bad) && lane_id() == 0) atomicOr(&g.ctl->verify_bad, 4);
}

__global__ void k_verify_opt(DG g, long long m2) {
    int bad = 0;
    const long long eps = g.ctl->eps;
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2; p += (long long)gridDim.x * BLK) {
        if (g.pos[p].rcap > 0) {
            const int t = g.pos[g.pos[p].rev].head;
            const long long cr = g.pos[p].cost + g.p0[ni(t)] - g.p0[ni(g.pos[p].head)];
            if (cr < -eps) bad = 1;
        }
    }
    if (__any(bad) && lane_id() == 0) atomicOr(&g.ctl->verify_bad, 2);
}

__global__ void k_verify_nodes(DG g) {
    int bad = 0;
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < g.n; v += (long long)gridDim.x * BLK)
        if (atom_load(&g.excess[v]) != 0) bad = 1;
    if (__any(bad) && lane_id() == 0) atomicOr(&g.ctl->verify_bad, 4);
}

// ======================================================== warm start ===
// Incremental re-solve (config 4). While the CSR stays valid the previous flow
// and prices simply remain in place (the store's kernels keep the residual
// state consistent with every delta). Across a rebuild they are carried by arc
// slot and node slot: saved before, restored (clamped to the new bounds) after.
__global__ void k_save_flows(int hi, const unsigned char* __restrict__ alive, const int* __restrict__ fwd,
                             const Pos* __restrict__ pos, long long* __restrict__ saved) {
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK) {
        const int p = fwd[s];
        saved[s] = (alive[s] && p >= 0) ? pos[pos[p].rev].rcap : 0;
    }
}

__global__ void k_restore_flows(int hi, const unsigned char* __restrict__ alive, const long long* __restrict__ saved,
                                const long long* __restrict__ low, const long long* __restrict__ cap,
                                const int* __restrict__ fwd, const int* __restrict__ src,
                                const int* __restrict__ dst, const int* __restrict__ perm, Pos* __restrict__ pos,
                                long long* __restrict__ excess) {
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK) {
        if (!alive[s]) continue;
        const long long u = cap[s] - low[s];
        long long f = saved[s];
        f = f < 0 ? 0 : (f > u ? u : f);
        if (f > 0) {
            const int p = fwd[s];
            pos[p].rcap = u - f;
            pos[pos[p].rev].rcap = f;
            atom_add(&excess[perm[src[s]]], -f);
            atom_add(&excess[perm[dst[s]]], f);
        }
    }
}

// Per-cell fallback: the cells in rng (node-slot ranges [lo, hi),
// nr of them) restart cold on the multi-kernel engine — their arcs' carried flows
// and their nodes' carried prices are zeroed between the save and the restore.
// *resets counts the live arc slots and node slots it reset (ks_result.fb_resets).
__global__ void k_fb_reset(int hi, int ncap, int nr, const long long* __restrict__ rng, const int* __restrict__ a_src,
                           const unsigned char* __restrict__ alive, long long* __restrict__ saved,
                           long long* __restrict__ pslot, unsigned long long* __restrict__ resets) {
    const long long n = hi > ncap ? hi : ncap;
    unsigned long long cnt = 0;
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const long long vs = i < hi ? a_src[i] : -1, vn = i < ncap ? i : -1;
        bool rs = false, rn = false;
        for (int r = 0; r < nr; ++r) {
            rs |= vs >= rng[2 * r] && vs < rng[2 * r + 1];
            rn |= vn >= rng[2 * r] && vn < rng[2 * r + 1];
        }
        if (rs) saved[i] = 0;
        if (rn) pslot[i] = 0;
        cnt += (rs && alive[i] ? 1 : 0) + (rn ? 1 : 0);
    }
    cnt = (unsigned long long)wave_sum((long long)cnt);
    if (lane_id() == 0 && cnt) atomicAdd(resets, cnt);
}

__global__ void k_save_prices(int ncap, const int* __restrict__ perm, const long long* __restrict__ p0,
                              long long* __restrict__ pslot) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK)
        pslot[v] = p0[ni(perm[v])];
}

// Saved prices by node slot, rescaled when the cost multiplier changed.
__global__ void k_restore_prices(int ncap, int n_prev, long long mult_prev, long long mult,
                                 const long long* __restrict__ pslot, const int* __restrict__ perm,
                                 long long* __restrict__ p0, long long* __restrict__ p1) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        long long p = 0;
        if (v < n_prev) {
            const long long q = pslot[v];
            p = mult == mult_prev ? q : (q / mult_prev) * mult + (q % mult_prev) * mult / mult_prev;
        }
        p0[ni(perm[v])] = p;
        p1[ni(perm[v])] = p;
    }
}

// Warm start: a node whose flow-carrying out-arc got dearer by δ (cost units)
// since the previous solve is priced down by δ·mult, so that arc keeps its
// reduced cost (ks_store.hip k_arc_upserts records δ).
__global__ void k_price_shift(int ncap, const unsigned long long* __restrict__ shift, const int* __restrict__ perm,
                              long long mult, long long* __restrict__ nd) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        const unsigned long long d = shift[v];
        if (!d) continue;
        const int x = perm[v];
        nd[ni(x)] -= (long long)d * mult;
        nd[ni(x) + 2] -= (long long)d * mult;
    }
}

// Nodes created since the previous solve (fresh[v] = 1) get the lowest price
// at which none of their residual out-arcs has a negative reduced cost.
__global__ void k_fresh_prices(int ncap, const unsigned char* __restrict__ fresh, const int* __restrict__ perm, DG g) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        if (!fresh[v]) continue;
        const int x = perm[v];
        long long best = -INF64;
        for (int a = g.first[x]; a < g.first[x + 1]; ++a)
            if (g.pos[a].rcap > 0) best = max(best, g.p0[ni(g.pos[a].head)] - g.pos[a].cost);
        if (best > -INF64) {
            g.p0[ni(x)] = best;
            g.p1[ni(x)] = best;
        }
    }
}

// Largest ε-optimality violation −(c + p(u) − p(w)) over residual arcs → ctl->gu_L.
__global__ void k_max_viol(DG g, long long m2) {
    long long mx = 0;
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2; p += (long long)gridDim.x * BLK) {
        if (g.pos[p].rcap > 0) {
            const long long cr = g.pos[p].cost + g.p0[ni(g.pos[g.pos[p].rev].head)] - g.p0[ni(g.pos[p].head)];
            if (-cr > mx) mx = -cr;
        }
    }
    mx = wave_max(mx);
    if (lane_id() == 0 && mx > 0) __hip_atomic_fetch_max(&g.ctl->gu_L, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// A hot kernel of the solve in the record layout the solve reads;
// KS_HOT_LDS: with LDS bytes of dynamic shared memory.
#define KS_HOT_LDS(CPV, K, GRID, BLKS, LDS, ST, ...)                                            \
    do {                                                                                        \
        if (CPV) K<true><<<dim3(GRID), dim3(BLKS), LDS, ST>>>(__VA_ARGS__);                    \
        else K<false><<<dim3(GRID), dim3(BLKS), LDS, ST>>>(__VA_ARGS__);                       \
    } while (0)
#define KS_HOT(CPV, K, GRID, BLKS, ST, ...) KS_HOT_LDS(CPV, K, GRID, BLKS, 0, ST, __VA_ARGS__)

Engine::Engine() : p_(new EngineImpl) {}
Engine::~Engine() { delete p_; }
int Engine::device() const { return p_->device; }

int Engine::init(int device, const ks_opts& opts, std::string& err) {
    EngineImpl& s = *p_;
    s.device = device;
    s.opts = opts;
    int ndev = 0;
    KS_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        err = "device index out of range";
        return KS_E_DEVICE;
    }
    KS_CHECK(hipSetDevice(device));
    KS_CHECK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    {   // LDS one workgroup may declare (the cell solver's size limit; 160 KiB on gfx950)
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess || v <= 0)
            KS_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        s.lds_limit = (size_t)std::max(v, 0);
    }
    for (auto& e : s.ev) KS_CHECK(hipEventCreate(&e));
    for (auto& e : s.kev) KS_CHECK(hipEventCreate(&e));
    for (auto& e : s.fin_ev) KS_CHECK(hipEventCreate(&e));
    for (auto& c : s.cev)
        for (auto& e : c) KS_CHECK(hipEventCreate(&e));
    for (auto& c : s.fev)
        for (auto& e : c) KS_CHECK(hipEventCreate(&e));
    for (auto& e : s.cdone) KS_CHECK(hipEventCreate(&e));
    for (int i = 0; i < CYC_SLOTS; ++i) {
        KS_CHECK(hipHostMalloc(&s.h_cyc[i], sizeof(Ctl), hipHostMallocCoherent | hipHostMallocMapped));
        std::memset(s.h_cyc[i], 0, sizeof(Ctl));
        KS_CHECK(hipHostGetDevicePointer((void**)&s.d_cyc[i], s.h_cyc[i], 0));
    }
    KS_CHECK(s.ctl.ensure(1));
    KS_CHECK(s.ctr.ensure(CTR_SHARDS * NCTR));
    KS_CHECK(s.xl.ensure(AUG_KMAX));
    KS_CHECK(s.xl2.ensure(AUG_K2));
    KS_CHECK(s.bx.ensure(BX_CAP));
    KS_CHECK(s.fdef.ensure(FDEF_CAP));
    KS_CHECK(s.sctl.ensure(1));
    KS_CHECK(hipMemset(s.sctl.p, 0, sizeof(StoreCtl)));
    KS_CHECK(hipHostMalloc(&s.h_ctl, sizeof(Ctl)));
    KS_CHECK(hipHostMalloc(&s.h_sctl, sizeof(StoreCtl)));
    std::memset(s.h_sctl, 0, sizeof(StoreCtl));
    return KS_OK;
}

void Engine::set_cells(const int64_t* off, size_t k) {
    EngineImpl& s = *p_;
    std::vector<int64_t> v;
    if (off && k) v.assign(off, off + k + 1);
    if (v != s.cell_off) {
        s.cell_off.swap(v);
        s.cell_first_valid = false;               // the dirty flags belong to the old partition
        s.cells_kept = false;
        if (s.cell_layout) s.csr_valid = false;   // the cells are laid out anew by the next build
    }
}

// A PU's segment must hold the running arcs of the tasks a round pins to it: up to the
// capacity of its arc into the sink, which its degree at the load (two arcs) does not
// show. The build takes the larger of its own estimate and this hint (k_capacity).
__global__ void k_hint_pu_slots(int hi, const unsigned char* __restrict__ alive, const int* __restrict__ src,
                                const int* __restrict__ dst, const long long* __restrict__ cap,
                                const unsigned char* __restrict__ type, int* __restrict__ hint) {
    for (long long a = blockIdx.x * (long long)BLK + threadIdx.x; a < hi; a += (long long)gridDim.x * BLK)
        if (alive[a] && type[src[a]] == KS_NODE_PU && type[dst[a]] == KS_NODE_SINK)
            hint[src[a]] = (int)(cap[a] < 4092 ? cap[a] : 4092) + 4;
}

int Engine::expect_deltas(int64_t nslots, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    if (int rc = ensure_nodes(s, std::max<int64_t>(nslots, 1), err)) return rc;
    s.nslots = std::max(s.nslots, nslots);
    s.incremental = true;
    s.csr_valid = false;
    if (const int hi = s.hi()) {
        hipLaunchKernelGGL(k_hint_pu_slots, dim3(grid_for(hi)), dim3(BLK), 0, s.stream, hi,
                           (const unsigned char*)s.a_alive.p, (const int*)s.a_src.p, (const int*)s.a_dst.p,
                           (const long long*)s.a_cap.p, (const unsigned char*)s.n_type.p, s.n_hint.p);
        KS_CHECK(hipGetLastError());
    }
    return KS_OK;
}

// The cell solver runs when every cell (the ks_batch partition, else the whole
// graph) fits one workgroup's LDS and ks_opts.cell_nodes allows it. Sizes are node
// slots as the build lays them out (the current build's, or the next one's). By
// default a lone graph takes it only up to kCellSingleNodes: one workgroup is one
// CU's VALU, and above that size the multi-kernel engine over the whole chip solves
// a single graph sooner (config 2: ~21 ms vs ~37 ms); a partition's cells run side
// by side on separate CUs, so they take it up to the LDS limit.
constexpr int64_t kCellSingleNodes = 4096;
static bool want_cells(const EngineImpl& s) {
    if (s.opts.cell_nodes < 0 || s.cell_refused || s.fb_active) return false;
    int64_t lim = std::min<int64_t>(cell_max_nodes(s.lds_limit), s.opts.cell_nodes > 0 ? s.opts.cell_nodes : INT32_MAX);
    if (s.opts.cell_nodes == 0 && s.cell_off.size() < 2) lim = std::min(lim, kCellSingleNodes);
    const int64_t ncap =
        s.csr_valid ? s.ncap : s.nslots + (s.incremental ? std::max<int64_t>(64, s.nslots / 16) : 0);
    if (ncap <= 0) return false;
    // a partition's last cell ends where the partition does: the spare slots the store
    // keeps past it once deltas arrive (max(64, nslots/16), tens of thousands on a config-5
    // union) belong to no cell and must not push the union off the cell solver
    const bool part = s.cell_off.size() >= 2;
    const size_t k = part ? s.cell_off.size() - 1 : 1;
    int64_t prev = 0;
    for (size_t i = 1; i <= k; ++i) {
        const int64_t b = i == k && !part ? ncap : std::min<int64_t>(ncap, std::max<int64_t>(prev, s.cell_off[i]));
        if (b - prev > lim) return false;
        prev = b;
    }
    return true;
}

// ================================================================== solve ===
namespace {

// One Bellman-Ford round of kind PR (0: global update; 1: price refinement; 2:
// refinement with parents, the cycle-cancelling finish) in the solve's record layout.
template <int PR>
void launch_bf_round(bool cpv, int grid, hipStream_t st, const DG& g, int seq, int dense) {
    if (cpv) k_bf_round<PR, true><<<dim3(grid), dim3(BLK), 0, st>>>(g, seq, dense);
    else k_bf_round<PR, false><<<dim3(grid), dim3(BLK), 0, st>>>(g, seq, dense);
}

// One solve from the state in place, on the stack of Engine::solve. run() is the
// order of events; the members are what its steps share, by kind: the plan (fixed
// once plan() has run), the tally (what ends in ks_result) and the running state.
struct SolveRun {
    // the engine must take the solve over from the cell solver (Engine::solve runs again)
    enum Retry { RETRY_NONE, RETRY_RANGE, RETRY_CELLS };
    enum { CYCLE_NEXT = 0, PHASE_OVER = 1 };   // what a cycle tells its phase (< 0: an error)

    EngineImpl& s;
    ks_result& res;
    std::string& err;
    const ks_opts& o;
    const hipStream_t st;
    const std::chrono::steady_clock::time_point t_host0 = std::chrono::steady_clock::now();
    // a per-cell fallback carries the cell solver's state (the cells that converged
    // keep their optima; the failing ones restart cold, k_fb_reset)
    const bool fb;
    const bool use_warm;
    Retry retry = RETRY_NONE;
    bool run_all = true;         // every cell runs (prepare(): which cells run)
    std::vector<int> run_list;   //   else these, ascending
    int cells_run = 0;           // cells the cell solver launched

    // ---- the graph as prepare() leaves it
    int hi = 0, nn = 0, ncells = 0;
    int64_t m2 = 0;
    long long mult = 1, maxc = 0;
    bool cpv = false;   // the hot kernels read the 16-B compact positions
    DG g{};

    // ---- plan: derived once from ks_opts and the graph's size (plan(); eps_start: warm_start())
    int alpha = 8, gi_base = 24, gi_tail = 4, pr_cap = 160, prc_cap = 4096, kb_margin = 6, kb_min = 8;
    long long pr_div = 32;   // certify at ε = 1 once ε·pr_div < one (scaled) cost unit
    int phase_exit = 256, phase_frac = 128, aug_slack = 4, walk_passes = 1, fwd_k = 64;
    bool use_pr = false, use_prc = false, use_fwd = false, use_aug = false, cycle_log = false;
    int cyc_lg = CYC_LOG;    // doubling steps of the finish's full searches (both solvers)
    int nhit = 0;
    int fgrid = 0, dgrid = 0, sgrid = 0, wgrid = 0, ngrid = 0, fsgrid = 0, vgrid = 0;
    long long eps_start = 1;   // ε before the first phase's division by α

    // ---- tally: what ends in ks_result
    uint64_t sweeps = 0, gus = 0, sweep_launches = 0, bf_launches = 0, sweep_kernels = 0, early_exits = 0;
    uint64_t fwd_updates = 0, fs_launches = 0;
    double ms_bf_k = 0, ms_sw_k = 0, ms_fs_k = 0;   // event-timed spans: BF rounds / sweeps / forward rounds
    double ms_sat = 0, ms_cycles = 0, ms_pr = 0, ms_cell = 0;
    int phases = 0;
    int prc_cycles = 0, prc_searches = 0;
    long long prc_rejected = 0;   // nodes / leader walks the searches' union-of-cycles test rejected
    unsigned long long cell_ctr[5] = {0, 0, 0, 0, 0};   // scans, visits, pushes, relabels, gu scans
    unsigned long long cell_rounds = 0, cticks_max = 0, cticks_sum = 0;
    long long tot_cost = 0, tot_flow = 0;
    bool launch_refused = false;   // RETRY_RANGE because the device refused the cell launch, not for a value
    bool cost_range = false, cost_wide = false;   // verify(): Σ |flow·cost| ≥ 2^63 / beyond what the kernel could add
    double cost_mag = 0;
    unsigned long long gu_prev = 0;   // cycle log: Bellman-Ford relaxations counted so far

    // ---- running state
    long long eps = 1;
    int kb = 24;                        // Bellman-Ford rounds enqueued per cycle (adaptive)
    int kf = 16;                        // forward rounds enqueued per cycle (adaptive)
    int sseq = 0, bseq = 0;             // frontier buffer sequences
    bool cp_dirty = false;              // the compact residuals hold changes Pos does not have yet
    int status = KS_OK;
    bool pr_failed = false;             // the last phase's refinement did not certify the flow
    bool prc_tried = false;
    long long solve_units = -1;         // excess units at the solve's first update (cold: the supply)
    long long warm_thr = 0;

    // the running phase (run_phase; its two kinds of cycle read and steer it)
    struct Phase {
        long long eps = 1;
        int wsl = 1;              // the tail walks' slack
        bool early = false;       // may end with a few excess nodes left
        int* prc_early = nullptr;
        uint64_t sweeps = 0;
        int gi = 0;               // sweeps in the next cycle (fewer in a phase's tail, where walks augment)
        int peak = 0;             // most excess nodes seen by an update of this phase
        int list = 0;             // the next update lists its excess nodes for the bound (the last apply found ≤ BX_CAP)
        int fwd = 0;              // the next cycle is a forward tail update (≤ fwd_k excess nodes left)
        int fwd_block = 0;        // a forward cycle failed or moved nothing: the next one is a backward update
        int fwd_budget = 64;      // rounds a forward search may take: twice the last global update's
        bool first_upd = true;
        int nupd = 1;             // forward updates per cycle (FWD_UPD once a search finished within its rounds)
        int completed0 = 0;       // fs_completed at the phase's start of forward cycles
        int cur = 0;              // the cycle's slot (control snapshot, events)
        int bf_pend = -1;         // a cycle whose Bellman-Ford event span is not read yet
        int rc = KS_OK;
    } ph;

    // the running finish (finish; search, enqueue_batch and batch_time share it)
    struct Finish {
        int2 *JMa, *JMb;          // jump words, double-buffered (8-B aligned)
        int *J0, *onc, *R, *gbad;
        int* indeg;               // members of its group pointing at a node
        long long *gsum, *gcap;
        bool lds_search;          // the whole search in one workgroup's LDS (k_cyc_lds)
        int nsearch, cap, used;
        int nb;                   // batches enqueued
        unsigned long long srch_seen;
    } fin{};

    SolveRun(EngineImpl& s_, ks_result& res_, std::string& err_, bool warm)
        : s(s_), res(res_), err(err_), o(s_.opts), st(s_.stream), fb(s_.fb_active),
          use_warm((warm && s_.has_prev) || s_.fb_active) {}

    double wall_s() const {
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_host0).count();
    }

    // A cold engine solve reads top to bottom: prepare, plan, phase_loop (run_phase, the
    // finish), certify (verify, recover), report. A cell solve takes cell_solve instead of
    // phase_loop; when it sets `retry`, Engine::solve runs the engine over the same graph.
    int run() {
        int rc = prepare();
        if (rc || nn == 0) return rc;
        plan();
        if ((rc = warm_start())) return rc;
        rc = s.cell_layout ? cell_solve() : phase_loop();
        if (rc || retry != RETRY_NONE) return rc;
        if (cycle_log)
            std::fprintf(stderr, "solve phases %d updates %llu (forward %llu) early phase ends %llu\n", phases,
                         (unsigned long long)gus, (unsigned long long)fwd_updates, (unsigned long long)early_exits);
        if (status == KS_E_INFEASIBLE && !s.cell_layout)
            err = "infeasible: some supply cannot reach a demand node (code " + std::to_string(s.h_ctl->infeasible) +
                  ", phase " + std::to_string(phases) + ", eps " + std::to_string(eps) + ", updates " +
                  std::to_string(gus) + ", sweeps " + std::to_string(sweep_launches) + ")";
        KS_CHECK(hipEventRecord(s.ev[5], st));
        if (status == KS_OK && (rc = certify())) return rc;
        return report();
    }

    // ------------------------------------------------- build / reset ---
    // The CSR persists between solves; it is rebuilt from the arc table only when
    // an in-place delta did not fit (or after a load). A cold solve resets the
    // residual state; a warm one keeps it (carried across a rebuild by slot).
    int prepare() {
        s.solved = false;
        {   // the cell solver's node order, or the multi-kernel engine's (a change rebuilds the CSR)
            const bool cells_now = want_cells(s);
            if (cells_now != s.cell_layout) {
                s.cell_layout = cells_now;
                s.csr_valid = false;
            }
        }
        // Which cells run: a warm solve of a partition whose last solve ended
        // on the cell path, with the residual state still in place (no build since, none
        // now, no fallback running), launches only the cells a record touched since.
        // Anything else runs every cell: skipping is only an optimisation.
        run_all = !(s.cell_off.size() >= 2 && o.warm_start >= 1 && use_warm && !fb && s.cells_kept && s.csr_valid &&
                    s.cell_layout);
        s.cells_kept = false;   // (until this solve ends well: report())
        run_list.clear();
        res.warm_started = use_warm ? 1 : 0;
        res.rebuilt = s.csr_valid ? 0 : 1;
        res.recoveries = 0;
        res.cell_fallbacks = 0;
        res.cycles_cancelled = 0;
        res.fb_resets = 0;
        res.cycles_rejected = 0;
        KS_CHECK(hipEventRecord(s.ev[0], st));
        KS_CHECK(hipMemsetAsync(s.ctr.p, 0, CTR_SHARDS * NCTR * sizeof(unsigned long long), st));
        KS_CHECK(hipMemsetAsync(s.ctl.p, 0, sizeof(Ctl), st));
        std::memset(s.h_ctl, 0, sizeof(Ctl));
        if (!s.csr_valid) {
            if (int rc = rebuild()) return rc;
        } else if (!use_warm) {
            if (int rc = cold_reset(s, err)) return rc;
        }
        hi = s.hi();
        nn = s.nn;
        m2 = s.m2cap;
        mult = s.mult;
        ncells = (int)s.h_cells.size();
        res.n_nodes = s.nslots;
        res.n_arcs = s.h_sctl->live;
        if (nn == 0) {
            res.total_cost = 0;
            res.flow_value = 0;   // no nodes: nothing flows
            s.solved = true;
            s.has_prev = true;
            return KS_OK;
        }
        // max |cost| → the first phase's ε
        if (hi)
            hipLaunchKernelGGL(k_max_cost, dim3(grid_for(hi, 512)), dim3(BLK), 0, st, hi,
                               (const unsigned char*)s.a_alive.p, (const long long*)s.a_cost.p, &s.ctl.p->gu_L);
        // the engine's hot kernels read 16-B copies of the positions when every value
        // fits; the range flag comes back with the control block below
        const bool want_cp = !s.cell_layout && s.opts.compact_pos >= 0 && m2 > 0;
        if (want_cp) {
            KS_CHECK(s.cpos.ensure(m2));
            KS_CHECK(s.crev.ensure(m2));
            hipLaunchKernelGGL(k_pack_pos, dim3(grid_for(m2, 4096)), dim3(BLK), 0, st, (long long)m2,
                               (const Pos*)s.pos.p, s.cpos.p, s.crev.p, &s.ctl.p->cp_bad);
        }
        // the cells' dirty flags come back with the control block (no sync of their own);
        // a partition no stream has marked yet has none set
        const bool flags = !run_all && s.cell_first_valid;
        if (flags) {
            s.h_cell_dirty.assign(ncells, 1);
            KS_CHECK(hipMemcpyAsync(s.h_cell_dirty.data(), s.cell_dirty.p, ncells * sizeof(int), hipMemcpyDeviceToHost,
                                    st));
        }
        KS_CHECK(read_ctl());
        if (flags)
            for (int c = 0; c < ncells; ++c)
                if (s.h_cell_dirty[c]) run_list.push_back(c);
        maxc = s.h_ctl->gu_L;
        cpv = want_cp && !s.h_ctl->cp_bad;
        cp_dirty = false;
        res.compact = cpv ? 1 : 0;
        KS_CHECK(hipMemsetAsync(&s.ctl.p->gu_L, 0, sizeof(long long), st));
        if (maxc > 0 && (double)maxc * (double)mult * 8.0 * (double)mult > 4.0e18) {
            err = "cost range too large for int64 scaled prices";
            return KS_E_RANGE;
        }
        KS_CHECK(hipEventRecord(s.ev[1], st));
        return KS_OK;
    }

    // The build, with a warm solve's flows and prices carried across it by slot (and
    // the failing cells of a per-cell fallback restarted cold).
    int rebuild() {
        const int64_t ncap_prev = s.ncap;
        const long long mult_prev = s.mult;
        const bool carry = use_warm && s.nn > 0;
        const int hi0 = s.hi();
        if (carry) {
            KS_CHECK(s.saved_flows.ensure(std::max(hi0, 1)));
            KS_CHECK(s.p_slot.ensure(std::max<int64_t>(ncap_prev, 1)));
            if (hi0)
                hipLaunchKernelGGL(k_save_flows, dim3(grid_for(hi0)), dim3(BLK), 0, st, hi0,
                                   (const unsigned char*)s.a_alive.p, (const int*)s.fwd.p, (const Pos*)s.pos.p,
                                   s.saved_flows.p);
            hipLaunchKernelGGL(k_save_prices, dim3(grid_for(ncap_prev)), dim3(BLK), 0, st, (int)ncap_prev,
                               (const int*)s.perm.p, (const long long*)s.nd.p, s.p_slot.p);
            if (fb && !s.fb_cells.empty()) {
                std::vector<long long> rng;
                const size_t kc = s.cell_off.size() >= 2 ? s.cell_off.size() - 1 : 1;
                for (int c : s.fb_cells) {
                    rng.push_back(kc > 1 ? s.cell_off[c] : 0);
                    rng.push_back(kc > 1 ? s.cell_off[c + 1] : ncap_prev);
                }
                KS_CHECK(s.fb_rng.ensure(rng.size()));
                KS_CHECK(hipMemcpyAsync(s.fb_rng.p, rng.data(), rng.size() * sizeof(long long), hipMemcpyHostToDevice,
                                        st));
                const int n = (int)std::max<int64_t>(hi0, ncap_prev);
                KS_CHECK(s.fb_cnt.ensure(1));
                KS_CHECK(hipMemsetAsync(s.fb_cnt.p, 0, sizeof(unsigned long long), st));
                hipLaunchKernelGGL(k_fb_reset, dim3(grid_for(std::max(n, 1))), dim3(BLK), 0, st, hi0, (int)ncap_prev,
                                   (int)(rng.size() / 2), (const long long*)s.fb_rng.p, (const int*)s.a_src.p,
                                   (const unsigned char*)s.a_alive.p, s.saved_flows.p, s.p_slot.p, s.fb_cnt.p);
                unsigned long long nres = 0;
                KS_CHECK(hipMemcpyAsync(&nres, s.fb_cnt.p, sizeof(nres), hipMemcpyDeviceToHost, st));
                KS_CHECK(hipStreamSynchronize(st));   // (rng is a host vector)
                res.fb_resets = nres;
            }
        }
        int rc = build(s, err);
        if (rc) return rc;
        rc = cold_reset(s, err);
        if (rc) return rc;
        if (carry) {
            if (hi0)
                hipLaunchKernelGGL(k_restore_flows, dim3(grid_for(hi0)), dim3(BLK), 0, st, hi0,
                                   (const unsigned char*)s.a_alive.p, (const long long*)s.saved_flows.p,
                                   (const long long*)s.a_low.p, (const long long*)s.a_cap.p, (const int*)s.fwd.p,
                                   (const int*)s.a_src.p, (const int*)s.a_dst.p, (const int*)s.perm.p, s.pos.p,
                                   s.excess.p);
            hipLaunchKernelGGL(k_restore_prices, dim3(grid_for(s.ncap)), dim3(BLK), 0, st, (int)s.ncap,
                               (int)ncap_prev, mult_prev, s.mult, (const long long*)s.p_slot.p, (const int*)s.perm.p,
                               s.nd.p, (s.nd.p + 2));
        }
        return KS_OK;
    }

    // -------------------------------------------------------------- plan ---
    // Tuning comes from ks_opts only (0 = default; include/ksmcmf.h): nothing in
    // the environment changes the algorithm.
    void plan() {
        g = s.dg();
        g.cp = cpv ? s.cpos.p : nullptr;
        g.crev = cpv ? s.crev.p : nullptr;
        // hops per Bellman-Ford launch (ks_opts.two_hop): 0 one, 1 two (through tasks and
        // PUs), 2 four (the workgroup's continuation queue; 3: TESTS ONLY, fault_inject
        // bit 9, a 2-entry queue). Default: DESIGN §3.
        {
            const int hops = o.two_hop < 0 ? 0 : (o.two_hop == 0 ? TWO_HOP_DEFAULT : std::min(2, (int)o.two_hop));
            g.expand = (hops == 2 && (o.fault_inject & 512)) ? 3 : hops;
        }
        g.bound = o.bf_bound < 0 ? 0 : 1;      // tail updates bounded at the excess nodes' distances
        g.fs_wide = std::max(2048, nn / 4);   // (measured: config 4's searches ≤ nn/6 wide, config 3's hub-bound ones ~nn/4 to 3nn/4)
        g.aug_k = o.tail_nodes > 0 ? std::min(AUG_KMAX, (int)o.tail_nodes) : 64;
        fgrid = s.window_grid();     // dense passes over every window (saturate)
        dgrid = s.dense_grid();      // dense Bellman-Ford round
        sgrid = s.sparse_grid();     // sparse Bellman-Ford rounds
        wgrid = s.sweep_grid();      // sweeps
        ngrid = grid_for(nn, 2048);
        fsgrid = s.nhitems * HSPLIT + FS_LIST_BLOCKS;   // forward tail rounds
        vgrid = grid_for(hi, VERIFY_GRID);  // verification
        // forward tail updates once ≤ fwd_k nodes hold excess (ks_opts.fwd_nodes; the
        // search key packs an arc position into FS_PB bits)
        use_fwd = o.fwd_nodes >= 0 && s.m2cap < FS_NONE;
        // (default by size: config 2's 12k-node searches widen sooner; interleaved A/B,
        // config 2 28.0 / 26.4 → 25.5 / 25.0 ms at 32, config 4 slower at 32 than at 64)
        fwd_k = o.fwd_nodes > 0 ? (int)o.fwd_nodes : (nn < 32768 ? 32 : 64);
        // α by size: with the cycle-cancelling finish a small engine graph is best with
        // one coarse phase and the finish (12 config-2 graphs, median / max ms: α 8 14.6 /
        // 17.9, 16 14.9 / 16.5, 32 11.6 / 15.4, 48 12.6 / 15.9, 1024 — a single phase at
        // the final ε — 13.4 / 24.4); config 3 and the config-4 rounds are slower at 16
        // and 32, and the cell solver's ladder stays at 8 (config 5 36 ms at 32) — DESIGN §3
        // (the small-graph α and the D below were tuned for the finish: they follow use_prc,
        // so a graph whose positions do not fit the packed keys keeps the plain schedule)
        use_pr = o.price_refine != 0;
        use_prc = use_pr && o.price_refine == 1 && !s.cell_layout && s.m2cap < PK_NONE;
        alpha = o.alpha >= 2 ? o.alpha : (!s.cell_layout && nn < 32768 && use_prc) ? 32 : 8;
        gi_base = o.gu_interval > 0 ? o.gu_interval : 24;
        gi_base = std::max(2, std::min(MAXB, gi_base)) & ~1;     // even: sweeps end on p0
        pr_cap = o.pr_rounds > 0 ? o.pr_rounds : 160;  // price-refinement rounds before giving up
        cycle_log = o.log_cycles != 0;
        nhit = s.nhitems;
        use_aug = o.walk_slack >= 0;               // tail augmentation (walks)
        aug_slack = o.walk_slack > 0 ? o.walk_slack : 4;   // walks take arcs of rc <= slack·ε
        walk_passes = o.walk_passes > 0 ? std::min(8, (int)o.walk_passes) : 1;
        // Bellman-Ford rounds enqueued per cycle: the last update's count + kb_margin,
        // at least kb_min (a launch that finds the update converged still costs ≈ 5 µs
        // with the gap before the next kernel; an update that needs more than was
        // enqueued costs a whole extra cycle)
        kb_margin = o.bf_margin > 0 ? o.bf_margin : 6;
        kb_min = 8;
        // the cycle-cancelling finish replaces the final cost-scaling phase (ks_opts.price_refine
        // 1, the default; 2: the final phase and plain refinement, as before round 5)
        // refinement rounds before the final phase takes over (TESTS ONLY, fault_inject bit 5: one batch)
        prc_cap = (o.fault_inject & 32) ? 32 : 4096;
        // (TESTS ONLY, fault_inject bit 7: every search 5 steps, a window shorter than
        // the parent chains — their nodes get marked and run into cycles' groups)
        cyc_lg = (o.fault_inject & 128) ? 5 : CYC_LOG;
        gi_tail = o.tail_sweeps > 0 ? std::max(2, std::min(MAXB, (int)o.tail_sweeps)) & ~1 : 4;
        // A phase that another phase follows may end with a few excess nodes left:
        // refine's start (saturate every negative reduced cost) accepts any
        // pseudoflow, so the next, finer phase absorbs them with its own excess.
        // Only the last phase (the one price refinement may certify, or ε = 1) must
        // end with a feasible flow. A coarse phase ends once at most phase_exit
        // nodes AND at most 1/phase_frac of its peak hold excess (the relative bound
        // keeps phases that start small — incremental rounds — doing their share).
        phase_exit = o.phase_exit < 0 ? 0 : (o.phase_exit > 0 ? o.phase_exit : 256);
        phase_frac = o.phase_frac > 0 ? o.phase_frac : 128;
        // ε schedule: the phase that price refinement certifies runs at 1/D of a cost
        // unit (ks_opts.final_div), the others at α-multiples of it, the first in
        // [max|cost|/α², max|cost|/α) scaled. D = 48 on large graphs. Measured on config 3
        // (40 solves each): ending at 1/32 of a unit (the plain max|cost|/α^k sequence)
        // left the flow short of optimal in 15 of 40 solves — a sixth phase, ≈ 28 ms —
        // at 1/48 in none; 1/64 and 1/96 cost more per phase. D = 20 on small graphs and
        // cells (under 32,768 nodes; every cell is): their flow is usually optimal a
        // phase earlier (config 2 26–27 → 20–21 ms, config 5 53–54 → 41–43 ms).
        // Round 5: with the cycle-cancelling finish the final phase no longer runs, and
        // D only places the ladder; large graphs take D = 24 — one coarse phase fewer
        // (config 3: 35.4–36.9 vs 36.6–38.6 ms in interleaved pairs).
        eps = std::max<long long>(1, maxc * mult);
        {
            const long long D = o.final_div < 0 ? 0
                                : o.final_div > 0 ? o.final_div
                                : (s.cell_layout || nn < 32768) ? 20 : (use_prc ? 24 : 48);
            if (D > 0 && use_pr && maxc > 0) {
                long long e = std::max<long long>(1, (mult - 1) / D);
                // the cell solver's ladder is powers of two (α = 8): its arc lengths
                // floor(rc/ε) are then shifts (the final phase lands in (1/2D, 1/D] of a unit)
                if (s.cell_layout && (alpha & (alpha - 1)) == 0)
                    while (e & (e - 1)) e &= e - 1;
                const long long lo = std::max<long long>(1, eps / ((long long)alpha * alpha));
                while (e < lo && e <= (1LL << 58) / alpha) e *= alpha;
                eps = e * alpha;   // the loop divides before each phase
                pr_div = D;
            }
        }
        eps_start = eps;
    }

    // warm start: the previous flow and prices (in place), fresh nodes priced off
    // their out-arcs, then a start at a small ε (≤ 8 cost units) saturating only
    // the arcs that violate it
    int warm_start() {
        if (!use_warm || fb) return KS_OK;
        if (o.warm_shift >= 0)
            hipLaunchKernelGGL(k_price_shift, dim3(grid_for(s.ncap, 2048)), dim3(BLK), 0, st, (int)s.ncap,
                               (const unsigned long long*)s.n_cshift.p, (const int*)s.perm.p, mult, s.nd.p);
        hipLaunchKernelGGL(k_fresh_prices, dim3(grid_for(s.ncap, 2048)), dim3(BLK), 0, st, (int)s.ncap,
                           (const unsigned char*)s.n_fresh.p, (const int*)s.perm.p, g);
        if (m2) hipLaunchKernelGGL(k_max_viol, dim3(grid_for(m2, 2048)), dim3(BLK), 0, st, g, (long long)m2);
        KS_CHECK(read_ctl());
        const long long viol = s.h_ctl->gu_L;
        constexpr long long kWarmUnits = 8;   // the first warm phase at ≤ 8 cost units
        long long e0 = std::max<long long>(1, std::min<long long>({viol, kWarmUnits * mult, eps}));
        if (s.cell_layout && (alpha & (alpha - 1)) == 0)   // a power of two ≥ the violation (cell ladder)
            while (e0 & (e0 - 1)) e0 += e0 & -e0;
        warm_thr = e0;
        eps = e0 * alpha;   // the first phase runs at e0
        eps_start = eps;
        KS_CHECK(hipMemsetAsync(&s.ctl.p->gu_L, 0, sizeof(long long), st));
        if (cycle_log) {   // diagnostics: the carried prices' span (in cost units) and the start
            std::vector<long long> h((size_t)4 * nn);
            KS_CHECK(hipMemcpyAsync(h.data(), s.nd.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
            KS_CHECK(hipStreamSynchronize(st));
            long long lo = INF64, hi2 = -INF64;
            for (int v = 0; v < nn; ++v) {
                lo = std::min(lo, h[(size_t)4 * v]);
                hi2 = std::max(hi2, h[(size_t)4 * v]);
            }
            std::fprintf(stderr, "warm start: largest violation %.3f units, first phase at %.3f units, price span %.1f units\n",
                         (double)viol / mult, (double)e0 / mult, (double)(hi2 - lo) / mult);
        }
        return KS_OK;
    }

    // -------------------------------------------------------- primitives ---
    hipError_t read_ctl() {
        hipError_t e = hipMemcpyAsync(s.h_ctl, s.ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(st);
    }
    // ε (and, by flags, the control words a phase or the finish starts from) set by a
    // one-thread kernel: a host-to-device copy is a copy kernel behind a staging gap,
    // and each memset another launch
    hipError_t set_eps(long long e, int flags = 0) {
        hipLaunchKernelGGL(k_set_eps, dim3(1), dim3(1), 0, st, g, e, 1.0 / (double)e, flags);
        return hipGetLastError();
    }
    // One Bellman-Ford round on the next frontier buffer.
    // mode 0: global update; 1: price refinement; 2: refinement with parents (cycle cancelling)
    void bf_round(int mode, bool dense) {
        const int grid = dense ? dgrid : sgrid;
        if (mode == 2) launch_bf_round<2>(cpv, grid, st, g, bseq, dense ? 1 : 0);
        else if (mode) launch_bf_round<1>(cpv, grid, st, g, bseq, dense ? 1 : 0);
        else launch_bf_round<0>(cpv, grid, st, g, bseq, dense ? 1 : 0);
        ++bseq;
        ++bf_launches;
    }
    void bf_rounds(int mode, int k, bool first_dense) {
        for (int r = 0; r < k; ++r) bf_round(mode, first_dense && r == 0);
    }
    // the compact solve's residuals back into the 32-B records (Pos is the authoritative copy)
    void sync_pos() {
        if (!cp_dirty) return;
        hipLaunchKernelGGL(k_unpack_pos, dim3(grid_for(m2, 4096)), dim3(BLK), 0, st, (long long)m2,
                           (const CPos*)s.cpos.p, s.pos.p);
        cp_dirty = false;
    }
    // (diagnostics, ks_opts.log_cycles) Bellman-Ford relaxations since the last call,
    // from the sharded counters
    int relaxations(unsigned long long* since) {
        std::vector<unsigned long long> hctr((size_t)CTR_SHARDS * NCTR);
        KS_CHECK(hipMemcpy(hctr.data(), s.ctr.p, hctr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long gsc = 0;
        for (int i = 0; i < CTR_SHARDS; ++i) gsc += hctr[(size_t)i * NCTR + C_GUSCAN];
        *since = gsc - gu_prev;
        gu_prev = gsc;
        return KS_OK;
    }

    // ------------------------------------------------------------ phases ---
    // The "last phase" of the ladder: the one price refinement may certify, or ε = 1.
    bool is_last(long long e) const { return e / alpha < 1 || e <= 1 || (use_pr && e * pr_div < mult); }

    // The ε ladder of the multi-kernel engine.
    int phase_loop() {
        do {
            eps = std::max<long long>(1, eps / alpha);
            ++phases;
            // After a failed refinement the flow is feasible and ε-optimal at the old ε:
            // saturating only the arcs that violate the new ε (rc < −ε) is a valid start
            // (push-relabel at ε needs an ε-optimal pseudoflow, not a 0-optimal one) and
            // disturbs far less than saturating every negative arc.
            // warm_start 2: every phase of a warm solve saturates only the arcs that
            // violate its ε (the previous optimum's arcs in [−1, 0) stay as they are)
            // per-cell fallback: the cold ε ladder, every phase saturating only the arcs
            // that violate its ε (the converged cells' optimal flows stay untouched)
            long long sat_thr = phases == 1 && use_warm && !fb
                                    ? warm_thr
                                    : ((pr_failed || fb || (use_warm && o.warm_start >= 2)) ? eps : 0LL);
            pr_failed = false;
            const bool last_phase = is_last(eps);
            // the phase before the final one drains completely when the cycle-cancelling
            // finish replaces the final phase
            const long long eps_next = std::max<long long>(1, eps / alpha);
            const bool before_last = !last_phase && !prc_tried && is_last(eps_next);
            const bool prc_now = use_prc && before_last;
            // two phases before the last: the finish may follow this phase instead
            // (run_phase prc_early) when the flow is already close to optimal
            const long long eps_next2 = std::max<long long>(1, eps_next / alpha);
            const bool before_last2 = !last_phase && !before_last && is_last(eps_next2);
            // walk slack > 1 only while a finer phase or price refinement still follows
            // (ε > 1): a phase at ε = 1 must end 1-optimal (fault_inject bit 0 breaks
            // exactly this, for the certificate-recovery test)
            const int walk_sl = (eps > 1 || (o.fault_inject & 1)) ? aug_slack : 1;
            int prc_early = 0;
            // (only from a phase at most two cost units coarse: earlier, the finish has
            // too many cycles to cancel — config 4 with D = 24 at 2.6 units: 26 vs 20 ms)
            const bool may_early = use_prc && !prc_tried && before_last2 && !use_warm && !fb && eps <= 2 * mult;
            const int rc = run_phase(eps, sat_thr, !last_phase && !prc_now, walk_sl, may_early ? &prc_early : nullptr);
            if (rc == KS_E_INFEASIBLE) {
                status = rc;
                break;
            }
            if (rc) return rc;
            if (prc_now || prc_early) {   // the feasible flow of the last coarse phase: cancel its negative cycles
                prc_tried = true;
                int used = 0;
                const int pr = finish(&used, prc_early ? std::min(prc_cap, 1024) : prc_cap);
                if (pr < 0) return pr;
                if (pr == 1) {
                    eps = 1;
                    break;
                }
                pr_failed = true;   // the final phase follows, saturating only its violations
                continue;
            }
            // certify optimality early: a flow that is 1-optimal (scaled) is optimal.
            // Tried once ε is below 1/32 of a cost unit, where it usually succeeds.
            if (use_pr && eps > 1 && eps * pr_div < mult) {
                int used = 0;
                const int pr = price_refine(1, &used, pr_cap);
                if (pr < 0) return pr;
                if (pr == 1) eps = 1;
                else pr_failed = true;
            }
        } while (eps > 1);
        return KS_OK;
    }

    // One ε-phase from the pseudoflow in place: saturate every residual arc whose
    // reduced cost is below −sat_thr (thr 0: Goldberg's refine start; thr ε: only
    // the arcs that violate ε-optimality), then update/sweep cycles until no node
    // holds excess — a coarse phase (may_end_early) may stop with a few excess
    // nodes left for the next, finer one. walk_sl: the tail walks' slack (1 when the
    // phase must end ε-optimal at ε = 1). Returns KS_OK, KS_E_INFEASIBLE (status),
    // or a device / convergence error.
    // prc_early: when non-null, the phase may turn itself into the one the cycle-
    // cancelling finish follows (*prc_early = 1, the phase then drains): at its first
    // update, if at most 1/KS_PRC_UNITS_DIV of the solve's first-update units hold
    // excess — the flow is already close to optimal (config 4's churn
    // rounds, 0.07–0.11 of the supply, vs ≥ 1.9 for cold configs 2 and 3)
    int run_phase(long long eps_ph, long long sat_thr, bool may_end_early, int walk_sl, int* prc_early = nullptr) {
        KS_CHECK(hipEventRecord(s.ev[2], st));
        KS_CHECK(set_eps(eps_ph, use_fwd ? SET_FWD : 0));   // a phase never continues another phase's forward search
        KS_HOT(cpv, k_saturate, fgrid, BLK, st, g, sat_thr);
        cp_dirty = cpv;
        KS_CHECK(hipEventRecord(s.ev[3], st));
        ph = Phase{};
        ph.eps = eps_ph;
        ph.wsl = walk_sl;
        ph.early = may_end_early;
        ph.prc_early = prc_early;
        ph.gi = gi_base;
        // Cycles run one at a time (enqueueing the next one before reading this
        // one's control block was measured slower: the speculative launches cost
        // more GPU time than the host's decision gap).
        for (;;) {
            const int r = ph.fwd ? fwd_cycle() : bwd_cycle();
            if (r < 0) return r;
            if (r == PHASE_OVER) break;
        }
        flush_bf();
        KS_CHECK(hipEventRecord(s.ev[4], st));
        KS_CHECK(hipEventSynchronize(s.ev[4]));
        ms_sat += ev_ms(s.ev[2], s.ev[3]);
        ms_cycles += ev_ms(s.ev[3], s.ev[4]);
        return ph.rc;
    }

    // Forward cycle: nupd × [init (or continue the pending search)][kf rounds][apply]
    // [trace][end], then the cycle end; no sweeps (the trace routes the units). An
    // update whose search has not converged when the next one starts is continued
    // by it. fev brackets each update's search rounds (the forward kind's time).
    hipError_t enqueue_fwd(int par, int nupd) {
        hipError_t e = hipSuccess;
        for (int u = 0; u < nupd; ++u) {
            hipLaunchKernelGGL(k_fs_init, dim3(ngrid), dim3(BLK), 0, st, g, bseq);
            if ((e = hipEventRecord(s.fev[par][2 * u], st)) != hipSuccess) return e;
            for (int r = 0; r < kf; ++r) {
                KS_HOT(cpv, k_fs_round, fsgrid, BLK, st, g, bseq);
                ++bseq;
                ++fs_launches;
            }
            if ((e = hipEventRecord(s.fev[par][2 * u + 1], st)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_fs_apply, dim3(ngrid), dim3(BLK), 0, st, g);
            KS_HOT(cpv, k_fs_trace, FDEF_CAP, WAVE, st, g);
            hipLaunchKernelGGL(k_fs_end, dim3(1), dim3(WAVE), 0, st, g);
        }
        hipLaunchKernelGGL(k_cycle_end, dim3(1), dim3(128), 0, st, g, s.d_cyc[par], 1);
        return hipEventRecord(s.cdone[par], st);
    }
    int fwd_cycle() {
        KS_CHECK(enqueue_fwd(ph.cur, ph.nupd));
        KS_CHECK(hipEventSynchronize(s.cdone[ph.cur]));
        const Ctl* hc = s.h_cyc[ph.cur];
        double t_fs = 0;
        for (int u = 0; u < ph.nupd; ++u) t_fs += ev_ms(s.fev[ph.cur][2 * u], s.fev[ph.cur][2 * u + 1]);
        ms_fs_k += t_fs;
        ph.cur ^= 1;
        const bool completed = hc->fs_done || hc->fs_fail;
        if (cycle_log)
            std::fprintf(stderr, "fwd cycle phase %d eps %lld updates %d rounds %d fs_ms %.3f units %lld n_exc %d done %d fail %d D %lld deficits %d moved %d width %d\n",
                         phases, ph.eps, ph.nupd, hc->fs_rounds, t_fs, hc->u_exc_rep, hc->n_exc_rep,
                         hc->fs_done, hc->fs_fail, hc->fs_D < FS_DMAX ? hc->fs_D : -1LL, hc->n_fdef,
                         hc->fs_moved_cyc, hc->fs_maxcnt);
        if (completed && hc->n_exc_rep == 0) return PHASE_OVER;   // no excess left: the phase is done
        const int done_now = hc->fs_completed - ph.completed0;
        ph.completed0 = hc->fs_completed;
        gus += done_now;
        fwd_updates += done_now;
        bool wide = hc->fs_fail == 2;
        if (!completed && hc->fs_rounds >= ph.fwd_budget) {
            // longer than two global updates: drop it like a wide one
            KS_CHECK(hipMemsetAsync(&s.ctl.p->fs_pending, 0, sizeof(int), st));
            KS_CHECK(hipMemsetAsync(s.ctl.p->fs_cnt, 0, sizeof(s.ctl.p->fs_cnt), st));
            wide = true;
        }
        if (hc->fs_fail || wide) {
            // list overflow, no deficit in range, or a search too wide or too long
            // (a hub's arcs in reach): ONE global update, then forward again
            ph.fwd = 0;
            ph.fwd_block = 1;
            ph.nupd = 1;
            return CYCLE_NEXT;
        }
        if (!completed) {            // the search continues next cycle
            kf = std::min(256, 2 * kf);
            ph.nupd = 1;
            return CYCLE_NEXT;
        }
        kf = std::max(8, std::min(256, hc->fs_rounds + 4));
        ph.nupd = FWD_UPD;
        if (hc->fs_moved_cyc == 0) {
            ph.fwd = 0;
            ph.fwd_block = 1;
        }
        if (wall_s() > kSolveWallLimitS) {
            (void)hipStreamSynchronize(st);
            err = "forward tail did not converge (" + std::to_string(wall_s()) + " s)";
            return KS_E_DEVICE;
        }
        return CYCLE_NEXT;
    }

    // One cycle: [GU init (or continue the pending update)][kb BF rounds][max]
    // [apply][tail walks][gi sweeps][end: control block → pinned host memory].
    // cev[0..1] bracket the Bellman-Ford rounds (the sweeps: device clock).
    hipError_t enqueue_bwd(int par) {   // one cycle into slot par
        const int gi = ph.gi, wsl = ph.wsl;
        hipLaunchKernelGGL(k_gu_init, dim3(ngrid), dim3(BLK), 0, st, g, bseq, ph.list);
        hipError_t e = hipEventRecord(s.cev[par][0], st);
        if (e != hipSuccess) return e;
        for (int r = 0; r < kb; ++r) bf_round(0, false);   // sparse from the first round: k_gu_init flags the deficits
        if ((e = hipEventRecord(s.cev[par][1], st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gu_max, dim3(ngrid), dim3(BLK), 0, st, g);
        hipLaunchKernelGGL(k_gu_apply, dim3(ngrid), dim3(BLK), 0, st, g, sseq);
        if (use_aug) {   // tail: walkers, hub distribution, walkers from what it fed
            KS_HOT(cpv, k_augment, g.aug_k, WAVE, st, g, sseq, 0, wsl);
            if (nhit) KS_HOT(cpv, k_aug_hub, nhit, BLK, st, g, sseq, wsl);
            KS_HOT(cpv, k_augment, AUG_K2, WAVE, st, g, sseq, 1, wsl);
            // further passes retry the units left short at the listed nodes
            for (int wp = 1; wp < walk_passes; ++wp)
                KS_HOT(cpv, k_augment, g.aug_k, WAVE, st, g, sseq, 0, wsl);
        }
        // (the sweeps are timed by the device clock — the first sweep's start to
        // k_cycle_end's — not by HIP events: an event between two kernels costs a
        // ~5.7 µs gap of its own, two per cycle; profiles/r06_*)
        for (int k = 0; k < gi; ++k) KS_HOT(cpv, k_sweep, wgrid, BLK, st, g, k, sseq + k);
        hipLaunchKernelGGL(k_cycle_end, dim3(1), dim3(128), 0, st, g, s.d_cyc[par], 0);
        sseq += gi;
        return hipEventRecord(s.cdone[par], st);
    }
    void flush_bf() {
        if (ph.bf_pend >= 0) ms_bf_k += ev_ms(s.cev[ph.bf_pend][0], s.cev[ph.bf_pend][1]);
        ph.bf_pend = -1;
    }
    int bwd_cycle() {
        const int cur = ph.cur, gi = ph.gi;
        if (ph.bf_pend == cur) flush_bf();   // (the slot's events are about to be recorded again)
        KS_CHECK(enqueue_bwd(cur));
        flush_bf();   // the previous cycle's event time, read while this one runs
        KS_CHECK(hipEventSynchronize(s.cdone[cur]));
        const Ctl* hc = s.h_cyc[cur];
        sweep_kernels += gi;
        double t_bf = 0;
        if (cycle_log) {
            t_bf = ev_ms(s.cev[cur][0], s.cev[cur][1]);
            ms_bf_k += t_bf;   // BF rounds only
        } else {
            ph.bf_pend = cur;  // read after the next cycle is enqueued (off the host's critical path)
        }
        const double t_sw = hc->t_end > hc->t_sw0 ? (double)(hc->t_end - hc->t_sw0) / 1e5 : 0.0;   // 100 MHz ticks
        ms_sw_k += t_sw;   // sweeps only
        if (hc->infeasible) {
            ph.rc = KS_E_INFEASIBLE;
            std::memcpy(s.h_ctl, hc, sizeof(Ctl));
            return PHASE_OVER;
        }
        if (!hc->bf_done) {
            // update still running: its sweeps were skipped and the next cycle continues it
            kb = std::min(256, kb * 2);
            ph.cur ^= 1;
            return CYCLE_NEXT;
        }
        if (cycle_log) {
            // (diagnostics: the update's relaxations, from the sharded counters)
            unsigned long long relax = 0;
            if (int rc = relaxations(&relax)) return rc;
            std::fprintf(stderr, "cycle phase %d eps %lld bf %d relax %llu bf_ms %.3f sw_ms %.3f active %d units %lld n_exc %d walks %d/%d",
                         phases, ph.eps, hc->bf_count - hc->bf_r0, relax, t_bf, t_sw, hc->sweep_act[gi - 1], hc->u_exc, hc->n_exc,
                         hc->aug_reached, hc->aug_short);
            for (int k = 0; k < std::min(4, hc->n_exc); ++k) {
                const int x = hc->dbg_x[k];
                int c = 0;
                while (c < NGC && x >= s.obeg[c + 1]) ++c;
                std::fprintf(stderr, " [x%d c%d e%d]", x, x >= s.hub_base ? 9 : c, hc->dbg_e[k]);
            }
            std::fprintf(stderr, "\n");
        }
        if (ph.first_upd) {
            ph.first_upd = false;
            if (solve_units < 0) solve_units = hc->u_exc;
            if (ph.prc_early && ph.early && hc->u_exc * kPrcUnitsDiv <= solve_units) {
                ph.early = false;
                *ph.prc_early = 1;
            }
        }
        kb = std::max(kb_min, std::min(256, hc->bf_count - hc->bf_r0 + kb_margin));
        ph.fwd_budget = std::max(16, 2 * (hc->bf_count - hc->bf_r0));
        ++gus;
        sweeps += gi;
        sweep_launches += gi;
        ph.sweeps += gi;
        int last = 0;
        for (int k = 0; k < gi; ++k)
            if (hc->sweep_act[k]) last = k + 1;
        if (!hc->sweep_act[gi - 1]) {
            sweeps -= gi - last;
            return PHASE_OVER;   // no excess left: refine done
        }
        ph.peak = std::max(ph.peak, hc->n_exc);
        if (ph.early && hc->n_exc <= phase_exit && (long long)hc->n_exc * phase_frac <= ph.peak) {
            ++early_exits;
            return PHASE_OVER;   // a coarse phase: the next one absorbs the few units left
        }

        ph.gi = (use_aug && hc->n_exc <= g.aug_k) ? gi_tail : gi_base;
        ph.list = g.bound && hc->n_exc > 0 && hc->n_exc <= BX_CAP;
        // forward tail updates only in coarse phases: in the last phase config 3's
        // searches reach the cluster aggregator and widen
        ph.fwd = use_fwd && ph.early && !ph.fwd_block && hc->n_exc > 0 && hc->n_exc <= fwd_k;
        ph.fwd_block = 0;
        if (ph.sweeps > (uint64_t)(64 * ((uint64_t)nn + 64)) || wall_s() > kSolveWallLimitS) {
            (void)hipStreamSynchronize(st);
            err = "push/relabel did not converge (sweeps " + std::to_string(ph.sweeps) + ", " +
                  std::to_string(wall_s()) + " s)";
            return KS_E_DEVICE;
        }
        ph.cur ^= 1;
        return CYCLE_NEXT;
    }

    // Price refinement at eps_try: 1 = success (prices updated), 0 = failed, <0 error.
    int price_refine(long long eps_try, int* rounds_used, int cap, int from_p = 0) {
        KS_CHECK(hipEventRecord(s.ev[5], st));
        KS_CHECK(set_eps(eps_try));
        hipLaunchKernelGGL(k_pr_init, dim3(ngrid), dim3(BLK), 0, st, g, bseq, from_p);
        int used = 0, ok = 0;
        for (int batch = 0; used < cap; ++batch) {
            const int k = std::min(64, cap - used);
            KS_CHECK(hipEventRecord(s.kev[0], st));
            bf_rounds(1, k, batch == 0);
            KS_CHECK(hipEventRecord(s.kev[1], st));
            used += k;
            KS_CHECK(read_ctl());
            ms_bf_k += ev_ms(s.kev[0], s.kev[1]);
            if (s.h_ctl->bf_done) {
                ok = 1;
                break;
            }
        }
        if (ok) hipLaunchKernelGGL(k_pr_apply, dim3(ngrid), dim3(BLK), 0, st, g, 0);
        KS_CHECK(hipEventRecord(s.ev[6], st));
        KS_CHECK(hipEventSynchronize(s.ev[6]));
        ms_pr += ev_ms(s.ev[5], s.ev[6]);
        *rounds_used = used;
        return ok;
    }

    // ------------------------------------------------------------ finish ---
    // The cycle-cancelling finish: refinement rounds that record parents
    // (PR = 2), and after every batch that has not converged a search of the parent
    // graph that cancels the negative cycles it holds. 1 = certified (prices set),
    // 0 = gave up within cap rounds (the final cost-scaling phase follows), < 0 error.
    int finish(int* rounds_used, int cap) {
        KS_CHECK(hipEventRecord(s.ev[5], st));
        KS_CHECK(s.cyc.ensure((size_t)9 * nn));
        KS_CHECK(s.cyc64.ensure((size_t)2 * nn));
        fin = Finish{};
        fin.cap = cap;
        fin.JMa = reinterpret_cast<int2*>(s.cyc.p);
        fin.JMb = fin.JMa + nn;
        fin.J0 = reinterpret_cast<int*>(fin.JMb + nn);
        fin.onc = fin.J0 + nn;
        fin.R = fin.onc + nn;
        fin.gbad = fin.R + nn;
        fin.indeg = fin.gbad + nn;
        fin.gsum = s.cyc64.p;
        fin.gcap = fin.gsum + nn;
        KS_CHECK(set_eps(1, SET_CYC));   // and cyc_done, cyc_rej zeroed
        hipLaunchKernelGGL(k_pr_init, dim3(ngrid), dim3(BLK), 0, st, g, bseq, 2);
        // graphs whose parent graph fits one workgroup's LDS search in one launch
        // (k_cyc_lds) instead of 12–15
        fin.lds_search = nn <= CYC_LDS_MAX && cyc_lds_bytes(nn) <= s.lds_limit;
        if (fin.lds_search) {
            KS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cyc_lds<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)cyc_lds_bytes(nn)));
            KS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cyc_lds<false>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)cyc_lds_bytes(nn)));
        }
        // Batches of CYC_PERIODS × (CYC_EVERY[_LDS] rounds + a search), pipelined two deep:
        // batch b+1 is enqueued before the host waits for batch b's control snapshot
        // (k_prc_snap, into pinned memory), so the GPU does not idle through the
        // host's round trip (~27 µs per batch with a copy-engine read, r06 traces).
        // Once the refinement has converged, every kernel of the batch in flight
        // exits at once. A batch's Bellman-Ford time is its event span less its
        // searches (device clock: k_cyc_par / k_cyc_lds to the next round's start).
        // One event per batch, after its snapshot: batch b's span runs from batch
        // b−1's event (the first: fin_ev[3]) — two events back to back cost a gap each.
        int ok = 0;
        KS_CHECK(hipEventRecord(s.fin_ev[3], st));
        KS_CHECK(enqueue_batch(0));
        int done_b = 0;   // batches whose snapshot the host has read
        for (int batch = 0;; ++batch) {
            const int slot = batch & 1;
            const bool more = fin.used < fin.cap;
            if (more) KS_CHECK(enqueue_batch(slot ^ 1));
            KS_CHECK(hipEventSynchronize(batch_end(batch)));
            ++done_b;
            const Ctl* hc = s.h_cyc[slot];
            const double span = batch_time(batch);
            cp_dirty = cpv;
            if (cycle_log) {   // one line per batch: rounds so far, cycles so far, relaxations, time
                unsigned long long relax = 0;
                if (int rc = relaxations(&relax)) return rc;
                std::fprintf(stderr, "finish batch %d rounds %d worked %d cycles %d rejected %d relax %llu ms %.3f (searches %.3f)\n",
                             batch, fin.used, hc->bf_count, hc->cyc_done, hc->cyc_rej, relax, span,
                             (double)hc->srch_ticks / 1e5);
            }
            if (hc->bf_done) {
                ok = 1;
                break;
            }
            if (!more) break;   // the round cap: this was the last batch
        }
        if (fin.nb > done_b) {   // the batch enqueued behind the converged one (its kernels exited at once)
            KS_CHECK(hipEventSynchronize(batch_end(fin.nb - 1)));
            batch_time(fin.nb - 1);
        }
        if (ok) hipLaunchKernelGGL(k_pr_apply, dim3(ngrid), dim3(BLK), 0, st, g, 1);
        KS_CHECK(hipEventRecord(s.ev[6], st));
        KS_CHECK(hipEventSynchronize(s.ev[6]));
        ms_pr += ev_ms(s.ev[5], s.ev[6]);
        KS_CHECK(read_ctl());
        prc_cycles += s.h_ctl->cyc_done;
        prc_rejected += s.h_ctl->cyc_rej;
        *rounds_used = fin.used;
        if (cycle_log)
            std::fprintf(stderr, "cycle-cancelling refinement: %s after %d rounds, %d searches, %d cycles cancelled\n",
                         ok ? "certified" : "gave up", fin.used, prc_searches, s.h_ctl->cyc_done);
        return ok;
    }
    // the parent graph: pointer doubling over CYC_WALK steps, cycles grouped by
    // their least id, every good negative one cancelled in parallel (each kernel
    // returns at once when the refinement has converged)
    void search() {
        const Finish& f = fin;
        const int* done = &s.ctl.p->bf_done;
        // three of four searches double only CYC_SHORT times (cycles of up to 128
        // arcs: the ones the finish meets); every fourth covers 2^CYC_LOG
        // (fault_inject bit 7: every search cyc_lg = 5 steps)
        const bool full = (o.fault_inject & 128) || fin.nsearch++ % 4 == 3;
        const int lg = full ? cyc_lg : CYC_SHORT;
        const int apply_check = (o.fault_inject & 256) ? 0 : 1;
        if (f.lds_search) {   // small graphs: the whole search in one workgroup, in LDS
            KS_HOT_LDS(cpv, k_cyc_lds, 1, CYC_LDS_T, cyc_lds_bytes(nn), st, g, lg, apply_check, bseq, f.gsum, f.gcap,
                       f.gbad);
            return;
        }
        KS_HOT(cpv, k_cyc_par, ngrid, BLK, st, g, f.J0, f.JMa, f.onc, f.R, f.gsum, f.gcap, f.gbad, f.indeg);
        const int2* JMK = f.JMa;
        for (int left = lg, k = 0; left > 0; ++k) {   // ×4 per launch, ×2 for an odd remainder
            const int2* in = (k & 1) ? f.JMb : f.JMa;
            int2* out = (k & 1) ? f.JMa : f.JMb;
            const int f2 = left >= 2 ? 2 : 1;
            left -= f2;
            const int mark = left == 0 ? 1 : 0;
            if (f2 == 2)
                hipLaunchKernelGGL(k_cyc_jump<4>, dim3(ngrid), dim3(BLK), 0, st, nn, done, in, out, mark,
                                   (const int*)f.J0, f.onc);
            else
                hipLaunchKernelGGL(k_cyc_jump<2>, dim3(ngrid), dim3(BLK), 0, st, nn, done, in, out, mark,
                                   (const int*)f.J0, f.onc);
            JMK = out;
        }
        KS_HOT(cpv, k_cyc_group, ngrid, BLK, st, g, (const int*)f.J0, JMK, (const int*)f.onc, (const int*)f.R, f.gsum,
               f.gcap, f.gbad, f.indeg);
        hipLaunchKernelGGL(k_cyc_check, dim3(ngrid), dim3(BLK), 0, st, nn, done, (const int*)f.J0, JMK,
                           (const int*)f.onc, (const int*)f.indeg, f.gbad, apply_check, &s.ctl.p->cyc_rej);
        KS_HOT(cpv, k_cyc_push, ngrid, BLK, st, g, (const int*)f.J0, JMK, (const int*)f.onc, (const int*)f.R,
               (const long long*)f.gsum, (const long long*)f.gcap, (const int*)f.gbad, bseq);
    }
    hipEvent_t batch_end(int b) const { return s.fin_ev[b % 3]; }
    hipEvent_t batch_start(int b) const { return b == 0 ? s.fin_ev[3] : s.fin_ev[(b - 1) % 3]; }
    hipError_t enqueue_batch(int slot) {
        const int b = fin.nb++;
        for (int per = 0; per < (b == 0 ? 1 : CYC_PERIODS) && fin.used < fin.cap; ++per) {
            const int every = fin.lds_search ? CYC_EVERY_LDS : CYC_EVERY;
            const int k = std::min(b == 0 ? 2 * every : every, fin.cap - fin.used);
            bf_rounds(2, k, b == 0);
            fin.used += k;
            search();
            ++prc_searches;
        }
        hipLaunchKernelGGL(k_prc_snap, dim3(1), dim3(128), 0, st, g, s.d_cyc[slot]);
        return hipEventRecord(batch_end(b), st);
    }
    double batch_time(int b) {   // → ms_bf_k
        const Ctl* hc = s.h_cyc[b & 1];
        const double span = ev_ms(batch_start(b), batch_end(b));
        const double srch = hc->srch_ticks > fin.srch_seen ? (double)(hc->srch_ticks - fin.srch_seen) / 1e5 : 0.0;
        fin.srch_seen = std::max(fin.srch_seen, hc->srch_ticks);
        ms_bf_k += std::max(0.0, span - srch);
        return span;
    }

    // ------------------------------------------------------- cell solver ---
    // The cell solver (ks_cell.h): every cell's whole solve in one workgroup, one
    // launch for all cells. `retry` is set when the engine must take over: a value the
    // compact record cannot hold (RETRY_RANGE), or cells that gave up (RETRY_CELLS).
    int cell_solve() {
        KS_CHECK(s.cl_pos.ensure(std::max<int64_t>(m2, 1)));
        KS_CHECK(hipEventRecord(s.ev[3], st));
        if (!run_all && run_list.empty()) {   // no cell changed since its last solve: no launch,
            eps = 1;                          // verification reports the flow in place again
            return KS_OK;
        }
        const int cs = run_cells(0);
        if (cs < 0) return cs;
        if (cs == CS_RANGE) {
            retry = RETRY_RANGE;
            return KS_OK;
        }
        KS_CHECK(hipEventRecord(s.ev[4], st));
        KS_CHECK(hipEventSynchronize(s.ev[4]));
        ms_cycles += ev_ms(s.ev[3], s.ev[4]);
        if (cs == CS_TIMEOUT || cs == CS_NOCONV) {
            retry = RETRY_CELLS;
            return KS_OK;
        }
        if (int rc = cell_status(cs, "solve")) return rc;
        eps = 1;
        return KS_OK;
    }
    // One launch (mode 0: the solve; 1: certificate recovery at ε = 1); per-cell status
    // and counters come back in CellOut. Returns the worst CellStatus, or < 0.
    int run_cells(int mode) {
        CellArgs a{};
        a.pos = s.pos.p;
        a.cp = s.cl_pos.p;
        a.first = s.first.p;
        a.m2 = (int)s.m2cap;
        a.nd = s.nd.p;
        a.excess = s.excess.p;
        a.cells = s.cells.p;
        a.ncells = ncells;
        // the solve launches the listed cells only; the certificate recovery, every cell
        const bool part = mode == 0 && !run_all;
        a.list = nullptr;
        a.nlist = ncells;
        if (part) {
            s.h_cell_list = run_list;   // (the copy's source outlives the stream's use of it)
            KS_CHECK(s.cell_list.ensure(run_list.size()));
            KS_CHECK(hipMemcpyAsync(s.cell_list.p, s.h_cell_list.data(), run_list.size() * sizeof(int),
                                    hipMemcpyHostToDevice, st));
            // a skipped cell reports "ok, zero work"
            KS_CHECK(hipMemsetAsync(s.cl_out.p, 0, ncells * sizeof(CellOut), st));
            a.list = s.cell_list.p;
            a.nlist = (int)run_list.size();
        }
        cells_run = part ? (int)run_list.size() : ncells;
        a.nn = nn;
        a.lists = s.cl_lists.p;
        a.rl_node = s.cl_rln.p;
        a.rl_p = s.cl_rlp.p;
        a.out = s.cl_out.p;
        a.mult = mult;
        a.eps_start = eps_start;
        a.sat_thr0 = warm_thr;
        a.warm = use_warm ? (o.warm_start >= 2 ? 2 : 1) : 0;
        a.alpha = alpha;
        a.pr_div = (int)pr_div;
        a.use_pr = use_pr ? 1 : 0;
        a.pr_cap = pr_cap;
        a.use_prc = (use_pr && o.price_refine == 1 && !use_warm && mode == 0) ? 1 : 0;
        a.prc_cap = prc_cap;
        a.gi = gi_base;
        a.bound = o.bf_bound < 0 ? 0 : 1;
        a.phase_exit = phase_exit;
        a.phase_frac = phase_frac;
        a.mode = mode;
        a.max_nodes = s.cell_max;
        a.timeout_ticks = (unsigned long long)(kCellLimitS * 1e8);
        a.diag = cycle_log ? 1 : 0;
        // TESTS ONLY (fault_inject bit 4): the middle cell gives up after 40 operations
        a.fault_cell = (o.fault_inject & 16) && mode == 0 ? ncells / 2 : -1;
        if (part && a.fault_cell >= 0) {   // (the kernel compares its workgroup index: the cell's place in the list)
            const auto it = std::find(run_list.begin(), run_list.end(), a.fault_cell);
            a.fault_cell = it == run_list.end() ? -1 : (int)(it - run_list.begin());
        }
        a.fault_ops = 40;
        a.cyc_lg = cyc_lg;
        KS_CHECK(hipEventRecord(s.kev[2], st));
        {   // a launch the device refuses (its LDS) → the multi-kernel engine instead; any
            // other launch error is reported (it used to disable the cell solver)
            bool refused = false;
            const hipError_t le = cell_launch(a, s.cl_bad.p, s.lds_limit, st, &refused);
            if (le != hipSuccess) {
                (void)hipGetLastError();
                if (refused) {
                    launch_refused = true;
                    return (int)CS_RANGE;
                }
                err = std::string("cell solver launch: ") + hipGetErrorString(le);
                return KS_E_DEVICE;
            }
        }
        KS_CHECK(hipEventRecord(s.kev[3], st));
        KS_CHECK(hipMemcpyAsync(s.h_cell_out.data(), s.cl_out.p, ncells * sizeof(CellOut), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        ms_cell += ev_ms(s.kev[2], s.kev[3]);
        int worst = CS_OK, pmax = 0;
        for (const CellOut& o : s.h_cell_out)
            if (o.status == CS_RANGE) return (int)CS_RANGE;
        for (const CellOut& o : s.h_cell_out) {
            if (o.status != CS_OK && (worst == CS_OK || worst == CS_INFEASIBLE)) worst = o.status;
            pmax = std::max(pmax, o.phases);
            sweeps += o.sweeps;
            gus += o.updates;
            cell_rounds += o.bf_rounds;
            cell_ctr[0] += o.scans;
            cell_ctr[1] += o.visits;
            cell_ctr[2] += o.pushes;
            cell_ctr[3] += o.relabels;
            cell_ctr[4] += o.gu_scans;
            prc_cycles += o.cycles;
            prc_rejected += o.rejected;
            cticks_max = std::max<unsigned long long>(cticks_max, o.ticks);
            cticks_sum += o.ticks;
        }
        phases += pmax;
        if (cycle_log) log_slowest_cell();
        return worst;
    }
    // per-operation device time of the slowest cell (ks_opts.log_cycles)
    void log_slowest_cell() const {
        size_t w = 0;
        for (size_t i = 1; i < s.h_cell_out.size(); ++i)
            if (s.h_cell_out[i].ticks > s.h_cell_out[w].ticks) w = i;
        const CellOut& o = s.h_cell_out[w];
        static const char* names[CELL_NOPS] = {"sat", "gu_init", "bf", "gu_fin", "sweep", "pr_init", "pr", "pr_fin",
                                               "cyc"};
        std::fprintf(stderr, "cell %zu of %d: %.3f ms, phases %d updates %d sweeps %llu rounds %llu:", w, ncells,
                     o.ticks / 1e5, o.phases, o.updates, o.sweeps, o.bf_rounds);
        for (int i = 0; i < CELL_NOPS; ++i)
            if (o.op_n[i])
                std::fprintf(stderr, " %s %u x %.2f us (items %.2f..%.2f)", names[i], o.op_n[i],
                             o.op_ticks[i] / 100.0 / o.op_n[i], o.first_ticks[i] / 100.0 / o.op_n[i],
                             o.item_ticks[i] / 100.0 / o.op_n[i]);
        static const char* const steps[4] = {"sweep", "bf", "pr", "sat"};
        for (int s = 0; s < 4; ++s) {
            std::fprintf(stderr, "\n  %s items:", steps[s]);
            for (int c = 0; c < 7; ++c)
                if (o.cls_n[8 * s + c])
                    std::fprintf(stderr, " c%d %u x %.2f us", c, o.cls_n[8 * s + c],
                                 o.cls_ticks[8 * s + c] / 100.0 / o.cls_n[8 * s + c]);
        }
        std::fprintf(stderr, "\n  finish: cycles %d searches %d parents %u marked %u leaders %u closed %u", o.cycles,
                     o.searches, o.cyc_dbg[0], o.cyc_dbg[1], o.cyc_dbg[2], o.cyc_dbg[3]);
        std::fprintf(stderr, "\n  ms by phase:");
        for (int i = 0; i < 8; ++i)
            if (o.phase_ticks[i]) std::fprintf(stderr, " %s%d %.2f", i == 7 ? "pr/" : "p", i + 1, o.phase_ticks[i] / 1e5);
        static const char* const sz[6] = {"<=16", "<=64", "<=256", "<=1k", "<=4k", ">4k"};
        for (int h = 0; h < 12; ++h) {
            if (h % 6 == 0) std::fprintf(stderr, "\n  %s by frontier:", h ? "bf" : "sweep");
            if (o.hist_n[h])
                std::fprintf(stderr, " %s %u x %.2f us", sz[h % 6], o.hist_n[h], o.hist_t[h] / 100.0 / o.hist_n[h]);
        }
        std::fprintf(stderr, "\n");
    }
    int cell_status(int cs, const char* what) {
        if (cs == CS_OK) return KS_OK;
        if (cs == CS_INFEASIBLE) {
            status = KS_E_INFEASIBLE;
            err = std::string("infeasible: some supply cannot reach a demand node (cell solver, ") + what + ")";
            return KS_OK;
        }
        err = std::string("cell solver did not converge (") + (cs == CS_TIMEOUT ? "wall-clock limit" : "step cap") +
              ", " + what + ")";
        return KS_E_DEVICE;
    }

    // ------------------------------------------------------------ verify ---
    // The certificate of a solve that ended feasible: verification, the repair of a
    // failed optimality certificate, and a warm start's canonical prices.
    int certify() {
        if (o.fault_inject & 2)   // TESTS ONLY: break the certificate, not the flow
            hipLaunchKernelGGL(k_perturb_price, dim3(1), dim3(1), 0, st, g, 0, 1000 * mult);
        int bad = 0;
        int rc = verify(&bad);
        if (rc) return rc;
        if ((rc = recover(&bad))) return rc;
        if (status == KS_OK && cost_range) {   // (whatever ks_opts.verify says: the number would be wrong)
            char what[96];
            if (cost_wide)
                std::snprintf(what, sizeof(what), "a single arc's flow * cost, or one thread's share, is beyond 2^64");
            else
                std::snprintf(what, sizeof(what), "the sum of |flow * cost| is %.6g", cost_mag);
            status = KS_E_RANGE;
            err = std::string("total cost outside int64: ") + what + ", the limit is 2^63 (9.22337e+18)";
            tot_cost = 0;
        }
        if (status == KS_OK && bad && o.verify) {
            status = KS_E_VERIFY;
            err = std::string("on-device verification failed (") + ((bad & 1) ? "capacity " : "") +
                  ((bad & 2) ? "optimality " : "") + ((bad & 4) ? "conservation" : "") + ")";
        }
        // warm starts: replace the carried prices by the flow's canonical ones (the
        // next round starts from prices without history). Kept only if the
        // Bellman-Ford converges; the certificate holds either way.
        if (status == KS_OK && !bad && o.warm_start > 0 && o.warm_canon >= 0 && !s.cell_layout) {
            int used = 0;
            const int pr = price_refine(1, &used, 4 * pr_cap, 1);
            if (pr < 0) return pr;
            if (cycle_log) std::fprintf(stderr, "canonical prices: %s after %d rounds\n", pr ? "set" : "not converged", used);
        }
        return KS_OK;
    }
    // Conservation, capacity, 1-optimality of the final prices (scaled units), the
    // int64 cost and the flow value measured from the resident flow. → verify_bad bits
    int verify(int* bad) {
        sync_pos();   // the compact solve's residuals back into the 32-B records first
        if ((o.fault_inject & 64) && m2)   // TESTS ONLY: break conservation, not the excess words
            hipLaunchKernelGGL(k_break_conservation, dim3(1), dim3(64), 0, st, g, (long long)m2);
        KS_CHECK(hipMemsetAsync(&s.ctl.p->verify_bad, 0, sizeof(int), st));
        KS_CHECK(set_eps(1));
        hipLaunchKernelGGL(k_drain_all, dim3((std::max(1, s.nheavy) + BLK - 1) / BLK), dim3(BLK), 0, st, g);
        KS_CHECK(s.vbal.ensure(std::max<int64_t>(s.ncap, 1)));
        KS_CHECK(hipMemsetAsync(s.vbal.p, 0, std::max<int64_t>(s.ncap, 1) * sizeof(long long), st));
        if (hi)
            hipLaunchKernelGGL(k_verify_arcs, dim3(vgrid), dim3(BLK), 0, st, g, hi, (const unsigned char*)s.a_alive.p,
                               (const int*)s.fwd.p, (const int*)s.a_src.p, (const int*)s.a_dst.p,
                               (const long long*)s.n_supply.p, (const long long*)s.a_low.p,
                               (const long long*)s.a_cap.p, (const long long*)s.a_cost.p, s.flows.p, s.part.p,
                               s.part.p + 4096, s.vbal.p);
        if (s.ncap)
            hipLaunchKernelGGL(k_verify_balance, dim3(grid_for(s.ncap, 2048)), dim3(BLK), 0, st, g, (int)s.ncap,
                               (const unsigned char*)s.n_alive.p, (const long long*)s.n_supply.p,
                               (const long long*)s.vbal.p);
        if (m2) hipLaunchKernelGGL(k_verify_opt, dim3(grid_for(m2, 2048)), dim3(BLK), 0, st, g, (long long)m2);
        hipLaunchKernelGGL(k_verify_nodes, dim3(ngrid), dim3(BLK), 0, st, g);
        // per block: the signed cost sums, then the high halves of Σ |flow·cost|, in part; the
        // flow values, then the low halves, in part + 4096
        std::vector<long long> parts(hi ? 2 * vgrid : 0), partf(hi ? 2 * vgrid : 0);
        if (hi) {
            KS_CHECK(hipMemcpyAsync(parts.data(), s.part.p, parts.size() * sizeof(long long), hipMemcpyDeviceToHost,
                                    st));
            KS_CHECK(hipMemcpyAsync(partf.data(), s.part.p + 4096, partf.size() * sizeof(long long),
                                    hipMemcpyDeviceToHost, st));
        }
        KS_CHECK(read_ctl());
        tot_cost = tot_flow = 0;
        unsigned __int128 mag = 0;
        for (int b = 0; hi && b < vgrid; ++b) {
            tot_cost = (long long)((unsigned long long)tot_cost + (unsigned long long)parts[b]);
            tot_flow += partf[b];
            mag += ((unsigned __int128)(unsigned long long)parts[vgrid + b] << 32) +
                   (unsigned long long)partf[vgrid + b];
        }
        *bad = s.h_ctl->verify_bad & ~VERIFY_COST_RANGE;
        cost_wide = (s.h_ctl->verify_bad & VERIFY_COST_RANGE) != 0;
        cost_range = cost_wide || mag >= ((unsigned __int128)1 << 63);
        cost_mag = (double)mag;
        return KS_OK;
    }
    // A failed optimality certificate on a feasible flow is repaired, not fatal:
    // price refinement at ε = 1 (the flow may be optimal, only its prices off),
    // else one more ε = 1 phase from the current flow (saturating only the arcs
    // that violate 1-optimality), then verification again. Capacity and
    // conservation violations stay fatal (KS_E_VERIFY).
    int recover(int* bad) {
        for (int attempt = 0; attempt < 2 && *bad == 2; ++attempt) {
            ++res.recoveries;
            if (s.cell_layout) {   // the same repair inside each cell's workgroup
                const int cs = run_cells(1);
                if (cs < 0) return cs;
                if (int rc = cell_status(cs, "certificate recovery")) return rc;
                if (status != KS_OK) return KS_OK;
            } else {
                int used = 0;
                const int pr = price_refine(1, &used, 4 * pr_cap);
                if (pr < 0) return pr;
                if (pr == 0) {
                    ++phases;
                    const int rc = run_phase(1, 1, false, 1);
                    if (rc == KS_E_INFEASIBLE) {
                        status = rc;
                        err = "infeasible during certificate recovery";
                        return KS_OK;
                    }
                    if (rc) return rc;
                }
            }
            if (int rc = verify(bad)) return rc;
        }
        return KS_OK;
    }

    // ------------------------------------------------------------ report ---
    int report() {
        sync_pos();   // (a solve that ended without verification: Pos stays the authoritative copy)
        KS_CHECK(hipEventRecord(s.ev[6], st));
        unsigned long long hc[CTR_SHARDS * NCTR];
        KS_CHECK(hipMemcpyAsync(hc, s.ctr.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        unsigned long long tc[NCTR] = {0};
        for (int i = 0; i < CTR_SHARDS; ++i)
            for (int k = 0; k < NCTR; ++k) tc[k] += hc[i * NCTR + k];
        if (s.cell_layout) {
            tc[C_SCAN] += cell_ctr[0];
            tc[C_VISIT] += cell_ctr[1];
            tc[C_PUSH] += cell_ctr[2];
            tc[C_RELABEL] += cell_ctr[3];
            tc[C_GUSCAN] += cell_ctr[4];
            tc[C_BFROUND] += cell_rounds;
        }
        if (cycle_log)
            std::fprintf(stderr, "solve tail walks to a deficit %llu, hops %llu, recoveries %d\n", tc[C_AUGWALK],
                         tc[C_AUGHOP], res.recoveries);

        res.total_cost = tot_cost;
        res.flow_value = tot_flow;
        res.phases = phases;
        res.sweeps = sweeps;
        res.arc_scans = tc[C_SCAN];
        res.node_visits = tc[C_VISIT];
        res.pushes = tc[C_PUSH];
        res.relabels = tc[C_RELABEL];
        res.global_updates = gus;
        res.gu_iterations = tc[C_BFROUND];
        res.ms_phase[0] = ev_ms(s.ev[0], s.ev[1]);
        res.ms_phase[1] = ms_sat;
        res.ms_phase[2] = ms_cycles;
        res.ms_phase[3] = ms_pr;
        res.ms_phase[4] = ev_ms(s.ev[5], s.ev[6]);
        res.ms_phase[5] = 1e3 * wall_s();
        res.gu_arc_scans = tc[C_GUSCAN];
        res.gu_leaf_scans = tc[C_GULEAF];
        res.fs_arc_scans = tc[C_FSSCAN];
        res.sweep_launches = sweep_kernels;
        res.ms_sweep_kernels = ms_sw_k;
        res.gu_launches = bf_launches;
        res.ms_gu_kernels = ms_bf_k;
        res.fs_launches = fs_launches;
        res.ms_fs_kernels = ms_fs_k;
        res.fwd_updates = fwd_updates;
        res.solver = s.cell_layout ? 1 : 0;
        res.cells = s.cell_layout ? ncells : 0;
        res.cells_run = s.cell_layout ? cells_run : 0;
        res.ms_cell_kernel = ms_cell;
        res.cell_ticks_max = cticks_max;
        res.cell_ticks_sum = cticks_sum;
        res.status = status;
        res.cycles_cancelled = (uint64_t)prc_cycles;
        res.cycles_rejected = (uint64_t)prc_rejected;
        KS_CHECK(hipMemsetAsync(s.n_cshift.p, 0, s.nstore * sizeof(unsigned long long), st));
        if (status == KS_OK) {
            KS_CHECK(hipMemsetAsync(s.n_fresh.p, 0, s.nstore, st));
            // every cell now holds its optimum: the dirty flags start over
            if (s.cell_first_valid && s.cell_dirty.p)
                KS_CHECK(hipMemsetAsync(s.cell_dirty.p, 0, (s.cell_off.size() - 1) * sizeof(int), st));
            KS_CHECK(hipStreamSynchronize(st));
            s.solved = true;
            s.has_prev = true;
            s.cells_kept = s.cell_layout;
        } else {
            s.has_prev = false;   // a failed solve leaves no usable warm state
            s.cells_kept = false;
        }
        return status;
    }
};

}  // namespace

// The driver: one SolveRun, and the cell solver's two hand-overs to the multi-kernel
// engine, each a second run over the same graph in the engine's node order.
int Engine::solve(ks_result& res, bool warm, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    SolveRun run(s, res, err, warm);
    const int rc = run.run();
    if (run.retry == SolveRun::RETRY_RANGE) {   // a value the compact record cannot hold: the multi-kernel engine instead
        s.cell_refused = true;
        s.cell_refused_values = !run.launch_refused;   // (an arc delta may bring the values back into range)
        s.cell_layout = false;
        s.csr_valid = false;
        // the warm start's price shift is already in the carried prices: the retry
        // must not apply it a second time
        if (run.use_warm) KS_CHECK(hipMemsetAsync(s.n_cshift.p, 0, s.nstore * sizeof(unsigned long long), s.stream));
        return solve(res, warm, err);
    }
    if (run.retry == SolveRun::RETRY_CELLS) {
        // Per-cell fallback: only the cells that gave up are solved again, on the
        // multi-kernel engine (engine order, the state carried across the rebuild:
        // the converged cells keep their optimal flows and prices, the failing ones
        // restart cold). One hard cell no longer discards the batch.
        std::vector<int> bad;
        for (size_t i = 0; i < s.h_cell_out.size(); ++i)
            if (s.h_cell_out[i].status == CS_TIMEOUT || s.h_cell_out[i].status == CS_NOCONV) bad.push_back((int)i);
        s.fb_cells = bad;
        s.fb_active = true;
        s.cell_layout = false;
        s.csr_valid = false;
        const int rc2 = solve(res, warm, err);
        s.fb_active = false;
        s.fb_cells.clear();
        res.cell_fallbacks = bad.size();
        res.solver = 1;
        res.cells = run.ncells;
        res.cells_run = run.cells_run;
        return rc2;
    }
    return rc;
}

}  // namespace ks
