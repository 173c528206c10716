// ks_engine_build.hip — the engine's residual CSR, built on the device from the arc
// table of the store, and the cold reset of its flow and prices.
// Entry points: build() and cold_reset(), declared in ks_engine_impl.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ks_engine_impl.h"

namespace ks {
namespace {

// ===================================================================== build ===
// The residual CSR is built on device from the arc table of the store
// (ks_store.h). Every node owns a segment of CAPACITY positions: its live arcs
// (forward arcs and reverses of its in-arcs), plus slack once the graph is
// edited incrementally, so later inserts land in place. Internal ids group the
// nodes by the degree class of their capacity, hubs last; dead positions are
// inert (no capacity, head = owner, cost DEAD_COST).
__global__ void k_degree(int hi, const unsigned char* __restrict__ alive, const int* __restrict__ src,
                         const int* __restrict__ dst, int* __restrict__ deg) {
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK)
        if (alive[s]) {
            atomicAdd(&deg[src[s]], 1);
            atomicAdd(&deg[dst[s]], 1);
        }
}

// Segment capacity of a node slot. Tight after a load (its degree). Once the
// graph is edited incrementally: tasks (≤ 8 arcs: preferences, or one running
// arc after the pin) one 8-lane group — a removed task's segment is reused
// whole by the task that takes over its id (flowgraph/graph.go:169-182), and
// so are dead and spare slots; other nodes their degree +50 % (at least 4)
// rounded up to a lane group (≤ 64) or a 64-arc chunk, never less than what
// they had before (hint) unless that is 4× their need — an aggregator whose
// degree fell after the pins keeps room for the next arrivals — and twice that
// when an insert overflowed them since the last build.
__host__ __device__ inline int seg_capacity(int deg, bool alive, bool task, int slack) {
    if (!slack) return deg;
    if ((!alive || task) && deg <= 8) return 8;
    const int c = deg + (deg / 2 > 4 ? deg / 2 : 4);
    if (c <= 64) {
        int g = 4;
        while (g < c) g <<= 1;
        return g;
    }
    return (c + 63) / 64 * 64;
}

__global__ void k_capacity(int ncap, int nstore, const int* __restrict__ deg, const unsigned char* __restrict__ alive,
                           const unsigned char* __restrict__ type, int slack, int* __restrict__ hint,
                           unsigned char* __restrict__ grow, int* __restrict__ capv, unsigned char* __restrict__ cls) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        const int d = v < nstore ? deg[v] : 0;
        const bool a = v < nstore && alive[v];
        int c = seg_capacity(d, a, a && type[v] == KS_NODE_TASK, slack);
        if (slack && v < nstore) {
            const int h = hint[v];
            if (grow[v]) c = max(c, 2 * max(h, 4));
            else if (h <= 4 * c) c = max(c, h);
            else c = max(c, h / 2);
            if (c > 64) c = (c + 63) / 64 * 64;
            grow[v] = 0;
        }
        if (v < nstore) hint[v] = c;
        capv[v] = c;
        cls[v] = (unsigned char)degree_class(c);
    }
}

// perm[list[i]] = base + i (one class, or the hubs).
__global__ void k_make_perm(int cnt, int base, const int* __restrict__ list, int* __restrict__ perm) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < cnt; i += (long long)gridDim.x * BLK)
        perm[list[i]] = base + (int)i;
}

__global__ void k_capi(int ncap, const int* __restrict__ perm, const int* __restrict__ capv, int* __restrict__ capi,
                       int* __restrict__ iperm) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK) {
        capi[perm[v]] = capv[v];
        iperm[perm[v]] = (int)v;
    }
}

// Sort keys: the tail (internal id) of every residual arc; dead slots sort last.
__global__ void k_pos_keys(int hi, int sentinel, const unsigned char* __restrict__ alive, const int* __restrict__ src,
                           const int* __restrict__ dst, const int* __restrict__ perm, unsigned* __restrict__ keys,
                           int* __restrict__ vals) {
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK) {
        const bool a = alive[s];
        keys[2 * s] = a ? (unsigned)perm[src[s]] : (unsigned)sentinel;
        keys[2 * s + 1] = a ? (unsigned)perm[dst[s]] : (unsigned)sentinel;
        vals[2 * s] = (int)(2 * s);
        vals[2 * s + 1] = (int)(2 * s + 1);
    }
}

// rs[v] = lower bound of v in the sorted keys, v ∈ [0, nn].
__global__ void k_first(int nn, long long m2, const unsigned* __restrict__ keys, int* __restrict__ rs) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v <= nn; v += (long long)gridDim.x * BLK) {
        long long lo = 0, hi = m2;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (keys[mid] < (unsigned)v) lo = mid + 1; else hi = mid;
        }
        rs[v] = (int)lo;
    }
}

// Every position inert, owned by the node whose segment holds it.
__global__ void k_inert_all(long long m2cap, int nn, const int* __restrict__ first, Pos* __restrict__ pos,
                            int* __restrict__ ent) {
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2cap; p += (long long)gridDim.x * BLK) {
        int lo = 0, hi = nn;   // owner: the last v with first[v] <= p
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= p) lo = mid; else hi = mid;
        }
        pos[p] = Pos{DEAD_COST, 0, 0, lo, (int)p};
        ent[p] = -1;
    }
}

__global__ void k_fill_csr(long long m2, int nn, const unsigned* __restrict__ keys, const int* __restrict__ vals,
                           const int* __restrict__ rs, const int* __restrict__ first, const int* __restrict__ perm,
                           const int* __restrict__ src, const int* __restrict__ dst, const long long* __restrict__ low,
                           const long long* __restrict__ cap, const long long* __restrict__ cost, long long mult,
                           Pos* __restrict__ pos, int* __restrict__ ent, int* __restrict__ fwd,
                           int* __restrict__ pos_of) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < m2; i += (long long)gridDim.x * BLK) {
        const int v = (int)keys[i];
        if (v >= nn) continue;
        const int p = first[v] + (int)(i - rs[v]);
        const int val = vals[i];
        const int s = val >> 1;
        const bool r = val & 1;
        pos_of[val] = p;
        const long long u = cap[s] - low[s];
        pos[p].head = perm[r ? src[s] : dst[s]];
        pos[p].rcap = r ? 0 : u;
        pos[p].ucap = u;
        pos[p].cost = (r ? -cost[s] : cost[s]) * mult;
        ent[p] = val;
        if (!r) fwd[s] = p;
    }
}

__global__ void k_fill_rev(long long m2, int nn, const unsigned* __restrict__ keys, const int* __restrict__ vals,
                           const int* __restrict__ pos_of, Pos* __restrict__ pos) {
    for (long long i = blockIdx.x * (long long)BLK + threadIdx.x; i < m2; i += (long long)gridDim.x * BLK) {
        if ((int)keys[i] >= nn) continue;
        const int val = vals[i];
        pos[pos_of[val]].rev = pos_of[val ^ 1];
    }
}

__global__ void k_used(int nn, const int* __restrict__ rs, int* __restrict__ used) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < nn; v += (long long)gridDim.x * BLK)
        used[v] = rs[v + 1] - rs[v];
}

// ------------------------------------------------------------ cold reset ---
// Zero flow: forward residual = u, reverse 0; excess = supply with the
// lower-bound transform; prices 0. Runs before every cold solve (no rebuild).
__global__ void k_reset_pos(long long m2cap, const int* __restrict__ ent, Pos* __restrict__ pos) {
    for (long long p = blockIdx.x * (long long)BLK + threadIdx.x; p < m2cap; p += (long long)gridDim.x * BLK) {
        const int e = ent[p];
        if (e >= 0) pos[p].rcap = (e & 1) ? 0 : pos[p].ucap;
    }
}

// Segment bounds into the node records (the CSR's first[] is fixed per build).
__global__ void k_node_bounds(int nn, const int* __restrict__ first, long long* __restrict__ nd) {
    for (long long x = blockIdx.x * (long long)BLK + threadIdx.x; x < nn; x += (long long)gridDim.x * BLK)
        nd[ni(x) + ND_SEG] = (long long)(((unsigned long long)(unsigned)first[x + 1] << 32) | (unsigned)first[x]);
}

__global__ void k_reset_nodes(int nn, int ncap, const int* __restrict__ iperm, const unsigned char* __restrict__ alive,
                              const long long* __restrict__ supply, long long* __restrict__ excess,
                              long long* __restrict__ p0, long long* __restrict__ p1) {
    for (long long x = blockIdx.x * (long long)BLK + threadIdx.x; x < nn; x += (long long)gridDim.x * BLK) {
        const int v = iperm[x];
        excess[x] = (v >= 0 && v < ncap && alive[v]) ? supply[v] : 0;
        p0[ni(x)] = 0;
        p1[ni(x)] = 0;
    }
}

__global__ void k_reset_low(int hi, const unsigned char* __restrict__ alive, const int* __restrict__ src,
                            const int* __restrict__ dst, const int* __restrict__ perm,
                            const long long* __restrict__ low, long long* __restrict__ excess) {
    for (long long s = blockIdx.x * (long long)BLK + threadIdx.x; s < hi; s += (long long)gridDim.x * BLK) {
        const long long l = low[s];
        if (alive[s] && l) {
            atom_add(&excess[perm[src[s]]], -l);
            atom_add(&excess[perm[dst[s]]], l);
        }
    }
}


struct ClassIs {
    const unsigned char* cls;
    unsigned char c;
    __host__ __device__ bool operator()(const int& v) const { return cls[v] == c; }
};

}  // namespace

// Cell-major internal ids for the cell solver (ks_cell.h): every cell (a ks_batch
// graph, or the whole graph) is one contiguous id range, its nodes grouped by the
// cell solver's degree classes (cell_class of the segment capacity). Without a partition
// the one cell covers every slot; slots past a partition belong to no cell. Computed on
// the host from the capacities.
static int cell_order(EngineImpl& s, int64_t ncap, std::string& err) {
    hipStream_t st = s.stream;
    std::vector<int> capv(ncap);
    if (ncap) KS_CHECK(hipMemcpyAsync(capv.data(), s.capv.p, ncap * sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const size_t k = s.cell_off.size() >= 2 ? s.cell_off.size() - 1 : 1;
    std::vector<int64_t> bound(k + 1, 0);   // slot bounds of each cell
    for (size_t i = 1; i < k; ++i) bound[i] = std::min<int64_t>(ncap, std::max<int64_t>(0, s.cell_off[i]));
    // a partition ends at its last offset: the store's spare slots past it belong to no
    // cell (they take the internal ids after the last cell; no arc can reach them)
    bound[k] = s.cell_off.size() >= 2 ? std::min<int64_t>(ncap, std::max<int64_t>(bound[k - 1], s.cell_off[k])) : ncap;
    std::vector<int> cnt(k * CELL_NCLS, 0);
    std::vector<unsigned char> cls(ncap);
    for (size_t c = 0; c < k; ++c)
        for (int64_t v = bound[c]; v < bound[c + 1]; ++v) {
            cls[v] = (unsigned char)cell_class(capv[v]);
            ++cnt[c * CELL_NCLS + cls[v]];
        }
    s.h_cells.assign(k, CellDesc{});
    std::vector<int> next(k * CELL_NCLS);
    int o = 0, mx = 0;
    for (size_t c = 0; c < k; ++c) {
        const int b = o;
        for (int q = 0; q < CELL_NCLS; ++q) {
            s.h_cells[c].cb[q] = o;
            next[c * CELL_NCLS + q] = o;
            o += cnt[c * CELL_NCLS + q];
        }
        s.h_cells[c].cb[CELL_NCLS] = o;
        mx = std::max(mx, o - b);
    }
    std::vector<int> perm(ncap);
    for (size_t c = 0; c < k; ++c)
        for (int64_t v = bound[c]; v < bound[c + 1]; ++v) perm[v] = next[c * CELL_NCLS + cls[v]]++;
    for (int64_t v = bound[k]; v < ncap; ++v) perm[v] = o++;   // slots past the partition: after the last cell
    if (ncap) KS_CHECK(hipMemcpyAsync(s.perm.p, perm.data(), ncap * sizeof(int), hipMemcpyHostToDevice, st));
    s.cell_max = mx;
    for (int c = 0; c <= NGC; ++c) s.ncls[c] = 0;
    for (int c = 0; c <= NGC; ++c) s.obeg[c] = s.wbeg[c] = 0;
    for (int c = 0; c < NGC; ++c) s.oend[c] = 0;
    s.nheavy = 0;
    s.hub_base = (int)ncap;
    s.nn = (int)ncap;
    const int nn = (int)ncap;
    KS_CHECK(s.cells.ensure(k));
    KS_CHECK(hipMemcpyAsync(s.cells.p, s.h_cells.data(), k * sizeof(CellDesc), hipMemcpyHostToDevice, st));
    KS_CHECK(s.cl_lists.ensure(2 * (size_t)std::max(nn, 1)));
    KS_CHECK(s.cl_rln.ensure(std::max(nn, 1)));
    KS_CHECK(s.cl_rlp.ensure(std::max(nn, 1)));
    KS_CHECK(s.cl_out.ensure(k));
    KS_CHECK(s.cl_bad.ensure(1));
    s.h_cell_out.resize(k);
    return KS_OK;
}

// ------------------------------------------------------------------ build ---
int impl::build(EngineImpl& s, std::string& err) {
    hipStream_t st = s.stream;
    const int hi = s.hi();
    const int64_t spare = s.incremental ? std::max<int64_t>(64, s.nslots / 16) : 0;
    const int64_t ncap = s.nslots + spare;
    s.cells_kept = false;   // positions and internal ids move: every cell runs in the next solve
    int rc = ensure_nodes(s, ncap, err);
    if (rc) return rc;
    s.ncap = ncap;
    s.mult = ncap + 1;
    KS_CHECK(s.deg.ensure(std::max<int64_t>(ncap, 1)));
    KS_CHECK(s.capv.ensure(std::max<int64_t>(ncap, 1)));
    KS_CHECK(s.cls.ensure(std::max<int64_t>(ncap, 1)));
    KS_CHECK(s.perm.ensure(std::max<int64_t>(ncap, 1)));
    for (auto& b : s.cls_list) KS_CHECK(b.ensure(std::max<int64_t>(ncap, 1)));
    KS_CHECK(s.nsel.ensure(NGC + 1));
    KS_CHECK(s.part.ensure(2 * 4096));
    KS_CHECK(hipMemsetAsync(s.deg.p, 0, ncap * sizeof(int), st));
    // 1. degrees → segment capacities → classes
    if (hi)
        hipLaunchKernelGGL(k_degree, dim3(grid_for(hi)), dim3(BLK), 0, st, hi, (const unsigned char*)s.a_alive.p,
                           (const int*)s.a_src.p, (const int*)s.a_dst.p, s.deg.p);
    hipLaunchKernelGGL(k_capacity, dim3(grid_for(ncap)), dim3(BLK), 0, st, (int)ncap, (int)s.nstore,
                       (const int*)s.deg.p, (const unsigned char*)s.n_alive.p, (const unsigned char*)s.n_type.p,
                       s.incremental ? 1 : 0, s.n_hint.p,
                       s.n_grow.p, s.capv.p, s.cls.p);
    if (s.cell_layout) {
        int rc = cell_order(s, ncap, err);   // perm, cell descriptors; no lane-group classes or hubs
        if (rc) return rc;
    } else {
        {
            hipcub::CountingInputIterator<int> it(0);
            size_t tmp = 0, t2 = 0;
            for (unsigned char c = 0; c <= NGC; ++c) {
                KS_CHECK(hipcub::DeviceSelect::If(nullptr, t2, it, s.cls_list[c].p, s.nsel.p + c, (int)ncap,
                                                  ClassIs{s.cls.p, c}, st));
                tmp = std::max(tmp, t2);
            }
            KS_CHECK(s.sel_tmp.ensure(tmp));
            for (unsigned char c = 0; c <= NGC; ++c) {
                t2 = tmp;
                KS_CHECK(hipcub::DeviceSelect::If(s.sel_tmp.p, t2, it, s.cls_list[c].p, s.nsel.p + c, (int)ncap,
                                                  ClassIs{s.cls.p, c}, st));
            }
        }
        KS_CHECK(hipMemcpyAsync(s.ncls, s.nsel.p, (NGC + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        s.nheavy = s.ncls[NGC];
        // 2. internal ids: classes in order, each padded to whole 64-node blocks, hubs last
        {
            int o = 0, wv = 0;
            for (int c = 0; c < NGC; ++c) {
                s.obeg[c] = o;
                s.oend[c] = o + s.ncls[c];
                s.wbeg[c] = wv;
                const int pad = (s.ncls[c] + 63) / 64 * 64;
                o += pad;
                wv += pad / win_slots(c);
            }
            s.obeg[NGC] = o;
            s.wbeg[NGC] = wv;
            s.hub_base = o;
            s.nn = o + s.nheavy;
        }
        for (int c = 0; c <= NGC; ++c)
            if (s.ncls[c])
                hipLaunchKernelGGL(k_make_perm, dim3(grid_for(s.ncls[c])), dim3(BLK), 0, st, s.ncls[c],
                                   c < NGC ? s.obeg[c] : s.hub_base, (const int*)s.cls_list[c].p, s.perm.p);
    }
    const int nn = s.nn;
    KS_CHECK(s.capi.ensure(nn + 1));
    KS_CHECK(s.iperm.ensure(nn + 1));
    KS_CHECK(s.first.ensure(nn + 1));
    KS_CHECK(s.used.ensure(std::max(nn, 1)));
    KS_CHECK(s.scur.ensure(std::max(nn, 1)));
    KS_CHECK(hipMemsetAsync(s.scur.p, 0, std::max(nn, 1) * sizeof(int), st));
    KS_CHECK(s.rs.ensure(nn + 1));
    KS_CHECK(hipMemsetAsync(s.capi.p, 0, (nn + 1) * sizeof(int), st));
    KS_CHECK(hipMemsetAsync(s.iperm.p, 0xff, (nn + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_capi, dim3(grid_for(ncap)), dim3(BLK), 0, st, (int)ncap, (const int*)s.perm.p,
                       (const int*)s.capv.p, s.capi.p, s.iperm.p);
    {   // first = exclusive scan of the capacities (nn + 1 entries: first[nn] = Σ)
        size_t t = 0;
        KS_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t, s.capi.p, s.first.p, nn + 1, st));
        KS_CHECK(s.sort_tmp.ensure(std::max<size_t>(t, s.sort_tmp.n)));
        t = s.sort_tmp.n;
        KS_CHECK(hipcub::DeviceScan::ExclusiveSum(s.sort_tmp.p, t, s.capi.p, s.first.p, nn + 1, st));
    }
    int m2c = 0;
    KS_CHECK(hipMemcpyAsync(&m2c, s.first.p + nn, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    s.m2cap = m2c;
    const int64_t m2cap = std::max<int64_t>(m2c, 1);
    KS_CHECK(s.pos.ensure(m2cap));
    KS_CHECK(s.ent.ensure(m2cap));
    KS_CHECK(s.excess.ensure(std::max(nn, 1)));
    KS_CHECK(s.nd.ensure(4 * (size_t)std::max(nn, 1)));
    if (nn)
        hipLaunchKernelGGL(k_node_bounds, dim3(grid_for(nn)), dim3(BLK), 0, st, nn, (const int*)s.first.p, s.nd.p);
    if (m2c)
        hipLaunchKernelGGL(k_inert_all, dim3(grid_for(m2c)), dim3(BLK), 0, st, (long long)m2c, nn,
                           (const int*)s.first.p, s.pos.p, s.ent.p);
    // 3. live arcs into their segments, ordered by tail (radix sort of 2·hi keys)
    const int64_t m2 = 2 * (int64_t)hi;
    if (s.acap) KS_CHECK(hipMemsetAsync(s.fwd.p, 0xff, s.acap * sizeof(int), st));
    if (m2) {
        KS_CHECK(s.keys_in.ensure(m2));
        KS_CHECK(s.keys_out.ensure(m2));
        KS_CHECK(s.vals_in.ensure(m2));
        KS_CHECK(s.vals_out.ensure(m2));
        KS_CHECK(s.pos_of.ensure(m2));
        int bits = 1;
        while ((1LL << bits) <= nn + 1) ++bits;
        hipLaunchKernelGGL(k_pos_keys, dim3(grid_for(hi)), dim3(BLK), 0, st, hi, nn,
                           (const unsigned char*)s.a_alive.p, (const int*)s.a_src.p, (const int*)s.a_dst.p,
                           (const int*)s.perm.p, s.keys_in.p, s.vals_in.p);
        size_t t = 0;
        KS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t, s.keys_in.p, s.keys_out.p, s.vals_in.p,
                                                    s.vals_out.p, (int)m2, 0, bits, st));
        KS_CHECK(s.sort_tmp.ensure(std::max<size_t>(t, s.sort_tmp.n)));
        t = s.sort_tmp.n;
        KS_CHECK(hipcub::DeviceRadixSort::SortPairs(s.sort_tmp.p, t, s.keys_in.p, s.keys_out.p, s.vals_in.p,
                                                    s.vals_out.p, (int)m2, 0, bits, st));
        hipLaunchKernelGGL(k_first, dim3(grid_for(nn + 1)), dim3(BLK), 0, st, nn, (long long)m2,
                           (const unsigned*)s.keys_out.p, s.rs.p);
        hipLaunchKernelGGL(k_fill_csr, dim3(grid_for(m2)), dim3(BLK), 0, st, (long long)m2, nn,
                           (const unsigned*)s.keys_out.p, (const int*)s.vals_out.p, (const int*)s.rs.p,
                           (const int*)s.first.p, (const int*)s.perm.p, (const int*)s.a_src.p, (const int*)s.a_dst.p,
                           (const long long*)s.a_low.p, (const long long*)s.a_cap.p, (const long long*)s.a_cost.p,
                           s.mult, s.pos.p, s.ent.p, s.fwd.p, s.pos_of.p);
        hipLaunchKernelGGL(k_fill_rev, dim3(grid_for(m2)), dim3(BLK), 0, st, (long long)m2, nn,
                           (const unsigned*)s.keys_out.p, (const int*)s.vals_out.p, (const int*)s.pos_of.p, s.pos.p);
        hipLaunchKernelGGL(k_used, dim3(grid_for(nn)), dim3(BLK), 0, st, nn, (const int*)s.rs.p, s.used.p);
    } else {
        KS_CHECK(hipMemsetAsync(s.used.p, 0, std::max(nn, 1) * sizeof(int), st));
    }
    // 4. hub chunk table and the chunked class's 64-arc chunks (from the segments)
    {
        std::vector<int> hf(s.nheavy + 1);
        if (s.nheavy) {
            KS_CHECK(hipMemcpyAsync(hf.data(), s.first.p + s.hub_base, (s.nheavy + 1) * sizeof(int),
                                    hipMemcpyDeviceToHost, st));
            KS_CHECK(hipStreamSynchronize(st));
        }
        std::vector<HItem> items;
        std::vector<int> nch(s.nheavy);
        for (int h = 0; h < s.nheavy; ++h) {
            int c = 0;
            for (int b = hf[h]; b < hf[h + 1]; b += CHUNK, ++c)
                items.push_back(HItem{s.hub_base + h, h, b, std::min(b + CHUNK, hf[h + 1])});
            nch[h] = c;
        }
        s.nhitems = (int)items.size();
        KS_CHECK(s.hitems.ensure(items.size()));
        KS_CHECK(s.hnchunks.ensure(s.nheavy));
        KS_CHECK(s.inbox.ensure((size_t)s.nheavy * SHARDS));
        KS_CHECK(s.flags.ensure(6 * (size_t)std::max(1, s.hub_base)));
        KS_CHECK(s.fl.ensure(3 * ((size_t)std::max(1, s.nn) + 4096)));
        KS_CHECK(s.hubflags.ensure(6 * (size_t)std::max(1, s.nheavy)));
        KS_CHECK(hipMemsetAsync(s.flags.p, 0, 6 * (size_t)std::max(1, s.hub_base), st));
        KS_CHECK(hipMemsetAsync(s.hubflags.p, 0, 6 * (size_t)std::max(1, s.nheavy) * sizeof(int), st));
        if (s.nheavy) {
            KS_CHECK(hipMemcpyAsync(s.hitems.p, items.data(), items.size() * sizeof(HItem), hipMemcpyHostToDevice, st));
            KS_CHECK(hipMemcpyAsync(s.hnchunks.p, nch.data(), nch.size() * sizeof(int), hipMemcpyHostToDevice, st));
            KS_CHECK(hipMemsetAsync(s.inbox.p, 0, (size_t)s.nheavy * SHARDS * sizeof(long long), st));
        }
        const int c0 = s.obeg[CCLS], cn = s.ncls[CCLS];
        std::vector<int> cf(cn + 1);
        if (cn) KS_CHECK(hipMemcpyAsync(cf.data(), s.first.p + c0, (cn + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        std::vector<CItem> ci;
        for (int k = 0; k < cn; ++k)
            for (int b = cf[k]; b < cf[k + 1]; b += 64)
                ci.push_back(CItem{c0 + k, b, std::min(b + 64, cf[k + 1]), b == cf[k] ? 1 : 0});
        s.ncitems = (int)ci.size();
        KS_CHECK(s.citems.ensure(std::max<size_t>(1, ci.size())));
        if (!ci.empty())
            KS_CHECK(hipMemcpyAsync(s.citems.p, ci.data(), ci.size() * sizeof(CItem), hipMemcpyHostToDevice, st));
        const int nq = std::max(1, s.nheavy);
        KS_CHECK(s.q_req.ensure(nq));
        KS_CHECK(s.aug_req.ensure(nq));
        KS_CHECK(hipMemsetAsync(s.aug_req.p, 0, nq * sizeof(long long), st));
        KS_CHECK(s.q_taken.ensure(nq));
        KS_CHECK(s.q_min.ensure(nq));
        KS_CHECK(s.q_unsat.ensure(nq));
        KS_CHECK(s.q_arrive.ensure(nq));
        std::vector<long long> qm(nq, INF64);
        KS_CHECK(hipMemcpyAsync(s.q_min.p, qm.data(), nq * sizeof(long long), hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemsetAsync(s.q_req.p, 0, nq * sizeof(long long), st));
        KS_CHECK(hipMemsetAsync(s.q_taken.p, 0, nq * sizeof(long long), st));
        KS_CHECK(hipMemsetAsync(s.q_unsat.p, 0, nq * sizeof(int), st));
        KS_CHECK(hipMemsetAsync(s.q_arrive.p, 0, nq * sizeof(int), st));
        KS_CHECK(hipStreamSynchronize(st));
    }
    s.csr_valid = true;
    ++s.rebuilds;
    return KS_OK;
}

// zero flow, supplies with the lower-bound transform, zero prices
int impl::cold_reset(EngineImpl& s, std::string& err) {
    hipStream_t st = s.stream;
    const int hi = s.hi();
    if (s.m2cap)
        hipLaunchKernelGGL(k_reset_pos, dim3(grid_for(s.m2cap)), dim3(BLK), 0, st, (long long)s.m2cap,
                           (const int*)s.ent.p, s.pos.p);
    hipLaunchKernelGGL(k_reset_nodes, dim3(grid_for(s.nn)), dim3(BLK), 0, st, s.nn, (int)s.ncap,
                       (const int*)s.iperm.p, (const unsigned char*)s.n_alive.p, (const long long*)s.n_supply.p,
                       s.excess.p, s.nd.p, (s.nd.p + 2));
    if (hi)
        hipLaunchKernelGGL(k_reset_low, dim3(grid_for(hi)), dim3(BLK), 0, st, hi, (const unsigned char*)s.a_alive.p,
                           (const int*)s.a_src.p, (const int*)s.a_dst.p, (const int*)s.perm.p,
                           (const long long*)s.a_low.p, s.excess.p);
    KS_CHECK(hipGetLastError());
    return KS_OK;
}

}  // namespace ks
