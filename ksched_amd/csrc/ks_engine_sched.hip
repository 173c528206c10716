// ks_engine_sched.hip — the engine's scheduler glue: bindings, scheduling deltas,
// unscheduled costs, topology statistics, ks_commit_schedule and ks_commit_preemptive,
// ks_remove_resources, ks_complete_tasks, ks_add_tasks, ks_add_resources, ks_update_tasks,
// ks_update_nodes and ks_get_bindings. It launches the kernels of ks_sched.hip and ks_store.hip through their
// launchers, none of the engine's.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ks_engine_impl.h"

namespace ks {

namespace {
struct NonZero {
    __host__ __device__ int operator()(int x) const { return x != 0; }
};
// ks_update_nodes: an arc slot whose flag carries a record (NOD_RECORD, NOD_UNLISTED).
struct NodRecord {
    __host__ __device__ int operator()(int x) const { return x >= NOD_RECORD; }
};

// out[i] = in[0] + … + in[i − 1] for i < n, on st; hipcub's scratch is map_tmp.
template <typename In>
hipError_t exclusive_sum(EngineImpl& s, In in, int* out, int64_t n, hipStream_t st) {
    size_t t = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, t, in, out, (int)n, st);
    if (e == hipSuccess) e = s.map_tmp.ensure(std::max(t, s.map_tmp.n));
    t = s.map_tmp.n;
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(s.map_tmp.p, t, in, out, (int)n, st);
    return e;
}

// Bump-pointer carve of one buffer: a pass over base == nullptr sizes it (n), the same
// statements over the allocation hand out the arrays.
template <typename T>
struct Carve {
    T* base;
    int64_t n = 0;
    T* take(int64_t len) {
        T* p = base ? base + n : nullptr;
        n += len;
        return p;
    }
};

// The scratch of a delta call (the commit's buffers): carve(ci, cu), the call's own part, takes its
// int arrays from cm_i and its u64 arrays from cm_u; it runs twice, to size and to hand out.
// cm_i starts zeroed, cm_u in its first zero_u words (kAllU64: all of it), and with flags the
// flag bytes per node slot, cm_b, too.
constexpr int64_t kAllU64 = -1;
template <class F>
int carve_scratch(EngineImpl& s, F&& carve, int64_t zero_u, bool flags, std::string& err) {
    hipStream_t st = s.stream;
    Carve<int> ci{nullptr};
    Carve<unsigned long long> cu{nullptr};
    carve(ci, cu);
    const int64_t n_i = ci.n, n_u = cu.n;
    const int64_t nb = (s.nstore + 4) & ~3LL;   // byte flags, word-aligned for the atomics
    KS_CHECK(s.cm_i.ensure(n_i));
    KS_CHECK(s.cm_u.ensure(n_u));
    if (flags) KS_CHECK(s.cm_b.ensure(nb));
    ci = {s.cm_i.p};
    cu = {s.cm_u.p};
    carve(ci, cu);
    KS_CHECK(hipMemsetAsync(s.cm_i.p, 0, n_i * sizeof(int), st));
    KS_CHECK(hipMemsetAsync(s.cm_u.p, 0, (zero_u == kAllU64 ? n_u : zero_u) * 8, st));
    if (flags) KS_CHECK(hipMemsetAsync(s.cm_b.p, 0, nb, st));
    return KS_OK;
}

// A call's control word, zeroed on st.
template <typename C>
hipError_t clear_ctl(DBuf<C>& ctl, hipStream_t st) {
    const hipError_t e = ctl.ensure(1);
    return e == hipSuccess ? hipMemsetAsync(ctl.p, 0, sizeof(C), st) : e;
}

// The store's (src, dst) index as a call's kernels read it.
template <typename Dev>
void wire_hash(const EngineImpl& s, Dev& d) {
    d.hkey = s.hkey.p;
    d.hval = s.hval.p;
    d.hmask = s.hcap ? (int)(s.hcap - 1) : -1;
}

// A stale residual CSR is rebuilt from the table (the solution in place goes with it).
int fresh_csr(EngineImpl& s, std::string& err) {
    if (s.csr_valid) return KS_OK;
    const int rc = build(s, err);
    if (rc) return rc;
    s.has_prev = false;
    s.solved = false;
    return KS_OK;
}

int check_agg_ids(const EngineImpl& s, const uint64_t* ids, size_t k, std::string& err) {
    for (size_t i = 0; ids && i < k; ++i)
        if (ids[i] == 0 || (int64_t)ids[i] > s.nstore) {
            err = "unscheduled aggregator id beyond the graph";
            return KS_E_INVALID;
        }
    return KS_OK;
}

// The capacity passes climb from one sink, or, over a cell partition, from every cell's own.
int check_one_sink(const EngineImpl& s, bool caps, int64_t sink_slot, std::string& err) {
    const bool every_sink = sink_slot == Engine::kEverySink && s.cell_off.size() >= 2;
    if (caps && !every_sink && (sink_slot < 0 || sink_slot >= s.ncap)) {
        err = "resource capacities need exactly one sink";
        return KS_E_INVALID;
    }
    return KS_OK;
}

// A refusal's control word holds count − index of the first offender in input order (the kernels
// keep the largest), 0 when there is none: → its index, n for none; false: no such word.
bool first_bad(int word, size_t n, size_t* idx) {
    if (word < 0 || (size_t)word > n) return false;
    *idx = n - (size_t)word;
    return true;
}

// A union's sinks for the aggregator records of an arrival or a refresh and for the new PUs of a
// growth (sink_slot == kEverySink over a cell partition): the table is rebuilt on every call, one
// pass over the slot bytes.
template <class Dev>
int wire_cell_sinks(EngineImpl& s, const SchedDev& d, Dev& a, int64_t sink_slot, std::string& err) {
    if (sink_slot != Engine::kEverySink || s.cell_off.size() < 2) return KS_OK;
    const int ncells = (int)s.cell_off.size() - 1;
    if (int rc = ensure_cell_first(s, err)) return rc;
    KS_CHECK(s.cell_sink.ensure(ncells));
    KS_CHECK(hipMemsetAsync(s.cell_sink.p, 0xff, ncells * sizeof(int), s.stream));
    KS_CHECK(sched_cell_sinks(d, a.nst, s.cell_first.p, ncells, s.cell_sink.p, s.stream));
    a.cell_sink = s.cell_sink.p;
    a.cell_first = s.cell_first.p;
    a.ncells = ncells;
    return KS_OK;
}

// A batch call's heads leave their graphs' numbering on the device (d_goff, d_base: ng + 1 words
// each; Arc: ks_task_arc or ks_node_arc; bad_range: that word of the call's control struct).
template <class Arc>
int translate_heads(EngineImpl& s, const BatchView& bv, unsigned long long* d_goff, unsigned long long* d_base,
                    unsigned long long* d_arcs, size_t na, int* bad_range, std::string& err) {
    KS_CHECK(hipMemcpyAsync(d_goff, bv.arc_goff, (bv.ng + 1) * 8, hipMemcpyHostToDevice, s.stream));
    KS_CHECK(hipMemcpyAsync(d_base, bv.off, (bv.ng + 1) * 8, hipMemcpyHostToDevice, s.stream));
    KS_CHECK(sched_translate_heads((Arc*)d_arcs, (int)na, d_goff, (const long long*)d_base, (int)bv.ng, bad_range,
                                   s.stream));
    return KS_OK;
}

// What every range refusal of a batch call ends with (span: the ids of the offender's graph).
std::string outside_ids_tail(int64_t span) {
    return " is outside the graph's ids 1.." + std::to_string(span) + " (its highest id at the load plus the reserved ids)";
}

// The refusal of a head outside its graph's ids (word: the control struct's bad_range; what: the
// noun of the k listed ids, "task" or "node"; the host's arcs are still graph-local: the device
// translated its own copy).
template <class Arc>
int range_refusal(const BatchView& bv, int word, const char* what, const uint64_t* ids, const uint64_t* arc_off,
                  size_t k, const Arc* arcs, size_t na, std::string& err) {
    size_t j;
    if (!first_bad(word, na, &j) || j >= na) {
        err = "inconsistent arc index";
        return KS_E_DEVICE;
    }
    const size_t g = (size_t)(std::upper_bound(bv.arc_goff, bv.arc_goff + bv.ng, (uint64_t)j) - bv.arc_goff) - 1;
    const size_t i = (size_t)(std::upper_bound(arc_off, arc_off + k, (uint64_t)j) - arc_off) - 1;
    err = id_name(&bv, what, ids[i]) + ": head " + std::to_string(arcs[j].dst) + outside_ids_tail(bv.off[g + 1] - bv.off[g]);
    return KS_E_RANGE;
}

// The refusal of a gaining aggregator whose cell has no single sink (word: AddCtl::bad_sink).
int sink_refusal(const BatchView* bv, int word, int64_t nst, std::string& err) {
    size_t v;
    if (!first_bad(word, (size_t)nst, &v)) {
        err = "inconsistent aggregator slot";
        return KS_E_DEVICE;
    }
    err = id_name(bv, "unscheduled aggregator", (uint64_t)v + 1) + " gains a unit, and its cell has no sink or several: "
          "the capacity of its arc into the sink needs exactly one";
    return KS_E_INVALID;
}

double ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// Level 0 of the topology BFS over a cell partition: every live sink, one per cell. A
// union's sinks are few (one per graph) and far apart in slot space, so each is its
// own returning atomic on the frontier's counter (nothing to aggregate per wave). With
// one sink the frontier is that sink alone, as the single-graph seed writes it.
__global__ void k_seed_sinks(int ncap, const unsigned char* __restrict__ alive, const unsigned char* __restrict__ type,
                             const int* __restrict__ perm, int* __restrict__ lvl, int* __restrict__ front,
                             int* __restrict__ nfront) {
    for (long long v = blockIdx.x * (long long)BLK + threadIdx.x; v < ncap; v += (long long)gridDim.x * BLK)
        if (alive[v] && type[v] == KS_NODE_SINK) {
            const int x = perm[v];
            lvl[x] = 0;
            front[atomicAdd(nfront, 1)] = x;
        }
}
}  // namespace

uint64_t BatchView::base_of(uint64_t id) const {
    // graph i owns the ids (off[i], off[i + 1]]
    size_t i = (size_t)(std::lower_bound(off, off + ng + 1, (int64_t)id) - off);
    i = i ? i - 1 : 0;
    return (uint64_t)off[std::min(i, ng ? ng - 1 : 0)];
}

std::string id_name(const BatchView* bv, const char* what, uint64_t id) {
    if (!bv || !bv->ng) return std::string(what) + " " + std::to_string(id);
    size_t i = (size_t)(std::lower_bound(bv->off, bv->off + bv->ng + 1, (int64_t)id) - bv->off);
    i = std::min(i ? i - 1 : 0, bv->ng - 1);
    return "graph " + std::to_string(bv->graph[i]) + ": " + what + " " + std::to_string(id - (uint64_t)bv->off[i]);
}

// ------------------------------------------------- scheduler-side sweeps ---
int Engine::set_bindings(const uint64_t* task, const uint64_t* pu, size_t k, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    if (!k) return KS_OK;
    std::vector<unsigned long long> ids(task, task + k), vals(pu, pu + k);
    for (size_t i = 0; i < k; ++i)
        if (ids[i] == 0 || (int64_t)ids[i] > s.nstore) {
            err = "binding for a task id beyond the graph";
            return KS_E_INVALID;
        }
    KS_CHECK(s.sched_u.ensure(2 * k));
    hipStream_t st = s.stream;
    KS_CHECK(hipMemcpyAsync(s.sched_u.p, ids.data(), k * 8, hipMemcpyHostToDevice, st));
    KS_CHECK(hipMemcpyAsync(s.sched_u.p + k, vals.data(), k * 8, hipMemcpyHostToDevice, st));
    // the same scatter as the running counts: n_bind[id − 1] = pu
    KS_CHECK(sched_running_counts(s.schd(), s.sched_u.p, s.sched_u.p + k, (int)k, s.n_bind.p, st));
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

int Engine::sched_deltas(int commit, std::vector<ks_sched_delta>* out, size_t* count, int64_t n_tasks,
                         std::string& err) {
    EngineImpl& s = *p_;
    if (!s.solved) {
        err = "no successful solve";
        return KS_E_INVALID;
    }
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    uint64_t* dense = nullptr;
    size_t nt = 0;
    int rc = scratch(&dense, std::max<int64_t>(n_tasks, 1), err);
    if (rc == KS_OK) rc = task_pu(n_tasks ? dense : nullptr, n_tasks, &nt, n_tasks, err);   // also is_task / rank
    if (rc) return rc;
    const int64_t ncap = s.ncap;
    if (!n_tasks) {   // no tasks: map arrays were not built; every binding is a preemption
        KS_CHECK(s.map_is_task.ensure(ncap + 1));
        KS_CHECK(s.map_rank.ensure(ncap + 1));
        KS_CHECK(hipMemsetAsync(s.map_is_task.p, 0, (ncap + 1) * sizeof(int), st));
        KS_CHECK(hipMemsetAsync(s.map_rank.p, 0, (ncap + 1) * sizeof(int), st));
    }
    KS_CHECK(s.sched_i.ensure(4 * (ncap + 1) + 4));
    int* pre = s.sched_i.p;
    int* other = pre + (ncap + 1);
    int* pre_pos = other + (ncap + 1);
    int* other_pos = pre_pos + (ncap + 1);
    int* bad = other_pos + (ncap + 1);
    KS_CHECK(hipMemsetAsync(bad, 0, 4 * sizeof(int), st));
    const SchedDev d = s.schd();
    KS_CHECK(sched_delta_kinds(d, s.map_is_task.p, s.map_rank.p, (const unsigned long long*)dense, pre, other, bad, st));
    KS_CHECK(exclusive_sum(s, (const int*)pre, pre_pos, ncap + 1, st));
    // (other holds the kind, 1 PLACE or 2 MIGRATE: each counts as one delta)
    hipcub::TransformInputIterator<int, NonZero, const int*> is_other(other, NonZero());
    KS_CHECK(exclusive_sum(s, is_other, other_pos, ncap + 1, st));
    int h[3] = {0, 0, 0};
    KS_CHECK(hipMemcpyAsync(&h[0], pre_pos + ncap, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipMemcpyAsync(&h[1], other_pos + ncap, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipMemcpyAsync(&h[2], bad, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    if (h[2]) {
        err = "mapping names a destination that is not a PU (graph_manager.go:259-262)";
        return KS_E_VERIFY;
    }
    const int npre = h[0], noth = h[1];
    *count = (size_t)(npre + noth);
    if (!out) return KS_OK;
    KS_CHECK(s.sched_d.ensure(std::max(1, npre + noth)));
    KS_CHECK(sched_delta_emit(d, s.map_rank.p, (const unsigned long long*)dense, pre, pre_pos, other, other_pos, npre,
                              s.sched_d.p, commit, st));
    out->resize(npre + noth);
    if (npre + noth)
        KS_CHECK(hipMemcpyAsync(out->data(), s.sched_d.p, (npre + noth) * sizeof(ks_sched_delta), hipMemcpyDeviceToHost,
                                st));
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

int Engine::unsched_costs(const uint64_t* ids, size_t k, int mode, int64_t ucost, int64_t ccost, size_t* changed,
                          std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const int64_t nb = (s.nstore + 4) & ~3LL;   // byte flags, word-aligned for the atomics
    KS_CHECK(s.sched_b.ensure(nb));
    KS_CHECK(s.sched_i.ensure(4));
    KS_CHECK(hipMemsetAsync(s.sched_b.p, 0, nb, st));
    KS_CHECK(hipMemsetAsync(s.sched_i.p, 0, sizeof(int), st));
    const unsigned long long* dids = nullptr;
    if (ids && k) {
        if (int rc = check_agg_ids(s, ids, k, err)) return rc;
        KS_CHECK(s.sched_u.ensure(k));
        KS_CHECK(hipMemcpyAsync(s.sched_u.p, ids, k * 8, hipMemcpyHostToDevice, st));
        dids = s.sched_u.p;
    }
    KS_CHECK(sched_unsched_costs(s.schd(), ids ? dids : nullptr, (int)k, s.sched_b.p, mode, ucost, ccost, s.sched_i.p,
                                 st));
    int h = 0;
    KS_CHECK(hipMemcpyAsync(&h, s.sched_i.p, sizeof(int), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    if (changed) *changed = (size_t)h;
    if (h) {
        s.solved = false;
        s.cells_kept = false;   // costs changed in place, past the dirty flags: every cell runs next
    }
    return KS_OK;
}

// The level-synchronous BFS of ComputeTopologyStatistics from the sink (slot sink_slot <
// ncap) over the residual CSR's in-arcs; slots / run (per node slot) start zeroed.
// Uses sched_i.
static int topo_bfs(EngineImpl& s, const SchedDev& d, int64_t sink_slot, uint64_t mtpp,
                    const unsigned long long* pu_slots, const unsigned long long* cnt, unsigned long long* slots,
                    unsigned long long* run, std::string& err) {
    hipStream_t st = s.stream;
    const int64_t nn = s.nn;
    KS_CHECK(s.sched_i.ensure(3 * (nn + 1) + 2));
    int* lvl = s.sched_i.p;
    int* fa = lvl + (nn + 1);
    int* fb = fa + (nn + 1);
    int* nnext = fb + (nn + 1);
    KS_CHECK(hipMemsetAsync(lvl, 0xff, (nn + 1) * sizeof(int), st));
    int nfront = 1;
    if (sink_slot == Engine::kEverySink) {   // a partition: every live sink at level 0
        KS_CHECK(hipMemsetAsync(nnext, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_seed_sinks, dim3(grid_for(s.ncap, 1024)), dim3(BLK), 0, st, (int)s.ncap,
                           (const unsigned char*)s.n_alive.p, (const unsigned char*)s.n_type.p, (const int*)s.perm.p,
                           lvl, fa, nnext);
        KS_CHECK(hipGetLastError());
        KS_CHECK(hipMemcpyAsync(&nfront, nnext, sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
    } else {
        int sink_x = 0;
        KS_CHECK(hipMemcpyAsync(&sink_x, s.perm.p + sink_slot, sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        const int zero = 0;
        KS_CHECK(hipMemcpyAsync(lvl + sink_x, &zero, sizeof(int), hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(fa, &sink_x, sizeof(int), hipMemcpyHostToDevice, st));
    }
    for (int level = 0; nfront > 0 && level <= nn; ++level) {
        KS_CHECK(hipMemsetAsync(nnext, 0, sizeof(int), st));
        KS_CHECK(sched_topo_level(d, fa, nfront, level, lvl, fb, nnext, mtpp, pu_slots, cnt, slots, run, st));
        KS_CHECK(hipMemcpyAsync(&nfront, nnext, sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        std::swap(fa, fb);
    }
    return KS_OK;
}

int Engine::topology_stats(uint64_t mtpp, const uint64_t* pu_ids, const uint64_t* pu_running, size_t k,
                           int64_t sink_slot, uint64_t* slots_below, uint64_t* running_below, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    if (int rc = fresh_csr(s, err)) return rc;   // the BFS walks the residual CSR's in-arcs
    const int64_t ncap = s.ncap;
    if (sink_slot < 0 || sink_slot >= ncap || ncap == 0) {
        std::memset(slots_below, 0, s.nslots * sizeof(uint64_t));
        std::memset(running_below, 0, s.nslots * sizeof(uint64_t));
        return KS_OK;
    }
    KS_CHECK(s.sched_u.ensure(3 * (ncap + 1) + 2 * k));
    unsigned long long* cnt = s.sched_u.p;
    unsigned long long* slots = cnt + (ncap + 1);
    unsigned long long* run = slots + (ncap + 1);
    unsigned long long* kid = run + (ncap + 1);
    KS_CHECK(hipMemsetAsync(cnt, 0, 3 * (ncap + 1) * 8, st));
    if (pu_ids && k) {
        for (size_t i = 0; i < k; ++i)
            if (pu_ids[i] == 0 || (int64_t)pu_ids[i] > ncap) {
                err = "PU id beyond the graph";
                return KS_E_INVALID;
            }
        KS_CHECK(hipMemcpyAsync(kid, pu_ids, k * 8, hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(kid + k, pu_running, k * 8, hipMemcpyHostToDevice, st));
    }
    const SchedDev d = s.schd();
    KS_CHECK(sched_running_counts(d, pu_ids ? kid : nullptr, kid + k, (int)k, cnt, st));
    int rc = topo_bfs(s, d, sink_slot, mtpp, nullptr, cnt, slots, run, err);
    if (rc) return rc;
    const int64_t n = std::min<int64_t>(s.nslots, ncap);
    if (n) {
        KS_CHECK(hipMemcpyAsync(slots_below, slots, n * 8, hipMemcpyDeviceToHost, st));
        KS_CHECK(hipMemcpyAsync(running_below, run, n * 8, hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
    }
    return KS_OK;
}


// ks_commit_schedule and ks_commit_preemptive: the deltas of the last solve, then the
// records of their graph edit generated in d_recs and applied by store_apply with no node
// edit. Pinned mode (preempt == false; all deltas must be PLACEs): the pin, aggregator and
// resource-capacity records. Preemptive mode: the running-arc, delete, preemption-cost
// (pcost) and resource-capacity records of every delta. Two host syncs beside the deltas'
// own and the BFS levels': the record counts (CommitCtl → *h, one copy) and the store's
// counters. *dirty: the device state may have changed (a failure after that leaves it unknown).
int Engine::commit(bool preempt, int flags, int64_t ccost, int64_t pcost, const uint64_t* ids, size_t k,
                   int64_t sink_slot, int64_t n_tasks, size_t cap, std::vector<ks_sched_delta>* out, size_t* count,
                   CommitCtl* hc, bool* dirty, std::string& err) {
    EngineImpl& s = *p_;
    *dirty = false;
    if (!s.solved || !s.csr_valid) {
        err = "no successful solve";
        return KS_E_INVALID;
    }
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const bool log = s.opts.log_cycles != 0;   // (ks_opts.log_cycles: where a commit's time goes)
    const auto t0 = std::chrono::steady_clock::now();
    int rc = sched_deltas(0, out, count, n_tasks, err);   // leaves the kinds and their scan in sched_i
    if (rc) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    if (log) KS_CHECK(hipEventRecord(s.kev[0], st));
    if (cap < out->size()) {
        err = "output buffer smaller than the delta count";
        return KS_E_INVALID;
    }
    int npre = 0;   // (the PREEMPTs come first)
    for (const ks_sched_delta& x : *out) {
        if (x.type != KS_DELTA_PLACE && !preempt) {
            err = "the solve preempts or migrates task " + std::to_string(x.task) +
                  ": ks_commit_schedule pins placements only (no preemption mode)";
            return KS_E_INVALID;
        }
        npre += x.type == KS_DELTA_PREEMPT;
    }
    const int64_t ncap = s.ncap, nst = s.nstore;
    const int hi = s.hi();
    const int64_t np = (int64_t)out->size();
    CommitDev c{};
    c.preempt = preempt ? 1 : 0;
    c.resource_caps = (flags & KS_COMMIT_RESOURCE_CAPS) ? 1 : 0;
    c.ccost = ccost;
    c.pcost = pcost;
    c.np = (int)np;
    c.ni_max = (int)(np + s.m2cap / 64 + 1);
    rc = check_one_sink(s, c.resource_caps, sink_slot, err);
    if (rc) return rc;
    // scratch: int arrays per item, chunk item and arc slot in cm_i; counters per node slot
    // and the aggregator ids in cm_u; flags per node slot in cm_b
    unsigned long long* idbuf = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        for (int** a : {&c.pl_task, &c.pl_kind, &c.pl_pu, &c.pl_old, &c.pl_has, &c.pl_found, &c.pl_noarc, &c.add_off,
                        &c.nch, &c.ch_off})
            *a = ci.take(np + 1);
        for (int** a : {&c.icnt, &c.i_off}) *a = ci.take(c.ni_max + 1);
        for (int** a : {&c.aflag, &c.a_off}) *a = ci.take((int64_t)hi + 1);
        for (unsigned long long** a : {&c.agg_cnt, &c.pu_slots, &c.pu_run, &c.slots, &c.running}) *a = cu.take(nst + 1);
        idbuf = cu.take(k);
    }, kAllU64, true, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.cm_ctl, st));
    c.fl = s.cm_b.p;
    c.ctl = s.cm_ctl.p;
    rc = check_agg_ids(s, ids, k, err);
    if (rc) return rc;
    if (ids && k) KS_CHECK(hipMemcpyAsync(idbuf, ids, k * 8, hipMemcpyHostToDevice, st));
    const unsigned long long* dids = ids ? idbuf : nullptr;
    SchedDev d = s.schd();
    {   // the kinds of sched_deltas: [pre | other | pre_pos | other_pos] × (ncap + 1)
        const int* pre = s.sched_i.p;
        const int* other = pre + (ncap + 1);
        const int* pre_pos = other + (ncap + 1);
        const int* other_pos = pre_pos + (ncap + 1);
        const unsigned long long* newpu = (const unsigned long long*)s.map_scratch.p;
        KS_CHECK(sched_commit_items(d, c, s.map_rank.p, newpu, pre, pre_pos, other, other_pos, npre, dids, (int)k, st));
    }
    KS_CHECK(exclusive_sum(s, (const int*)c.nch, c.ch_off, np + 1, st));
    KS_CHECK(sched_commit_count(d, c, st));
    KS_CHECK(exclusive_sum(s, (const int*)c.icnt, c.i_off, c.ni_max + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)c.pl_noarc, c.add_off, np + 1, st));
    if (c.resource_caps) {
        KS_CHECK(sched_commit_pu(d, c, st));
        rc = topo_bfs(s, d, sink_slot, 0, c.pu_slots, c.pu_run, c.slots, c.running, err);
        if (rc) return rc;
    }
    KS_CHECK(sched_commit_arc_flags(d, c, st));
    KS_CHECK(exclusive_sum(s, (const int*)c.aflag, c.a_off, (int64_t)hi + 1, st));
    KS_CHECK(sched_commit_totals(d, c, st));
    CommitCtl& h = *hc;
    KS_CHECK(hipMemcpyAsync(&h, c.ctl, sizeof(CommitCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    if (h.bad & 2) {
        err = "a preempted or migrated task has no running arc into the PU it leaves (graph_manager.go:416-419)";
        return KS_E_VERIFY;
    }
    if (h.bad) {
        err = "a capacity would fall below its arc's lower bound";
        return KS_E_VERIFY;
    }
    const int64_t nrec = (int64_t)h.rec_pin + h.rec_add + h.rec_arc;
    if (h.rec_pin < 0 || h.rec_add < 0 || h.rec_add > np || h.rec_arc < 0 || h.rec_arc > hi ||
        h.rec_pin > s.m2cap || nrec > INT32_MAX) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    rc = ensure_arcs(s, (int64_t)hi + h.rec_add, err);   // the only new arcs: one running arc per placed task
    if (rc == KS_OK) rc = ensure_hash(s, h.rec_add, err);
    if (rc == KS_OK) rc = size_stream(s, nrec, 0, err);
    if (rc) return rc;
    d = s.schd();   // (the arc table may have moved)
    *dirty = true;
    KS_CHECK(sched_commit_emit(d, c, s.d_recs.p, st));
    // (arc_recs false although most records are UPDATE_ARC: the commit never reset cell_refused)
    rc = apply_stream(s, nrec, {}, false, err, log ? s.kev[1] : nullptr);
    if (rc) return rc;
    if (log) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "commit: %lld records, deltas %.3f ms, count passes %.3f ms, emit + apply %.3f ms, "
                     "device span after the deltas %.3f ms\n",
                     (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3), ev_ms(s.kev[0], s.kev[1]));
    }
    return KS_OK;
}

int Engine::commit_schedule(int flags, int64_t ccost, const uint64_t* ids, size_t k, int64_t sink_slot,
                            int64_t n_tasks, size_t cap, std::vector<ks_sched_delta>* out, size_t* count,
                            ks_commit_stats* stats, bool* dirty, std::string& err) {
    CommitCtl h{};
    const int rc = commit(false, flags, ccost, 0, ids, k, sink_slot, n_tasks, cap, out, count, &h, dirty, err);
    if (rc == KS_OK && stats) {
        const int64_t np = (int64_t)out->size();
        std::memset(stats, 0, sizeof(*stats));
        stats->placed = np;
        stats->running_converted = np - h.rec_add;
        stats->running_added = h.rec_add;
        stats->arcs_removed = h.rec_pin - stats->running_converted;
        stats->unsched_updates = h.unsched;
        stats->cap_updates = h.caps;
        stats->records = (int64_t)h.rec_pin + h.rec_add + h.rec_arc;
    }
    return rc;
}

int Engine::commit_preemptive(int flags, int64_t ccost, int64_t pcost, const uint64_t* ids, size_t k,
                              int64_t sink_slot, int64_t n_tasks, size_t cap, std::vector<ks_sched_delta>* out,
                              size_t* count, ks_preempt_stats* stats, bool* dirty, std::string& err) {
    CommitCtl h{};
    const int rc = commit(true, flags, ccost, pcost, ids, k, sink_slot, n_tasks, cap, out, count, &h, dirty, err);
    if (rc == KS_OK && stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (const ks_sched_delta& x : *out)
            ++(x.type == KS_DELTA_PLACE ? stats->placed : x.type == KS_DELTA_PREEMPT ? stats->preempted : stats->migrated);
        stats->running_added = h.rec_add;
        stats->running_converted = h.converted;
        stats->running_removed = h.removed;
        stats->unsched_cost_updates = h.rec_pin - h.converted - h.removed;
        stats->cap_updates = h.caps;
        stats->records = (int64_t)h.rec_pin + h.rec_add + h.rec_arc;
    }
    return rc;
}

// ks_remove_resources: the third body beside commit. The subtree is marked level by level
// (one host sync each: the depth is the topology's height below the roots), the evictions
// and the ascending id list come from two flag scans, the capacities from the commit's
// passes over the graph without the subtree. One control copy brings the counts; then the
// removed ids go to the host, which checks them against its node table and returns the
// node edits (make_edits), and the REMOVE_NODE records (stream positions 0 … nremoved − 1)
// with the capacity records behind them reach store_apply as one stream.
int Engine::remove_resources(int flags, const uint64_t* roots, size_t k, int64_t sink_slot, bool probe, size_t rcap,
                             size_t ecap, std::vector<uint64_t>* removed, std::vector<ks_sched_delta>* evicted,
                             size_t* nremoved, size_t* nevicted, ks_remove_stats* stats, const RemoveEdits& make_edits,
                             bool* dirty, std::string& err, const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = false;
    *nremoved = *nevicted = 0;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    int rc = fresh_csr(s, err);   // the descent and the BFS walk the residual CSR
    if (rc) return rc;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const bool caps = (flags & KS_REMOVE_RESOURCE_CAPS) != 0;
    const int64_t ncap = s.ncap, nst = s.nstore;
    const int hi = s.hi();
    rc = check_one_sink(s, caps, sink_slot, err);
    if (rc) return rc;
    if (k > (size_t)INT32_MAX) {
        err = "too many roots";
        return KS_E_RANGE;
    }
    CommitDev c{};
    c.preempt = (flags & KS_REMOVE_PREEMPTIVE) ? 1 : 0;
    c.resource_caps = 1;
    c.removing = 1;
    RemoveDev r{};
    r.k = (int)k;
    unsigned long long *d_roots = nullptr, *d_ids = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        for (int** a : {&r.front, &r.next, &r.nch, &r.ch_off, &r.rm, &r.rm_pos, &r.ev, &r.ev_pos}) *a = ci.take(ncap + 1);
        for (int** a : {&c.aflag, &c.a_off}) *a = ci.take((int64_t)hi + 1);
        for (unsigned long long** a : {&c.agg_cnt, &c.pu_slots, &c.pu_run, &c.slots, &c.running}) *a = cu.take(nst + 1);
        d_roots = cu.take(k);
        d_ids = cu.take(ncap + 1);
    }, kAllU64, true, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.cm_ctl, st));
    KS_CHECK(clear_ctl(s.rm_ctl, st));
    c.fl = r.fl = s.cm_b.p;
    c.ctl = s.cm_ctl.p;
    r.ctl = s.rm_ctl.p;
    r.roots = d_roots;
    if (k) KS_CHECK(hipMemcpyAsync(d_roots, roots, k * 8, hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    RemoveCtl h{};
    // ---- 1. the subtree
    KS_CHECK(sched_remove_seed(d, r, st));
    KS_CHECK(hipMemcpyAsync(&h, r.ctl, sizeof(RemoveCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    if (h.bad_root) {
        const uint64_t id = roots[k - (size_t)h.bad_root];
        err = id_name(bv, "root", id) + " is not a live resource or type-0 node (dead, beyond the graph, a task or a sink)";
        return KS_E_INVALID;
    }
    const int64_t nroots = h.nfront;
    int levels = 0;
    for (int nf = h.nfront; nf > 0 && levels <= s.nn; ++levels) {
        std::swap(r.front, r.next);
        KS_CHECK(hipMemsetAsync(&r.ctl->nfront, 0, sizeof(int), st));
        KS_CHECK(sched_remove_chunks(d, r, nf, st));
        KS_CHECK(exclusive_sum(s, (const int*)r.nch, r.ch_off, (int64_t)nf + 1, st));
        KS_CHECK(sched_remove_level(d, r, nf, (int)(nf + s.m2cap / 64 + 1), st));
        KS_CHECK(hipMemcpyAsync(&h.nfront, &r.ctl->nfront, sizeof(int), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        nf = h.nfront;
        if (nf < 0 || nf > ncap) {
            err = "inconsistent frontier length";
            return KS_E_DEVICE;
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    // ---- 2, 3. the evictions and the removed list: two flag scans over the node slots
    KS_CHECK(sched_remove_flags(d, r, st));
    KS_CHECK(exclusive_sum(s, (const int*)r.rm, r.rm_pos, ncap + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)r.ev, r.ev_pos, ncap + 1, st));
    if (log) KS_CHECK(hipStreamSynchronize(st));   // (only to split the log line's times)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 4. the capacities over the graph without the subtree
    if (caps) {
        KS_CHECK(sched_commit_pu(d, c, st));
        KS_CHECK(sched_remove_zero_pus(d, r, c, st));
        rc = topo_bfs(s, d, sink_slot, 0, c.pu_slots, c.pu_run, c.slots, c.running, err);
        if (rc) return rc;
        KS_CHECK(sched_commit_arc_flags(d, c, st));
        KS_CHECK(exclusive_sum(s, (const int*)c.aflag, c.a_off, (int64_t)hi + 1, st));
    }
    KS_CHECK(sched_remove_totals(d, r, c, caps ? 1 : 0, st));
    KS_CHECK(hipMemcpyAsync(&h, r.ctl, sizeof(RemoveCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t3 = std::chrono::steady_clock::now();
    if (h.nremoved < nroots || h.nremoved > ncap || h.nevicted < 0 || h.nevicted > ncap || h.rec_arc < 0 ||
        h.rec_arc > hi) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    *nremoved = (size_t)h.nremoved;
    *nevicted = (size_t)h.nevicted;
    if (probe) return KS_OK;
    if (rcap < *nremoved || ecap < *nevicted) {
        err = rcap < *nremoved ? "removed buffer smaller than the " + std::to_string(h.nremoved) + " removed nodes"
                               : "evicted buffer smaller than the " + std::to_string(h.nevicted) + " evicted tasks";
        return KS_E_INVALID;
    }
    if (h.bad) {
        err = "a capacity would fall below its arc's lower bound";
        return KS_E_VERIFY;
    }
    const int64_t nrec = (int64_t)h.nremoved + h.rec_arc;
    rc = size_stream(s, nrec, (size_t)h.nremoved, err);
    if (rc) return rc;
    KS_CHECK(s.sched_d.ensure(std::max(1, h.nevicted)));
    KS_CHECK(sched_remove_emit_nodes(d, r, d_ids, s.d_recs.p, st));
    removed->resize(h.nremoved);
    if (h.nremoved) KS_CHECK(hipMemcpyAsync(removed->data(), d_ids, h.nremoved * 8, hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    // the host's node table follows (and names an id it does not know as alive); from here
    // on a failure leaves the device state unknown
    std::vector<NodeEdit> edits;
    rc = make_edits(removed->data(), removed->size(), &edits, err);
    if (rc) return rc;
    *dirty = true;
    KS_CHECK(sched_remove_emit_evictions(d, r, s.sched_d.p, st));
    if (caps) KS_CHECK(sched_commit_emit(d, c, s.d_recs.p, st));
    evicted->resize(h.nevicted);   // (on the stream before the tail's sync)
    if (h.nevicted)
        KS_CHECK(hipMemcpyAsync(evicted->data(), s.sched_d.p, h.nevicted * sizeof(ks_sched_delta), hipMemcpyDeviceToHost,
                                st));
    rc = apply_stream(s, nrec, edits, h.rec_arc != 0, err);
    if (rc) return rc;
    if (log) {
        const auto t4 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "remove: %lld nodes, %lld evictions, %lld records, %d levels, mark %.3f ms, evict %.3f ms, "
                     "caps %.3f ms, emit + apply %.3f ms\n",
                     (long long)h.nremoved, (long long)h.nevicted, (long long)nrec, levels, ms(t0, t1), ms(t1, t2),
                     ms(t2, t3), ms(t3, t4));
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->roots = nroots;
        stats->nodes_removed = h.nremoved;
        stats->tasks_evicted = h.nevicted;
        stats->arcs_removed = s.h_sctl->killed;
        stats->cap_updates = h.rec_arc;
        stats->records = nrec;
    }
    return KS_OK;
}

// ks_complete_tasks: the fourth body. The ids are checked and claimed in the flag bytes (one
// host sync: the first illegal id, the distinct count, left), their segments' chunk items
// count the aggregators' losses, the ascending id list comes from the removal's flag scan and
// the capacities from the commit's passes in their completing mode. One more sync brings the
// counts; then the ids go to the host for its node edits (make_edits) and the REMOVE_NODE
// records (stream positions 0 … n − 1) with the capacity records behind them reach store_apply
// as one stream.
int Engine::complete_tasks(int flags, const uint64_t* tasks, size_t k, const uint64_t* unsched_ids, size_t nu,
                           int64_t sink_slot, uint64_t* left, ks_complete_stats* stats, const RemoveEdits& make_edits,
                           bool* dirty, bool* changed, std::string& err, const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = *changed = false;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const bool caps = (flags & KS_COMPLETE_RESOURCE_CAPS) != 0;
    if (!k && !caps) return KS_OK;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    int rc = fresh_csr(s, err);   // the chunk items and the BFS walk the residual CSR
    if (rc) return rc;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t ncap = s.ncap, nst = s.nstore;
    const int hi = s.hi();
    rc = check_one_sink(s, caps, sink_slot, err);
    if (rc) return rc;
    if (k > (size_t)INT32_MAX || nu > (size_t)INT32_MAX) {
        err = "too many ids";
        return KS_E_RANGE;
    }
    rc = check_agg_ids(s, unsched_ids, nu, err);
    if (rc) return rc;
    CommitDev c{};
    c.preempt = (flags & KS_COMPLETE_PREEMPTIVE) ? 1 : 0;
    c.resource_caps = caps ? 1 : 0;
    c.removing = 1;   // (no capacity record names a completed task)
    c.completing = 1;
    RemoveDev r{};
    r.k = (int)k;
    unsigned long long *d_tasks = nullptr, *d_left = nullptr, *d_agg = nullptr, *d_ids = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        for (int** a : {&r.front, &r.next, &r.nch, &r.ch_off, &r.rm, &r.rm_pos, &r.ev, &r.ev_pos}) *a = ci.take(ncap + 1);
        for (int** a : {&c.aflag, &c.a_off}) *a = ci.take((int64_t)hi + 1);
        for (unsigned long long** a : {&c.agg_cnt, &c.pu_slots, &c.pu_run, &c.slots, &c.running}) *a = cu.take(nst + 1);
        d_tasks = cu.take(k);
        d_left = cu.take(k);
        d_agg = cu.take(nu);
        d_ids = cu.take(ncap + 1);
    }, kAllU64, true, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.cm_ctl, st));
    KS_CHECK(clear_ctl(s.rm_ctl, st));
    c.fl = r.fl = s.cm_b.p;
    c.ctl = s.cm_ctl.p;
    r.ctl = s.rm_ctl.p;
    r.roots = d_tasks;
    if (k) KS_CHECK(hipMemcpyAsync(d_tasks, tasks, k * 8, hipMemcpyHostToDevice, st));
    if (unsched_ids && nu) KS_CHECK(hipMemcpyAsync(d_agg, unsched_ids, nu * 8, hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    RemoveCtl h{};
    std::vector<uint64_t> h_left(k);
    // ---- 1. the ids: checked, claimed, their bindings read
    int np = 0;
    if (k) {
        KS_CHECK(sched_complete_seed(d, r, unsched_ids ? d_agg : nullptr, (int)nu, d_left, st));
        KS_CHECK(hipMemcpyAsync(&h, r.ctl, sizeof(RemoveCtl), hipMemcpyDeviceToHost, st));
        KS_CHECK(hipMemcpyAsync(h_left.data(), d_left, k * 8, hipMemcpyDeviceToHost, st));
        KS_CHECK(hipStreamSynchronize(st));
        if (h.bad_root) {
            const uint64_t id = tasks[k - (size_t)h.bad_root];
            err = id_name(bv, "task", id) + " is not a live task node (0, beyond the graph, dead or of another type)";
            return KS_E_INVALID;
        }
        np = h.nfront;
        if (np < 1 || np > ncap || (size_t)np > k || h.nbound < 0 || h.nbound > np) {
            err = "inconsistent task count";
            return KS_E_DEVICE;
        }
    }
    const int nbound = h.nbound;
    const auto t1 = std::chrono::steady_clock::now();
    // ---- 2. the aggregators' losses, from the completed tasks' own segments
    if (np) {
        std::swap(r.front, r.next);
        KS_CHECK(sched_remove_chunks(d, r, np, st));
        KS_CHECK(exclusive_sum(s, (const int*)r.nch, r.ch_off, (int64_t)np + 1, st));
        KS_CHECK(sched_complete_count(d, r, c, np, (int)(np + s.m2cap / 64 + 1), st));
    }
    // the ascending id list: a flag scan over the node slots
    KS_CHECK(sched_remove_flags(d, r, st));
    KS_CHECK(exclusive_sum(s, (const int*)r.rm, r.rm_pos, ncap + 1, st));
    if (log) KS_CHECK(hipStreamSynchronize(st));   // (only to split the log line's times)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 3. the capacities over the graph without the completed tasks
    if (caps) {
        KS_CHECK(sched_commit_pu(d, c, st));
        rc = topo_bfs(s, d, sink_slot, 0, c.pu_slots, c.pu_run, c.slots, c.running, err);
        if (rc) return rc;
    }
    KS_CHECK(sched_commit_arc_flags(d, c, st));
    KS_CHECK(exclusive_sum(s, (const int*)c.aflag, c.a_off, (int64_t)hi + 1, st));
    KS_CHECK(sched_remove_totals(d, r, c, 1, st));
    CommitCtl hc{};
    KS_CHECK(hipMemcpyAsync(&h, r.ctl, sizeof(RemoveCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipMemcpyAsync(&hc, c.ctl, sizeof(CommitCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t3 = std::chrono::steady_clock::now();
    if (h.nremoved != np || h.nevicted != 0 || h.rec_arc < 0 || h.rec_arc > hi ||
        hc.unsched + hc.caps != h.rec_arc) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    if (h.bad) {
        err = "a capacity would fall below its arc's lower bound";
        return KS_E_VERIFY;
    }
    const int64_t nrec = (int64_t)np + h.rec_arc;
    if (left && k) std::memcpy(left, h_left.data(), k * 8);
    if (!nrec) return KS_OK;   // (k == 0 and every capacity stands: the solution stays valid)
    rc = size_stream(s, nrec, (size_t)np, err);
    if (rc) return rc;
    KS_CHECK(sched_remove_emit_nodes(d, r, d_ids, s.d_recs.p, st));
    std::vector<uint64_t> ids(np);
    if (np) KS_CHECK(hipMemcpyAsync(ids.data(), d_ids, (size_t)np * 8, hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    // the host's node table follows (and names an id it does not hold as a live task); from
    // here on a failure leaves the device state unknown
    std::vector<NodeEdit> edits;
    rc = make_edits(ids.data(), ids.size(), &edits, err);
    if (rc) return rc;
    *dirty = true;
    KS_CHECK(sched_commit_emit(d, c, s.d_recs.p, st));
    rc = apply_stream(s, nrec, edits, h.rec_arc != 0, err);
    if (rc) return rc;
    if (log) {
        const auto t4 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "complete: %d tasks, %lld records, seed %.3f ms, aggregator counts %.3f ms, caps %.3f ms, "
                     "emit + apply %.3f ms\n",
                     np, (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4));
    }
    *changed = true;
    if (stats) {
        stats->tasks = np;
        stats->bound = nbound;
        stats->arcs_removed = s.h_sctl->killed;
        stats->unsched_updates = hc.unsched;
        stats->cap_updates = hc.caps;
        stats->records = nrec;
    }
    return KS_OK;
}

// ks_add_tasks: the fifth body. The ids were checked against the host's node table; the ids,
// the offsets and the 16-byte arcs go up, one lane per arc checks its head and cost and counts
// the aggregators' gains, the store's index says which gaining aggregator still has its arc
// into the sink, and ONE host sync brings every refusal and the record counts (no step before
// it changes anything, so the checks need no sync of their own). Then the host's node edits,
// the sizing of the node store, the arc table and the index, and the ADD_NODE records (stream
// positions 0 … k − 1), the task arcs (k …) and the aggregator records behind them reach
// store_apply as one stream. Neither the residual CSR nor the topology BFS is needed.
int Engine::add_tasks(const uint64_t* tasks, size_t k, const uint64_t* arc_off, const ks_task_arc* arcs,
                      const uint64_t* unsched_ids, size_t nu, int64_t sink_slot, int64_t sink_cost, int64_t nslots,
                      ks_add_stats* stats, const AddEdits& make_edits, bool* dirty, std::string& err,
                      const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = false;
    if (!k) return KS_OK;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nst = s.nstore;
    const size_t na = (size_t)arc_off[k];
    if (k > (size_t)INT32_MAX / 4 || na > (size_t)INT32_MAX / 4 || nu > (size_t)INT32_MAX) {
        err = "too many tasks, arcs or aggregator ids";
        return KS_E_RANGE;
    }
    int rc = check_agg_ids(s, unsched_ids, nu, err);
    if (rc) return rc;
    AddDev a{};
    a.k = (int)k;
    a.na = (int)na;
    a.nst = nst;
    a.null_rule = unsched_ids ? 0 : 1;
    a.sink = sink_slot >= 0 && sink_slot < nst ? sink_slot : -1;
    a.sink_cost = sink_cost;
    unsigned long long *d_tasks = nullptr, *d_off = nullptr, *d_arcs = nullptr, *d_agg = nullptr;
    unsigned long long *d_goff = nullptr, *d_base = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        a.t_agg = ci.take((int64_t)k + 1);
        for (int** x : {&a.aflag, &a.a_off, &a.a_slot}) *x = ci.take(nst + 1);
        a.agg_cnt = cu.take(nst + 1);   // (first: the only u64 array that starts zeroed)
        d_tasks = cu.take(k);
        d_off = cu.take(k + 1);
        d_arcs = cu.take(2 * na);
        d_agg = cu.take(nu);
        d_goff = cu.take(bv ? bv->ng + 1 : 0);
        d_base = cu.take(bv ? bv->ng + 1 : 0);
    }, nst + 1, true, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.add_ctl, st));
    a.fl = s.cm_b.p;
    a.ctl = s.add_ctl.p;
    a.tasks = d_tasks;
    a.arc_off = d_off;
    a.arcs = (const ks_task_arc*)d_arcs;
    wire_hash(s, a);
    KS_CHECK(hipMemcpyAsync(d_tasks, tasks, k * 8, hipMemcpyHostToDevice, st));
    KS_CHECK(hipMemcpyAsync(d_off, arc_off, (k + 1) * 8, hipMemcpyHostToDevice, st));
    if (na) KS_CHECK(hipMemcpyAsync(d_arcs, arcs, na * sizeof(ks_task_arc), hipMemcpyHostToDevice, st));
    if (unsched_ids && nu) KS_CHECK(hipMemcpyAsync(d_agg, unsched_ids, nu * 8, hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    rc = wire_cell_sinks(s, d, a, sink_slot, err);
    if (rc == KS_OK && bv && na) rc = translate_heads<ks_task_arc>(s, *bv, d_goff, d_base, d_arcs, na, &a.ctl->bad_range, err);
    if (rc) return rc;
    // ---- 1. heads, costs, the aggregators' gains and their arcs into the sink: one sync
    KS_CHECK(sched_add_check(d, a, unsched_ids ? d_agg : nullptr, (int)nu, st));
    KS_CHECK(exclusive_sum(s, (const int*)a.aflag, a.a_off, nst + 1, st));
    KS_CHECK(sched_add_totals(a, st));
    AddCtl h{};
    KS_CHECK(hipMemcpyAsync(&h, a.ctl, sizeof(AddCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    auto task_of = [&](size_t j) {   // the last i with arc_off[i] ≤ j
        return (size_t)(std::upper_bound(arc_off, arc_off + k, (uint64_t)j) - arc_off) - 1;
    };
    if (bv && h.bad_range) return range_refusal(*bv, h.bad_range, "task", tasks, arc_off, k, arcs, na, err);
    if (h.bad_head || h.bad_cost) {   // the first offending arc in input order; on one arc the head comes first
        size_t jh, jc;
        if (!first_bad(h.bad_head, na, &jh) || !first_bad(h.bad_cost, na, &jc)) {
            err = "inconsistent arc index";
            return KS_E_DEVICE;
        }
        const bool head = jh <= jc;
        const size_t j = head ? jh : jc;
        const std::string who = id_name(bv, "task", tasks[task_of(j)]) + ": ";
        if (head) {
            err = who + "head " + std::to_string(arcs[j].dst) + " is not a node that was live before the call and is no "
                  "task (0, beyond the graph, dead, a task, or a task of this call)";
            return KS_E_INVALID;
        }
        err = who + "the cost of its arc into " + std::to_string(arcs[j].dst) + " is outside the supported range";
        return KS_E_RANGE;
    }
    if (h.bad_multi || h.bad_none) {
        size_t im, in;
        if (!first_bad(h.bad_multi, k, &im) || !first_bad(h.bad_none, k, &in)) {
            err = "inconsistent task index";
            return KS_E_DEVICE;
        }
        const bool multi = im <= in;
        const uint64_t id = tasks[multi ? im : in];
        err = multi ? id_name(bv, "task", id) + " has more than one arc into unscheduled aggregators: a task has one job"
                    : id_name(bv, "task", id) + " has no arc into a node with an arc into the sink; an aggregator "
                      "whose capacity fell to 0 has lost that arc: pass the aggregators' ids (unsched_ids)";
        return KS_E_INVALID;
    }
    if (a.cell_sink && h.bad_sink) return sink_refusal(bv, h.bad_sink, nst, err);
    if (h.units && a.sink < 0 && !a.cell_sink) {
        err = "an unscheduled aggregator's capacity needs exactly one sink";
        return KS_E_INVALID;
    }
    if (h.units < 0 || (size_t)h.units > na || h.rec_upd < 0 || h.rec_add < 0 || h.rec_upd + h.rec_add != h.rec_agg ||
        h.rec_agg > h.units || (h.units > 0) != (h.rec_agg > 0)) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    // ---- 2. room for the new nodes and arcs; the host's node table follows
    const int64_t nrec = (int64_t)k + (int64_t)na + h.rec_agg;
    rc = ensure_nodes(s, std::max<int64_t>(nslots, 1), err);
    if (rc == KS_OK) rc = ensure_arcs(s, (int64_t)s.hi() + (int64_t)na + h.rec_add, err);
    if (rc == KS_OK) rc = ensure_hash(s, (int64_t)na + h.rec_add, err);
    if (rc == KS_OK) rc = size_stream(s, nrec, k, err);
    if (rc) return rc;
    std::vector<NodeEdit> edits;
    make_edits(&edits);
    // from here on a failure leaves the device state unknown
    *dirty = true;
    s.nslots = std::max(s.nslots, nslots);
    d = s.schd();   // (the node store and the arc table may have moved)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 3. the records, at their fixed positions, and the apply
    KS_CHECK(sched_add_emit(d, a, s.d_recs.p, st));
    rc = apply_stream(s, nrec, edits, nrec > (int64_t)k, err);
    if (rc) return rc;
    if (log) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "add: %zu tasks, %zu arcs, %lld records, upload + checks + counts %.3f ms, node table + sizing "
                     "%.3f ms, emit + apply %.3f ms\n",
                     k, na, (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3));
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->tasks = (int64_t)k;
        stats->arcs_added = (int64_t)na;
        stats->unsched_updates = h.rec_upd;
        stats->unsched_added = h.rec_add;
        stats->records = nrec;
    }
    return KS_OK;
}

// ks_add_resources: the sixth body, on the scratch carve of add_tasks. The nodes were checked
// against the host's node table and entered there; the two 32-byte arrays go up, one lane per
// edge checks it and claims the child's parent word, the new PUs' slots climb the parent words,
// the store's index says which edge into a live head is still held, and ONE host sync brings
// every refusal and the record counts (no step before it writes anything but scratch). Then the
// host's node edits, the sizing of the node store, the arc table and the index, and the
// ADD_NODE records (stream positions 0 … n − 1), the PU → sink arcs and the edge records behind
// them reach store_apply as one stream. Neither the residual CSR nor the topology BFS is needed.
// first_pair: the first edge that repeats an earlier (parent, child), m: none (the host's sort).
int Engine::add_resources(const ks_res_node* nodes, size_t n, const ks_res_arc* arcs, size_t m, size_t first_pair,
                          int64_t sink_slot, int64_t nslots, ks_grow_stats* stats, const AddEdits& make_edits,
                          bool* dirty, bool* changed, std::string& err, const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = *changed = false;
    if (!n && !m) return KS_OK;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nst = s.nstore;
    if (n > (size_t)INT32_MAX / 16 || m > (size_t)INT32_MAX / 16) {
        err = "too many resource nodes or edges";
        return KS_E_RANGE;
    }
    // under a view the records are graph-local: the graph of node i or edge j, and how a message names it
    auto graph_of = [&](const uint64_t* goff, size_t j) {
        return (size_t)(std::upper_bound(goff, goff + bv->ng, (uint64_t)j) - goff) - 1;
    };
    auto in_graph = [&](const uint64_t* goff, size_t j) {
        return bv ? "graph " + std::to_string(bv->graph[graph_of(goff, j)]) + ": " : std::string();
    };
    int64_t ntot = nst, pus = 0, slots = 0;
    for (size_t i = 0; i < n; ++i) {
        ntot = std::max<int64_t>(ntot, (int64_t)nodes[i].id + (bv ? bv->off[graph_of(bv->node_goff, i)] : 0));
        if (nodes[i].type == KS_NODE_PU) {
            ++pus;
            slots += (int64_t)nodes[i].slots;
        }
    }
    GrowDev g{};
    g.n = (int)n;
    g.m = (int)m;
    g.nst = nst;
    g.ntot = ntot;
    g.sink = sink_slot >= 0 && sink_slot < nst ? sink_slot : -1;
    unsigned long long *d_nodes = nullptr, *d_arcs = nullptr;
    unsigned long long *d_ngoff = nullptr, *d_agoff = nullptr, *d_base = nullptr;
    int rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        for (int** x : {&g.newt, &g.par}) *x = ci.take(ntot + 1);
        for (int** x : {&g.nflag, &g.n_off}) *x = ci.take((int64_t)n + 1);
        for (int** x : {&g.eflag, &g.e_off, &g.e_slot}) *x = ci.take((int64_t)m + 1);
        g.S = cu.take(ntot + 1);   // (first: the only u64 array that starts zeroed)
        d_nodes = cu.take(4 * (int64_t)n);
        d_arcs = cu.take(4 * (int64_t)m);
        for (unsigned long long** x : {&d_ngoff, &d_agoff, &d_base}) *x = cu.take(bv ? bv->ng + 1 : 0);
    }, ntot + 1, false, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.grow_ctl, st));
    g.ctl = s.grow_ctl.p;
    g.nodes = (const ks_res_node*)d_nodes;
    g.arcs = (const ks_res_arc*)d_arcs;
    wire_hash(s, g);
    if (n) KS_CHECK(hipMemcpyAsync(d_nodes, nodes, n * sizeof(ks_res_node), hipMemcpyHostToDevice, st));
    if (m) KS_CHECK(hipMemcpyAsync(d_arcs, arcs, m * sizeof(ks_res_arc), hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    rc = pus ? wire_cell_sinks(s, d, g, sink_slot, err) : KS_OK;
    if (rc) return rc;
    if (pus && g.sink < 0 && !g.cell_sink) {
        err = "a new PU's arc into the sink needs exactly one sink";
        return KS_E_INVALID;
    }
    if (bv) {   // the records leave their graphs' numbering on the device
        KS_CHECK(hipMemcpyAsync(d_ngoff, bv->node_goff, (bv->ng + 1) * 8, hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(d_agoff, bv->arc_goff, (bv->ng + 1) * 8, hipMemcpyHostToDevice, st));
        KS_CHECK(hipMemcpyAsync(d_base, bv->off, (bv->ng + 1) * 8, hipMemcpyHostToDevice, st));
        KS_CHECK(sched_translate_res((ks_res_node*)d_nodes, (int)n, (ks_res_arc*)d_arcs, (int)m, d_ngoff, d_agoff,
                                     (const long long*)d_base, (int)bv->ng, g.ctl, st));
    }
    // ---- 1. the edges, the sums and the arcs the store still holds: one sync
    KS_CHECK(sched_grow_check(d, g, st));
    KS_CHECK(exclusive_sum(s, (const int*)g.nflag, g.n_off, (int64_t)n + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)g.eflag, g.e_off, (int64_t)m + 1, st));
    KS_CHECK(sched_grow_totals(g, st));
    GrowCtl h{};
    KS_CHECK(hipMemcpyAsync(&h, g.ctl, sizeof(GrowCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    if (bv && h.bad_range) {   // the first record in input order (nodes, then edges) with an id outside its graph
        size_t i;
        if (!first_bad(h.bad_range, n + m, &i) || i >= n + m) {
            err = "inconsistent record index";
            return KS_E_DEVICE;
        }
        const bool node = i < n;
        const size_t j = node ? i : i - n;
        const size_t gi = graph_of(node ? bv->node_goff : bv->arc_goff, j);
        const uint64_t span = (uint64_t)(bv->off[gi + 1] - bv->off[gi]);
        const bool parent = !node && (arcs[j].parent < 1 || arcs[j].parent > span);
        err = "graph " + std::to_string(bv->graph[gi]) + ": " +
              (node ? "resource node id " + std::to_string(nodes[j].id)
                    : "edge " + std::to_string(arcs[j].parent) + " -> " + std::to_string(arcs[j].child) + ": " +
                          (parent ? "parent " + std::to_string(arcs[j].parent) : "child " + std::to_string(arcs[j].child))) +
              outside_ids_tail((int64_t)span);
        return KS_E_RANGE;
    }
    if (h.bad_edge || first_pair < m) {   // the first offending edge in input order; on one edge the lowest class
        size_t j;   // (the word: count − index, then 7 − class in the low three bits)
        if (!first_bad(h.bad_edge >> 3, m, &j) || (h.bad_edge && ((h.bad_edge & 7) == 0 || h.bad_edge < 8))) {
            err = "inconsistent edge index";
            return KS_E_DEVICE;
        }
        int cls = h.bad_edge ? 7 - (h.bad_edge & 7) : 7;
        if (first_pair < j || (first_pair == j && cls == 6)) {   // (the repeated pair ranks before the second parent)
            j = first_pair;
            cls = 7;
        }
        const ks_res_arc& e = arcs[j];
        const std::string who = in_graph(bv ? bv->arc_goff : nullptr, j) + "edge " + std::to_string(e.parent) + " -> " +
                                std::to_string(e.child) + ": ";
        switch (cls) {
            case 0:
                err = who + "parent " + std::to_string(e.parent) + " is not a node of this call or a live node that is no task, "
                      "no sink and no PU";
                break;
            case 1:
                err = who + "child " + std::to_string(e.child) + " is not a node of this call or a live node that is no task and "
                      "no sink";
                break;
            case 2: err = who + "parent and child are node " + std::to_string(e.child); break;
            case 3: err = who + "unknown kind " + std::to_string(e.kind); break;
            case 4:
                err = who + "a tree edge from a new parent to live node " + std::to_string(e.child) + ": a live node does not move";
                break;
            case 5: err = who + "the cost is outside the supported range"; return KS_E_RANGE;
            case 6: err = who + "child " + std::to_string(e.child) + " has a second tree edge: a resource has one parent"; break;
            default: err = who + "the pair is listed twice"; break;
        }
        return KS_E_INVALID;
    }
    if (h.bad_depth) {
        size_t i;
        if (!first_bad(h.bad_depth, n, &i)) {
            err = "inconsistent node index";
            return KS_E_DEVICE;
        }
        err = in_graph(bv ? bv->node_goff : nullptr, i) + "PU " + std::to_string(nodes[i].id) + ": its tree edges do not end after " +
              std::to_string(KS_RES_MAX_DEPTH) + " steps (a cycle, or a topology too deep)";
        return KS_E_INVALID;
    }
    if (h.bad_cap) {
        size_t j;
        if (!first_bad(h.bad_cap, m, &j)) {
            err = "inconsistent edge index";
            return KS_E_DEVICE;
        }
        const ks_res_arc& e = arcs[j];
        err = in_graph(bv ? bv->arc_goff : nullptr, j) + "edge " + std::to_string(e.parent) + " -> " + std::to_string(e.child) +
              ": the raised capacity is outside the supported range";
        return KS_E_RANGE;
    }
    if (g.cell_sink && h.bad_sink) {   // the first new PU in input order whose cell has no single sink
        size_t i;
        if (!first_bad(h.bad_sink, n, &i) || i >= n) {
            err = "inconsistent node index";
            return KS_E_DEVICE;
        }
        err = in_graph(bv ? bv->node_goff : nullptr, i) + "PU " + std::to_string(nodes[i].id) +
              ": its cell has no sink or several, and a new PU's arc into the sink needs exactly one";
        return KS_E_INVALID;
    }
    if (h.rec_upd < 0 || h.rec_add < 0 || h.skipped < 0 || h.rec_upd + h.rec_add != h.rec_edge ||
        (int64_t)h.rec_edge + h.skipped != (int64_t)m || h.rec_pu != pus) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->arcs_skipped = h.skipped;
    }
    const int64_t nrec = (int64_t)n + h.rec_pu + h.rec_edge;
    if (!nrec) return KS_OK;   // chain edges alone with no new slot beneath them: nothing to write
    // ---- 2. room for the new nodes and arcs; the host's node table follows
    rc = ensure_nodes(s, std::max<int64_t>(nslots, 1), err);
    if (rc == KS_OK) rc = ensure_arcs(s, (int64_t)s.hi() + h.rec_pu + h.rec_add, err);
    if (rc == KS_OK) rc = ensure_hash(s, (int64_t)h.rec_pu + h.rec_add, err);
    if (rc == KS_OK) rc = size_stream(s, nrec, n, err);
    if (rc) return rc;
    std::vector<NodeEdit> edits;
    make_edits(&edits);
    // from here on a failure leaves the device state unknown
    *dirty = *changed = true;
    s.nslots = std::max(s.nslots, nslots);
    d = s.schd();   // (the node store and the arc table may have moved)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 3. the records, at their fixed positions, and the apply
    KS_CHECK(sched_grow_emit(d, g, h.rec_pu, s.d_recs.p, st));
    rc = apply_stream(s, nrec, edits, nrec > (int64_t)n, err);
    if (rc) return rc;
    if (log) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "grow: %zu nodes, %zu edges, %lld records, upload + checks + sums %.3f ms, node table + sizing "
                     "%.3f ms, emit + apply %.3f ms\n",
                     n, m, (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3));
    }
    if (stats) {
        stats->nodes = (int64_t)n;
        stats->pus = pus;
        stats->slots = slots;
        stats->sink_arcs = h.rec_pu;
        stats->arcs_added = h.rec_add;
        stats->cap_updates = h.rec_upd;
        stats->records = nrec;
    }
    return KS_OK;
}

// ks_update_tasks: the seventh body, on the scratch carve of add_tasks. The ids, the offsets and
// the 16-byte arcs go up; one lane per id checks and claims it, one lane per listed arc checks its
// head and cost and asks the store's index for the arc's slot, the tasks' segments (or, with
// KS_UPDATE_KEEP_UNLISTED, the arc table: no CSR is needed then) give the held arcs nobody listed,
// the aggregators' part is that of add_tasks, and ONE host sync brings every refusal and the
// record counts (no step before it writes anything but scratch). Then the sizing of the arc table
// and the index, and the records on held arcs (ascending arc slot), the new arcs (input order)
// and the aggregator records (ascending id) reach store_apply as one stream. No node is edited.
int Engine::update_tasks(int flags, const uint64_t* tasks, size_t k, const uint64_t* arc_off, const ks_task_arc* arcs,
                         size_t first_pair, const uint64_t* unsched_ids, size_t nu, int64_t sink_slot,
                         int64_t sink_cost, ks_update_stats* stats, bool* dirty, bool* changed, std::string& err,
                         const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = *changed = false;
    if (!k) return KS_OK;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const bool walk = !(flags & KS_UPDATE_KEEP_UNLISTED);
    int rc = walk ? fresh_csr(s, err) : KS_OK;   // the chunk items walk the residual CSR
    if (rc) return rc;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nst = s.nstore;
    const int hi = s.hi();
    const size_t na = (size_t)arc_off[k];
    if (k > (size_t)INT32_MAX / 4 || na > (size_t)INT32_MAX / 4 || nu > (size_t)INT32_MAX) {
        err = "too many tasks, arcs or aggregator ids";
        return KS_E_RANGE;
    }
    rc = check_agg_ids(s, unsched_ids, nu, err);
    if (rc) return rc;
    UpdDev u{};
    u.k = (int)k;
    u.na = (int)na;
    u.hi = hi;
    u.keep = walk ? 0 : 1;
    u.null_rule = unsched_ids ? 0 : 1;
    u.nst = nst;
    AddDev a{};   // the aggregators' gains: the lookup and the records of add_tasks
    a.nst = nst;
    a.sink = sink_slot >= 0 && sink_slot < nst ? sink_slot : -1;
    a.sink_cost = sink_cost;
    unsigned long long *d_tasks = nullptr, *d_off = nullptr, *d_arcs = nullptr, *d_agg = nullptr;
    unsigned long long *d_goff = nullptr, *d_base = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        for (int** x : {&u.t_own, &a.aflag, &a.a_off, &a.a_slot}) *x = ci.take(nst + 1);
        for (int** x : {&u.t_slot, &u.t_agg, &u.nch, &u.ch_off}) *x = ci.take((int64_t)k + 1);
        for (int** x : {&u.seen, &u.sflag, &u.s_off}) *x = ci.take((int64_t)hi + 1);
        for (int** x : {&u.lflag, &u.l_off}) *x = ci.take((int64_t)na + 1);
        u.agg_cnt = cu.take(nst + 1);   // (first: the only u64 array that starts zeroed)
        d_tasks = cu.take(k);
        d_off = cu.take(k + 1);
        d_arcs = cu.take(2 * na);
        d_agg = cu.take(nu);
        d_goff = cu.take(bv ? bv->ng + 1 : 0);
        d_base = cu.take(bv ? bv->ng + 1 : 0);
    }, nst + 1, true, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.upd_ctl, st));
    KS_CHECK(clear_ctl(s.add_ctl, st));
    u.fl = a.fl = s.cm_b.p;
    a.agg_cnt = u.agg_cnt;
    u.ctl = s.upd_ctl.p;
    a.ctl = s.add_ctl.p;
    u.tasks = d_tasks;
    u.arc_off = d_off;
    u.arcs = (const ks_task_arc*)d_arcs;
    wire_hash(s, u);
    wire_hash(s, a);
    KS_CHECK(hipMemcpyAsync(d_tasks, tasks, k * 8, hipMemcpyHostToDevice, st));
    KS_CHECK(hipMemcpyAsync(d_off, arc_off, (k + 1) * 8, hipMemcpyHostToDevice, st));
    if (na) KS_CHECK(hipMemcpyAsync(d_arcs, arcs, na * sizeof(ks_task_arc), hipMemcpyHostToDevice, st));
    if (unsched_ids && nu) KS_CHECK(hipMemcpyAsync(d_agg, unsched_ids, nu * 8, hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    rc = wire_cell_sinks(s, d, a, sink_slot, err);
    if (rc == KS_OK && bv && na) rc = translate_heads<ks_task_arc>(s, *bv, d_goff, d_base, d_arcs, na, &a.ctl->bad_range, err);
    if (rc) return rc;
    // ---- 1. ids, heads, costs, the diff, the aggregators' gains and their arcs into the sink: one sync
    KS_CHECK(sched_upd_check(d, u, unsched_ids ? d_agg : nullptr, (int)nu, walk, st));
    if (walk) KS_CHECK(exclusive_sum(s, (const int*)u.nch, u.ch_off, (int64_t)k + 1, st));
    KS_CHECK(sched_upd_unlisted(d, u, walk, (int)(k + s.m2cap / 64 + 1), st));
    KS_CHECK(sched_add_agg_flags(d, a, st));
    KS_CHECK(exclusive_sum(s, (const int*)u.sflag, u.s_off, (int64_t)hi + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)u.lflag, u.l_off, (int64_t)na + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)a.aflag, a.a_off, nst + 1, st));
    KS_CHECK(sched_upd_totals(u, st));
    KS_CHECK(sched_add_totals(a, st));
    UpdCtl h{};
    AddCtl ha{};
    KS_CHECK(hipMemcpyAsync(&h, u.ctl, sizeof(UpdCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipMemcpyAsync(&ha, a.ctl, sizeof(AddCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    if (bv && ha.bad_range) return range_refusal(*bv, ha.bad_range, "task", tasks, arc_off, k, arcs, na, err);
    if (h.bad_task) {
        size_t i;
        if (!first_bad(h.bad_task, k, &i)) {
            err = "inconsistent task index";
            return KS_E_DEVICE;
        }
        err = id_name(bv, "task", tasks[i]) + " is not a live task node listed once (0, beyond "
              "the graph, dead, of another type, or listed before)";
        return KS_E_INVALID;
    }
    auto task_of = [&](size_t j) {   // the last i with arc_off[i] ≤ j
        return (size_t)(std::upper_bound(arc_off, arc_off + k, (uint64_t)j) - arc_off) - 1;
    };
    // the first offending arc in input order; on one arc the head, then the repeat, then the cost
    if (h.bad_head || h.bad_cost || first_pair < na) {
        size_t jh, jc;
        if (!first_bad(h.bad_head, na, &jh) || !first_bad(h.bad_cost, na, &jc)) {
            err = "inconsistent arc index";
            return KS_E_DEVICE;
        }
        const size_t j = std::min({jh, first_pair, jc});
        const std::string who = id_name(bv, "task", tasks[task_of(j)]) + ": ";
        if (j == jh) {
            err = who + "head " + std::to_string(arcs[j].dst) + " is not a live node that is no task (0, beyond the graph, "
                  "dead or a task)";
            return KS_E_INVALID;
        }
        if (j == first_pair) {
            err = who + "head " + std::to_string(arcs[j].dst) + " is listed twice: the list is the set of arcs the task "
                  "should have";
            return KS_E_INVALID;
        }
        err = who + "the cost of its arc into " + std::to_string(arcs[j].dst) + " is outside the supported range";
        return KS_E_RANGE;
    }
    if (h.bad_multi || h.bad_none) {
        size_t im, in;
        if (!first_bad(h.bad_multi, k, &im) || !first_bad(h.bad_none, k, &in)) {
            err = "inconsistent task index";
            return KS_E_DEVICE;
        }
        const bool multi = im <= in;
        const uint64_t id = tasks[multi ? im : in];
        err = multi ? id_name(bv, "task", id) + " would have arcs into two unscheduled aggregators: a task does not "
                      "change its job"
                    : id_name(bv, "task", id) + " is unbound and would have no arc into a node with an arc into the "
                      "sink; an aggregator whose capacity fell to 0 has lost that arc: pass the aggregators' ids "
                      "(unsched_ids)";
        return KS_E_INVALID;
    }
    if (a.cell_sink && ha.bad_sink) return sink_refusal(bv, ha.bad_sink, nst, err);
    if (h.units && a.sink < 0 && !a.cell_sink) {
        err = "an unscheduled aggregator's capacity needs exactly one sink";
        return KS_E_INVALID;
    }
    if (h.units < 0 || h.n_cost < 0 || h.n_same < 0 || h.n_run < 0 || h.n_del < 0 || h.rec_add < 0 ||
        (int64_t)h.rec_add + h.n_cost + h.n_same + h.n_run != (int64_t)na || h.n_cost + h.n_del != h.rec_held ||
        h.rec_held > hi || h.units > h.rec_add || (!walk && h.n_del) || ha.rec_upd < 0 || ha.rec_add < 0 ||
        ha.rec_upd + ha.rec_add != ha.rec_agg || ha.rec_agg > h.units || (h.units > 0) != (ha.rec_agg > 0)) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    const int64_t nrec = (int64_t)h.rec_held + h.rec_add + ha.rec_agg;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->tasks = (int64_t)k;
        stats->arcs_added = h.rec_add;
        stats->cost_updates = h.n_cost;
        stats->arcs_unchanged = h.n_same;
        stats->running_kept = h.n_run;
        stats->arcs_removed = h.n_del;
        stats->unsched_updates = ha.rec_upd;
        stats->unsched_added = ha.rec_add;
        stats->records = nrec;
    }
    if (!nrec) return KS_OK;   // every list is what the store holds: the solution stands
    // ---- 2. room for the new arcs
    rc = ensure_arcs(s, (int64_t)hi + h.rec_add + ha.rec_add, err);
    if (rc == KS_OK) rc = ensure_hash(s, (int64_t)h.rec_add + ha.rec_add, err);
    if (rc == KS_OK) rc = size_stream(s, nrec, 0, err);
    if (rc) return rc;
    // from here on a failure leaves the device state unknown
    *dirty = true;
    d = s.schd();   // (the arc table may have moved)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 3. the records, at their fixed positions, and the apply
    KS_CHECK(sched_upd_emit(d, u, h.rec_held, s.d_recs.p, st));
    KS_CHECK(sched_add_emit_aggs(d, a, (int64_t)h.rec_held + h.rec_add, s.d_recs.p, st));
    rc = apply_stream(s, nrec, {}, true, err);
    if (rc) return rc;
    if (log) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "update: %zu tasks, %zu arcs, %lld records, upload + checks + diff %.3f ms, sizing %.3f ms, "
                     "emit + apply %.3f ms\n",
                     k, na, (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3));
    }
    *changed = true;
    return KS_OK;
}

// ks_update_nodes: the eighth body. The ids, the offsets and the 24-byte arcs go up; one lane per
// id checks and claims it, one lane per listed arc checks its head against its tail's type, asks
// the store's index for the arc's slot and takes its row of the table, the type-0 tails' segments
// give the held arcs nobody listed (with KS_NODES_KEEP_UNLISTED no segment is read and no CSR is
// needed), and ONE host sync brings every refusal and the record counts (no step before it writes
// anything but scratch). Over the arc slots there is one flag array and its scan; everything else
// is per tail, per listed arc or per chunk position. Then the sizing of the arc table and the
// index, and the records on held arcs (ascending arc slot) and the new arcs (input order) reach
// store_apply as one stream. No node is edited. Under a view (ks_batch_update_nodes) the tails are
// the union's already and the heads leave their graphs' numbering in one launch before the checks.
int Engine::update_nodes(int flags, const uint64_t* nodes, size_t k, const uint64_t* arc_off, const ks_node_arc* arcs,
                         size_t first_pair, size_t first_cost, size_t first_cap, ks_node_stats* stats, bool* dirty,
                         bool* changed, std::string& err, const BatchView* bv) {
    EngineImpl& s = *p_;
    *dirty = *changed = false;
    if (!k) return KS_OK;
    KS_CHECK(hipSetDevice(s.device));
    hipStream_t st = s.stream;
    const bool walk = !(flags & KS_NODES_KEEP_UNLISTED);
    int rc = walk ? fresh_csr(s, err) : KS_OK;   // the chunk items walk the residual CSR
    if (rc) return rc;
    const bool log = s.opts.log_cycles != 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t nst = s.nstore;
    const int hi = s.hi();
    const size_t na = (size_t)arc_off[k];
    if (k > (size_t)INT32_MAX / 4 || na > (size_t)INT32_MAX / 4) {
        err = "too many nodes or arcs";
        return KS_E_RANGE;
    }
    NodDev u{};
    u.k = (int)k;
    u.na = (int)na;
    u.hi = hi;
    u.keep = walk ? 0 : 1;
    u.nst = nst;
    unsigned long long *d_nodes = nullptr, *d_off = nullptr, *d_arcs = nullptr;
    unsigned long long *d_goff = nullptr, *d_base = nullptr;
    rc = carve_scratch(s, [&](Carve<int>& ci, Carve<unsigned long long>& cu) {
        u.n_own = ci.take(nst + 1);
        for (int** x : {&u.n_slot, &u.nch, &u.ch_off}) *x = ci.take((int64_t)k + 1);
        for (int** x : {&u.l_slot, &u.lflag, &u.l_off}) *x = ci.take((int64_t)na + 1);
        for (int** x : {&u.sflag, &u.s_off}) *x = ci.take((int64_t)hi + 1);
        d_nodes = cu.take(k);
        d_off = cu.take(k + 1);
        d_arcs = cu.take(3 * na);
        d_goff = cu.take(bv ? bv->ng + 1 : 0);
        d_base = cu.take(bv ? bv->ng + 1 : 0);
    }, 0, false, err);
    if (rc) return rc;
    KS_CHECK(clear_ctl(s.nod_ctl, st));
    u.ctl = s.nod_ctl.p;
    u.nodes = d_nodes;
    u.arc_off = d_off;
    u.arcs = (const ks_node_arc*)d_arcs;
    wire_hash(s, u);
    KS_CHECK(hipMemcpyAsync(d_nodes, nodes, k * 8, hipMemcpyHostToDevice, st));
    KS_CHECK(hipMemcpyAsync(d_off, arc_off, (k + 1) * 8, hipMemcpyHostToDevice, st));
    if (na) KS_CHECK(hipMemcpyAsync(d_arcs, arcs, na * sizeof(ks_node_arc), hipMemcpyHostToDevice, st));
    SchedDev d = s.schd();
    const int ni_max = (int)(k + s.m2cap / 64 + 1);
    rc = bv && na ? translate_heads<ks_node_arc>(s, *bv, d_goff, d_base, d_arcs, na, &u.ctl->bad_range, err) : KS_OK;
    if (rc) return rc;
    // ---- 1. ids, heads, the diff and the unlisted arcs: one sync
    KS_CHECK(sched_nod_check(d, u, walk, st));
    if (walk) {
        KS_CHECK(exclusive_sum(s, (const int*)u.nch, u.ch_off, (int64_t)k + 1, st));
        KS_CHECK(sched_nod_unlisted(d, u, ni_max, st));
    }
    hipcub::TransformInputIterator<int, NodRecord, const int*> is_rec(u.sflag, NodRecord());
    KS_CHECK(exclusive_sum(s, is_rec, u.s_off, (int64_t)hi + 1, st));
    KS_CHECK(exclusive_sum(s, (const int*)u.lflag, u.l_off, (int64_t)na + 1, st));
    KS_CHECK(sched_nod_totals(u, st));
    NodCtl h{};
    KS_CHECK(hipMemcpyAsync(&h, u.ctl, sizeof(NodCtl), hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    auto tail_of = [&](size_t j) {   // the last i with arc_off[i] ≤ j
        return (size_t)(std::upper_bound(arc_off, arc_off + k, (uint64_t)j) - arc_off) - 1;
    };
    if (bv && h.bad_range) return range_refusal(*bv, h.bad_range, "node", nodes, arc_off, k, arcs, na, err);
    if (h.bad_node) {
        size_t i;
        if (!first_bad(h.bad_node, k, &i)) {
            err = "inconsistent node index";
            return KS_E_DEVICE;
        }
        err = id_name(bv, "node", nodes[i]) + " is not a live class, machine, intermediate or PU node listed once "
              "(0, beyond the graph, dead, a task, a sink, or listed before)";
        return KS_E_INVALID;
    }
    // the first offending arc in input order; on one arc the head, the repeat, the cost, then the capacity
    if (h.bad_head || std::min({first_pair, first_cost, first_cap}) < na) {
        size_t jh;
        if (!first_bad(h.bad_head, na, &jh)) {
            err = "inconsistent arc index";
            return KS_E_DEVICE;
        }
        const size_t j = std::min({jh, first_pair, first_cost, first_cap});
        const std::string who = id_name(bv, "node", nodes[tail_of(j)]) + ": ";
        const std::string head = std::to_string(arcs[j].dst);
        if (j == jh) {
            err = who + "head " + head + " is not a legal head (0, beyond the graph, dead, a task or the tail itself; a "
                  "PU's only head is a sink, and only a PU or a type-0 node has an arc into a sink)";
            return KS_E_INVALID;
        }
        if (j == first_pair) {
            err = who + "head " + head + " is listed twice: the list is the set of arcs the node should have";
            return KS_E_INVALID;
        }
        err = who + (j == first_cost ? "the cost" : "the capacity") + " of its arc into " + head +
              " is outside the supported range";
        return KS_E_RANGE;
    }
    // then the store's answers: KS_CAP_KEEP on an arc it does not hold, a capacity below a lower bound
    if (h.bad_keep || h.bad_low) {
        size_t jk, jl;
        if (!first_bad(h.bad_keep, na, &jk) || !first_bad(h.bad_low, na, &jl)) {
            err = "inconsistent arc index";
            return KS_E_DEVICE;
        }
        const size_t j = std::min(jk, jl);
        const std::string who = id_name(bv, "node", nodes[tail_of(j)]) + ": ";
        if (j == jk) {
            err = who + "KS_CAP_KEEP on its arc into " + std::to_string(arcs[j].dst) + ", which the store does not hold: "
                  "there is no capacity to keep";
            return KS_E_INVALID;
        }
        err = who + "the capacity of its arc into " + std::to_string(arcs[j].dst) + " would fall below the arc's lower bound";
        return KS_E_VERIFY;
    }
    if (h.n_add < 0 || h.n_upd < 0 || h.n_same < 0 || h.n_skip < 0 || h.n_zero < 0 || h.n_del < 0 ||
        (int64_t)h.n_add + h.n_upd + h.n_same + h.n_skip + h.n_zero != (int64_t)na || h.rec_add != h.n_add ||
        h.n_upd + h.n_zero + h.n_del != h.rec_held || h.rec_held > hi || (!walk && h.n_del)) {
        err = "inconsistent record counts";
        return KS_E_DEVICE;
    }
    const int64_t nrec = (int64_t)h.rec_held + h.rec_add;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->nodes = (int64_t)k;
        stats->arcs_added = h.n_add;
        stats->arcs_updated = h.n_upd;
        stats->arcs_unchanged = h.n_same;
        stats->arcs_skipped = h.n_skip;
        stats->arcs_zeroed = h.n_zero;
        stats->arcs_removed = h.n_del;
        stats->records = nrec;
    }
    if (!nrec) return KS_OK;   // every list is what the store holds: the solution stands
    // ---- 2. room for the new arcs
    rc = ensure_arcs(s, (int64_t)hi + h.rec_add, err);
    if (rc == KS_OK) rc = ensure_hash(s, (int64_t)h.rec_add, err);
    if (rc == KS_OK) rc = size_stream(s, nrec, 0, err);
    if (rc) return rc;
    // from here on a failure leaves the device state unknown
    *dirty = true;
    d = s.schd();   // (the arc table may have moved)
    const auto t2 = std::chrono::steady_clock::now();
    // ---- 3. the records, at their fixed positions, and the apply
    KS_CHECK(sched_nod_emit(d, u, walk && h.n_del, ni_max, h.rec_held, s.d_recs.p, st));
    rc = apply_stream(s, nrec, {}, true, err);
    if (rc) return rc;
    if (log) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr,
                     "nodes: %zu nodes, %zu arcs, %lld records, upload + checks + diff %.3f ms, sizing %.3f ms, "
                     "emit + apply %.3f ms\n",
                     k, na, (long long)nrec, ms(t0, t1), ms(t1, t2), ms(t2, t3));
    }
    *changed = true;
    return KS_OK;
}

int Engine::get_bindings(const uint64_t* task, uint64_t* pu, size_t k, std::string& err) {
    EngineImpl& s = *p_;
    KS_CHECK(hipSetDevice(s.device));
    if (!k) return KS_OK;
    for (size_t i = 0; i < k; ++i)
        if (task[i] == 0 || (int64_t)task[i] > s.nstore) {
            err = "binding of a task id beyond the graph";
            return KS_E_INVALID;
        }
    KS_CHECK(s.sched_u.ensure(2 * k));
    hipStream_t st = s.stream;
    KS_CHECK(hipMemcpyAsync(s.sched_u.p, task, k * 8, hipMemcpyHostToDevice, st));
    KS_CHECK(sched_gather_bindings(s.schd(), s.sched_u.p, (int)k, s.sched_u.p + k, st));
    KS_CHECK(hipMemcpyAsync(pu, s.sched_u.p + k, k * 8, hipMemcpyDeviceToHost, st));
    KS_CHECK(hipStreamSynchronize(st));
    return KS_OK;
}

}  // namespace ks
