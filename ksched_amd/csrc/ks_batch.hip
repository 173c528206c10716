// ks_batch.hip — config 5 behind the C-ABI: independent cell graphs sharded over
// GPUs, solved concurrently, and their task→PU mappings gathered to rank 0 over
// RCCL inside libksmcmf (SURVEY §7 step 6, §8 row e).
//
// A single solve does not shard, so multi-GPU throughput comes
// from independent graphs (cluster cells, what-if variants). Graph g belongs to
// global rank g mod world (round-robin); each device solves the
// disjoint union of its graphs as ONE device solve (the min-cost flow of a
// disjoint union is the union of the optima). After the solves every device
// packs one row per graph — [cost, flow value, PU id of each task (cell-local,
// 0 = unscheduled)] — and rank 0 receives every device's rows with
// ncclSend/ncclRecv in one group: a single collective, no data-path exchange.
// Two ways to build the communicator: ks_batch_create (one process, several
// devices: ncclCommInitAll) and ks_batch_create_rank (one process per GPU, e.g.
// under torch.distributed.run: ncclCommInitRank with an id from rank 0).
// RCCL is loaded with dlopen on the first batch (the single-graph API never
// needs it); a process that already holds RCCL (torch) shares its copy.
// A TEST build of the library (-DKS_FAKE_COMM: libksmcmf_fakecomm.so, made by
// ksched_amd/_build.py build_fake_comm, never the shipped libksmcmf.so) binds the
// same entry points to tests/fake_comm/fake_nccl.cpp compiled into it instead —
// the ranks of one process on one GPU — so the world > 1 path of ks_batch_gather
// runs on a one-GPU box.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#ifdef KS_FAKE_COMM
extern "C" {
ncclResult_t ks_fake_ncclGetUniqueId(ncclUniqueId*);
ncclResult_t ks_fake_ncclCommInitAll(ncclComm_t*, int, const int*);
ncclResult_t ks_fake_ncclCommInitRank(ncclComm_t*, int, ncclUniqueId, int);
ncclResult_t ks_fake_ncclCommDestroy(ncclComm_t);
ncclResult_t ks_fake_ncclGroupStart();
ncclResult_t ks_fake_ncclGroupEnd();
ncclResult_t ks_fake_ncclSend(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ks_fake_ncclRecv(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ks_fake_ncclAllReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
const char* ks_fake_ncclGetErrorString(ncclResult_t);
}
#endif

#include "ks_ctx.h"

namespace {

struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                              hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;

    bool load(std::string& err) {
        if (h) return true;
#ifdef KS_FAKE_COMM
        GetUniqueId = ks_fake_ncclGetUniqueId;
        CommInitAll = ks_fake_ncclCommInitAll;
        CommInitRank = ks_fake_ncclCommInitRank;
        CommDestroy = ks_fake_ncclCommDestroy;
        GroupStart = ks_fake_ncclGroupStart;
        GroupEnd = ks_fake_ncclGroupEnd;
        Send = ks_fake_ncclSend;
        Recv = ks_fake_ncclRecv;
        AllReduce = ks_fake_ncclAllReduce;
        GetErrorString = ks_fake_ncclGetErrorString;
        h = this;
        (void)err;
        return true;
#endif
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) {
            err = std::string("RCCL not found: ") + dlerror();
            return false;
        }
        bool ok = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            ok = ok && fn;
        };
        sym(GetUniqueId, "ncclGetUniqueId");
        sym(CommInitAll, "ncclCommInitAll");
        sym(CommInitRank, "ncclCommInitRank");
        sym(CommDestroy, "ncclCommDestroy");
        sym(GroupStart, "ncclGroupStart");
        sym(GroupEnd, "ncclGroupEnd");
        sym(Send, "ncclSend");
        sym(Recv, "ncclRecv");
        sym(AllReduce, "ncclAllReduce");
        sym(GetErrorString, "ncclGetErrorString");
        if (!ok) err = "RCCL is missing a symbol";
        return ok;
    }
};

// RCCL, loaded on first use (the test build: the fake in-process ranks)
Rccl* comm_lib(std::string& err) {
    static Rccl r;
    return r.load(err) ? &r : nullptr;
}

// ---- row layout of ks_batch_gather (host code, shared by the packing, the
// unpacking and the CPU tests through the exported ks_batch_* layout calls) ----
// Graph g lives on global rank g mod world, as that rank's (g div world)-th
// graph. Every rank sends ONE block: [status word][slots rows], a row being
// [cost, flow value, PU id of each task (cell-local, 0 = unscheduled), padded to
// max_tasks]. Rank 0 receives the blocks in rank order.
inline size_t kb_slots(size_t ngraphs, int world) { return (ngraphs + (size_t)world - 1) / (size_t)std::max(1, world); }
inline size_t kb_rowlen(size_t max_tasks) { return 2 + max_tasks; }
inline size_t kb_block(size_t ngraphs, int world, size_t max_tasks) {
    return 1 + std::max<size_t>(1, kb_slots(ngraphs, world)) * kb_rowlen(max_tasks);
}
inline size_t kb_row_in_block(size_t slot, size_t max_tasks) { return 1 + slot * kb_rowlen(max_tasks); }

// row r: PU ids of its tasks made cell-local (subtract the cell's node offset)
__global__ void k_localize(int rows, int rowlen, const long long* __restrict__ off, long long* __restrict__ buf) {
    const int r = blockIdx.y;
    if (r >= rows) return;
    long long* row = buf + 1 + (size_t)r * rowlen;
    for (int i = 2 + blockIdx.x * blockDim.x + threadIdx.x; i < rowlen; i += gridDim.x * blockDim.x)
        if (row[i] > 0) row[i] -= off[r];
}

// ---- a graph's delta stream inside its id range (host code: ks_batch_translate_deltas
// and the error message of ks_batch_apply_deltas) ----
inline bool kb_arc_kind(int32_t kind) { return kind == KS_ADD_ARC || kind == KS_UPDATE_ARC; }
inline bool kb_node_kind(int32_t kind) { return kind == KS_ADD_NODE || kind == KS_REMOVE_NODE || kind == KS_SET_EXCESS; }
// the id of record x that lies outside 1..span, 0 when none does (*any: whether one does)
inline uint64_t kb_bad_id(const ks_delta& x, uint64_t span, bool* any) {
    auto out = [&](uint64_t id) { return id == 0 || id > span; };
    *any = true;
    if (kb_arc_kind(x.kind)) {
        if (out(x.src)) return x.src;
        if (out(x.dst)) return x.dst;
    } else if (kb_node_kind(x.kind) && out(x.id)) {
        return x.id;
    }
    *any = false;
    return 0;
}
// the first record with an id outside 1..span (k: none)
inline size_t kb_first_bad(const ks_delta* in, size_t k, uint64_t span) {
    for (size_t i = 0; i < k; ++i) {
        bool any = false;
        kb_bad_id(in[i], span, &any);
        if (any) return i;
    }
    return k;
}

}  // namespace

struct ks_batch {
    struct Local {
        int device = 0;
        int grank = 0;                  // global rank
        ks_ctx* ctx = nullptr;
        ncclComm_t comm = nullptr;
        std::vector<int> graphs;        // graph ids solved here, in order
        std::vector<int64_t> off;       // node-id offset of each graph in the union (+ total)
        std::vector<int64_t> toff;      // task offset of each graph in the dense task vector (+ total)
        long long* rows = nullptr;      // device: graphs.size() × rowlen
        long long* scratch = nullptr;   // device: dense task→PU vector, offsets
        long long* stat = nullptr;      // device: this rank's status word for the status all-reduce
        size_t rows_cap = 0, scratch_cap = 0;
        ks_result res{};
    };
    std::vector<Local> loc;
    const Rccl* nccl = nullptr;         // the communication library behind this batch
    int world = 1;
    size_t ngraphs = 0;
    std::string err;
    long long* root_buf = nullptr;      // rank 0: world × slots × rowlen
    size_t root_cap = 0;
    size_t spare = 0;                   // ks_batch_reserve: ids each graph may grow by (read by the next load)
    int fault_pack = 0;                 // TESTS ONLY (ks_opts.fault_inject bit 2): global rank + 1 whose packing fails
    int fault_root = 0;                 // TESTS ONLY (ks_opts.fault_inject bit 3): rank 0's receive buffer allocation fails

    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace {

#define KB_HIP(expr)                                                          \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return b->fail(KS_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

ks_batch* make_batch(const Rccl* api, int world, const ks_opts* opts, const std::vector<std::pair<int, int>>& dev_rank) {
    ks_batch* b = new (std::nothrow) ks_batch;
    if (!b) return nullptr;
    b->nccl = api;
    b->world = world;
    b->fault_pack = (opts && (opts->fault_inject & 4)) ? 1 : 0;   // TESTS ONLY: global rank 0's packing fails
    b->fault_root = (opts && (opts->fault_inject & 8)) ? 1 : 0;   // TESTS ONLY: rank 0's root buffer allocation fails
    for (auto [dev, rank] : dev_rank) {
        ks_batch::Local l;
        l.device = dev;
        l.grank = rank;
        l.ctx = ks_create(dev, opts);
        // the status word of the gather's all-reduce exists before any gather, so a
        // rank can always enter that collective
        if (!l.ctx || hipSetDevice(dev) != hipSuccess || hipMalloc(&l.stat, sizeof(long long)) != hipSuccess) {
            if (l.ctx) ks_destroy(l.ctx);
            for (auto& x : b->loc) {
                if (x.stat) (void)hipFree(x.stat);
                ks_destroy(x.ctx);
            }
            delete b;
            return nullptr;
        }
        b->loc.push_back(std::move(l));
    }
    return b;
}

// The local device that owns graph g and g's index among its graphs (nullptr: another rank's).
ks_batch::Local* owner_of(ks_batch* b, size_t g, size_t* idx) {
    if (g >= b->ngraphs) return nullptr;
    int r = 0;
    size_t slot = 0;
    ks_batch_owner(g, b->world, &r, &slot);
    for (auto& l : b->loc)
        if (l.grank == r && slot < l.graphs.size()) {
            *idx = slot;
            return &l;
        }
    return nullptr;
}

// The gather's task offsets from the host node table: row i of a graph stays "its i-th
// live task in id order" after tasks arrive and complete.
void recompute_toff(ks_batch::Local& l) {
    const std::vector<NodeRec>& nodes = l.ctx->nodes;
    l.toff.assign(1, 0);
    for (size_t i = 0; i + 1 < l.off.size(); ++i) {
        int64_t tasks = 0;
        const uint64_t hi = std::min<uint64_t>((uint64_t)l.off[i + 1], nodes.size() ? nodes.size() - 1 : 0);
        for (uint64_t id = (uint64_t)l.off[i] + 1; id <= hi; ++id)
            tasks += nodes[id].alive && nodes[id].type == KS_NODE_TASK;
        l.toff.push_back(l.toff.back() + tasks);
    }
}

// Per-graph auto_sink (graph_manager.go:640, 808, per cell): graph i of l as it will
// stand after its stream u[at..) (union ids) — when it then has exactly one sink whose
// supply is not −Σ of its other nodes' supplies, the SET_EXCESS record that makes it so
// is appended to u. A graph with no sink or several is left alone.
void append_auto_sink(const ks_batch::Local& l, size_t i, std::vector<ks_delta>& u, size_t at) {
    const std::vector<NodeRec>& nodes = l.ctx->nodes;
    const uint64_t lo = (uint64_t)l.off[i], hi = (uint64_t)l.off[i + 1];
    // the node records of the stream over the table (ids past the table are dead)
    std::vector<NodeRec> now(hi - lo + 1);
    for (uint64_t id = lo + 1; id <= hi; ++id)
        if (id < nodes.size()) now[id - lo] = nodes[id];
    for (size_t j = at; j < u.size(); ++j) {
        const ks_delta& x = u[j];
        if (!kb_node_kind(x.kind) || x.id <= lo || x.id > hi) continue;
        NodeRec& r = now[x.id - lo];
        if (x.kind == KS_ADD_NODE) r = NodeRec{x.excess, x.type, true, true};
        else if (x.kind == KS_REMOVE_NODE) r = NodeRec{};
        else if (r.alive) r.excess = x.excess;
    }
    int64_t sinks = 0, others = 0;
    uint64_t sink = 0;
    for (uint64_t id = lo + 1; id <= hi; ++id) {
        const NodeRec& r = now[id - lo];
        if (!r.alive) continue;
        if (r.type == KS_NODE_SINK) {
            ++sinks;
            sink = id;
        } else {
            others += r.excess;
        }
    }
    if (sinks != 1 || now[sink - lo].excess == -others) return;
    ks_delta d;
    std::memset(&d, 0, sizeof(d));
    d.kind = KS_SET_EXCESS;
    d.id = sink;
    d.excess = -others;
    u.push_back(d);
}

// The index among l's graphs of the graph that owns union id `id`: graph i owns (off[i], off[i+1]]
// (an id past the last graph is the last graph's; 0 when off holds no graph).
size_t graph_index(const ks_batch::Local& l, uint64_t id) {
    size_t i = (size_t)(std::lower_bound(l.off.begin(), l.off.end(), (int64_t)id) - l.off.begin());
    i = i ? i - 1 : 0;
    return std::min(i, l.off.size() >= 2 ? l.off.size() - 2 : 0);
}

template <class Stats>
void add_stats(Stats& sum, const Stats& st) {
    static_assert(sizeof(Stats) % sizeof(int64_t) == 0, "stats are int64 counters");
    for (size_t w = 0; w < sizeof(Stats) / sizeof(int64_t); ++w)
        reinterpret_cast<int64_t*>(&sum)[w] += reinterpret_cast<const int64_t*>(&st)[w];
}

// A commit's deltas of one device (union ids, the order of ks_scheduling_deltas) as
// ks_batch_delta records in graph-local ids.
void localize_deltas(const ks_batch::Local& l, const std::vector<ks_sched_delta>& v, std::vector<ks_batch_delta>& out) {
    for (const ks_sched_delta& x : v) {
        const size_t i = graph_index(l, x.task);
        const uint64_t base = (uint64_t)l.off[i];
        out.push_back(ks_batch_delta{x.type, l.graphs.empty() ? 0 : l.graphs[i], x.task - base, x.pu ? x.pu - base : 0});
    }
}

// Both batch commits: count over the local devices first (a cap that is too small
// changes nothing), then commit device by device, and the deltas grouped by graph.
template <class Stats, class Call>
int batch_commit(ks_batch* b, ks_batch_delta* out, size_t cap, size_t* count, Stats* stats, Call call) {
    if (!b || !count) return KS_E_INVALID;
    std::vector<size_t> n(b->loc.size(), 0);
    size_t total = 0;
    for (size_t li = 0; li < b->loc.size(); ++li) {
        const int rc = call(b->loc[li].ctx, nullptr, 0, &n[li], nullptr);
        if (rc) return b->fail(rc, ks_last_error(b->loc[li].ctx));
        total += n[li];
    }
    *count = total;
    if (!out) return KS_OK;
    if (cap < total) return b->fail(KS_E_INVALID, "output buffer smaller than the delta count");
    Stats sum;
    std::memset(&sum, 0, sizeof(sum));
    std::vector<ks_batch_delta> all;
    for (size_t li = 0; li < b->loc.size(); ++li) {
        auto& l = b->loc[li];
        std::vector<ks_sched_delta> v(std::max<size_t>(n[li], 1));
        Stats st;
        std::memset(&st, 0, sizeof(st));
        size_t got = 0;
        const int rc = call(l.ctx, v.data(), n[li], &got, &st);
        if (rc) return b->fail(rc, ks_last_error(l.ctx));
        v.resize(got);
        localize_deltas(l, v, all);
        add_stats(sum, st);
        recompute_toff(l);
    }
    // grouped by graph, ascending; within a graph the order of ks_scheduling_deltas
    std::stable_sort(all.begin(), all.end(),
                     [](const ks_batch_delta& x, const ks_batch_delta& y) { return x.graph < y.graph; });
    if (!all.empty()) std::memcpy(out, all.data(), all.size() * sizeof(ks_batch_delta));
    *count = all.size();
    if (stats) *stats = sum;
    return KS_OK;
}

// ---- what the round calls share: the checks of the per-graph lists, a graph's ids into the
// union's numbering, a device's view of its union, and the one lone call per device ----

// One list per loaded graph.
int check_list_array(ks_batch* b, size_t ngraphs, const void* lists) {
    if (ngraphs != b->ngraphs) return b->fail(KS_E_INVALID, "the list count differs from the loaded graphs");
    if (ngraphs && !lists) return b->fail(KS_E_INVALID, "null list array");
    return KS_OK;
}

std::string in_graph(size_t g) { return "graph " + std::to_string(g) + ": "; }

// Graph g's list of k ids (what: their noun) with arc_off[k + 1] into its arcs.
int check_offsets(ks_batch* b, size_t g, size_t k, const uint64_t* arc_off, const uint64_t* ids, bool null_arcs,
                  const char* what) {
    if (arc_off[0] != 0) return b->fail(KS_E_INVALID, in_graph(g) + "arc_off[0] must be 0");
    for (size_t i = 0; i < k; ++i)
        if (arc_off[i + 1] < arc_off[i])
            return b->fail(KS_E_INVALID, in_graph(g) + "arc_off decreases at " + what + " " + std::to_string(ids[i]));
    if (arc_off[k] && null_arcs) return b->fail(KS_E_INVALID, in_graph(g) + "null arc array");
    if (arc_off[k] > (uint64_t)INT32_MAX / 4) return b->fail(KS_E_RANGE, in_graph(g) + "too many arcs");
    return KS_OK;
}

int outside_ids(ks_batch* b, size_t g, const char* what, uint64_t id, uint64_t span) {
    return b->fail(KS_E_RANGE, in_graph(g) + what + " " + std::to_string(id) + " is outside the graph's ids 1.." +
                                   std::to_string(span) + " (its highest id at the load plus the reserved ids)");
}

uint64_t span_of(const ks_batch::Local& l, size_t i) { return (uint64_t)(l.off[i + 1] - l.off[i]); }

// k ids of l's graph i (what: their noun) in the union's numbering, appended to out: the O(k) part
// of a call, which the node table needs anyway. One outside 1..span of its graph is KS_E_RANGE.
int to_union(ks_batch* b, const ks_batch::Local& l, size_t i, const char* what, const uint64_t* ids, size_t k,
             std::vector<uint64_t>& out) {
    const uint64_t lo = (uint64_t)l.off[i], span = span_of(l, i);
    for (size_t j = 0; j < k; ++j) {
        if (ids[j] == 0 || ids[j] > span) return outside_ids(b, (size_t)l.graphs[i], what, ids[j], span);
        out.push_back(ids[j] + lo);
    }
    return KS_OK;
}

// A graph's k offsets and the arcs behind them appended to a union's: the offsets rebased, the
// arcs as the caller wrote them.
template <class Arc>
void append_arcs(std::vector<uint64_t>& union_off, std::vector<Arc>& union_arcs, size_t k, const uint64_t* arc_off,
                 const Arc* arcs) {
    const uint64_t at = union_off.back();
    for (size_t j = 1; j <= k; ++j) union_off.push_back(at + arc_off[j]);
    if (arc_off[k]) union_arcs.insert(union_arcs.end(), arcs, arcs + arc_off[k]);
}

// How the lone call addresses l's graphs: arc_goff (and node_goff, where the call has one) hold
// the first listed record of each graph (+ the total).
void wire_view(ks::BatchView& v, const ks_batch::Local& l, const std::vector<uint64_t>& arc_goff,
               const std::vector<uint64_t>* node_goff = nullptr) {
    v.ng = l.graphs.size();
    v.off = l.off.data();
    v.graph = l.graphs.data();
    v.arc_goff = arc_goff.data();
    v.node_goff = node_goff ? node_goff->data() : nullptr;
}

// ONE lone call per local device on its union input us[li], after every list passed the checks of
// every local device. want(l, u): whether the device is called at all; call(l, u, &st): the lone
// call, under the view that lets its messages name graphs; after(l, u): what follows a call that
// succeeded. A failure of either is the rank's, with the device's message. stats: the sum over
// the devices, zero from the start and whole at the end.
template <class Stats, class Union, class Want, class Call, class After>
int each_device(ks_batch* b, std::vector<Union>& us, Stats* stats, Want want, Call call, After after) {
    Stats sum;
    std::memset(&sum, 0, sizeof(sum));
    if (stats) *stats = sum;
    for (size_t li = 0; li < b->loc.size(); ++li) {
        ks_batch::Local& l = b->loc[li];
        if (!want(l, us[li])) continue;
        Stats st;
        std::memset(&st, 0, sizeof(st));
        l.ctx->view = &us[li].view;
        int rc = call(l, us[li], &st);
        l.ctx->view = nullptr;
        if (rc == KS_OK) rc = after(l, us[li]);
        if (rc) return b->fail(rc, "rank " + std::to_string(l.grank) + ": " + ks_last_error(l.ctx));
        add_stats(sum, st);
    }
    if (stats) *stats = sum;
    return KS_OK;
}
const auto nothing_after = [](ks_batch::Local&, const auto&) { return (int)KS_OK; };

// ---- the task side of a round: one device's part of ks_batch_add_tasks, _complete_tasks,
// _update_tasks. Its graphs' lists lie back to back in graph order: the task and aggregator
// ids in the union's numbering (the O(k) part, which the node table needs anyway), the arcs as
// the caller wrote them: their heads leave the graph's numbering on the device (BatchView).
struct UnionLists {
    std::vector<uint64_t> tasks, arc_off, agg;
    std::vector<uint64_t> task_goff, arc_goff;   // per graph of the device (+ total): its first task, its first arc
    std::vector<ks_task_arc> arcs;
    std::vector<size_t> touched;                 // the listed graphs, as indices into Local::graphs
    bool explicit_ids = false;                   // the listed graphs pass their aggregators (else the NULL rule)
    ks::BatchView view;
    const uint64_t* agg_ptr() const {            // (an empty list names no aggregator: not NULL, which is the NULL rule)
        static const uint64_t none = 0;
        return !explicit_ids ? nullptr : agg.empty() ? &none : agg.data();
    }
};

// What every rank can check of all the lists, before any device is asked: the arrays, the
// offsets, and the one aggregator mode of the call.
int check_lists(ks_batch* b, size_t ngraphs, const ks_batch_task_list* lists, bool with_arcs) {
    if (int rc = check_list_array(b, ngraphs, lists)) return rc;
    int mode = -1;   // 1: the listed graphs pass unsched_ids, 0: none does
    for (size_t g = 0; g < ngraphs; ++g) {
        const ks_batch_task_list& L = lists[g];
        if (!L.k) continue;
        const std::string who = in_graph(g);
        if (!L.tasks) return b->fail(KS_E_INVALID, who + "null task array");
        if (L.k > (size_t)INT32_MAX / 4) return b->fail(KS_E_RANGE, who + "too many tasks");
        if (L.unsched_ids == nullptr && L.nu) return b->fail(KS_E_INVALID, who + "null aggregator array");
        const int m = L.unsched_ids ? 1 : 0;
        if (mode >= 0 && m != mode)
            return b->fail(KS_E_INVALID, who + "either every listed graph passes unsched_ids or none does (one rule per call)");
        mode = m;
        if (!with_arcs) continue;
        if (!L.arc_off) return b->fail(KS_E_INVALID, who + "null offset array");
        if (int rc = check_offsets(b, g, L.k, L.arc_off, L.tasks, !L.arcs, "task")) return rc;
    }
    return KS_OK;
}

// The lists of l's graphs as one union input. A task or an aggregator outside 1..span of its
// graph is KS_E_RANGE here (a head: on the device, before anything changes there).
int build_union(ks_batch* b, const ks_batch::Local& l, const ks_batch_task_list* lists, bool with_arcs, UnionLists& u) {
    u.task_goff.assign(1, 0);
    u.arc_goff.assign(1, 0);
    if (with_arcs) u.arc_off.assign(1, 0);
    for (size_t i = 0; i < l.graphs.size(); ++i) {
        const ks_batch_task_list& L = lists[(size_t)l.graphs[i]];
        if (L.k) {
            if (int rc = to_union(b, l, i, "task", L.tasks, L.k, u.tasks)) return rc;
            if (int rc = to_union(b, l, i, "unscheduled aggregator", L.unsched_ids, L.unsched_ids ? L.nu : 0, u.agg)) return rc;
            u.explicit_ids = L.unsched_ids != nullptr;
            if (with_arcs) {
                append_arcs(u.arc_off, u.arcs, L.k, L.arc_off, L.arcs);
                if (u.arcs.size() > (size_t)INT32_MAX / 4) return b->fail(KS_E_RANGE, "too many arcs on one device");
            }
            u.touched.push_back(i);
        }
        u.task_goff.push_back(u.tasks.size());
        u.arc_goff.push_back(u.arcs.size());
    }
    wire_view(u.view, l, u.arc_goff);
    return KS_OK;
}

// All three task calls: every list checked on every local device first, then ONE lone call
// per device on its union input (call(ctx, lists, left of the union's tasks, stats)), under the
// view that lets its messages name graphs. A device that changed gets its touched graphs'
// auto-sink records (supplies: tasks arrived or left) and its gather rows recounted, and
// the bindings it returned leave the union's numbering.
// every_device: a device whose graphs list nothing is called as well (the plain capacity refresh).
template <class Stats, class Call>
int batch_task_call(ks_batch* b, size_t ngraphs, const ks_batch_task_list* lists, bool with_arcs, bool supplies,
                    uint64_t* const* left, Stats* stats, Call call, bool every_device = false) {
    if (!b) return KS_E_INVALID;
    if (int rc = check_lists(b, ngraphs, lists, with_arcs)) return rc;
    std::vector<UnionLists> us(b->loc.size());
    for (size_t li = 0; li < b->loc.size(); ++li)
        if (int rc = build_union(b, b->loc[li], lists, with_arcs, us[li])) return rc;
    // the bindings the device being called returns, in the union's numbering: filled by a device's
    // call, read by its after-step, then reused for the next device (valid only between the two)
    std::vector<uint64_t> hl;
    return each_device(
        b, us, stats,
        [&](const ks_batch::Local& l, const UnionLists& u) { return !u.touched.empty() || (every_device && !l.graphs.empty()); },
        [&](ks_batch::Local& l, const UnionLists& u, Stats* st) {
            hl.assign(u.tasks.size(), 0);
            return call(l.ctx, u, hl.data(), st);
        },
        [&](ks_batch::Local& l, const UnionLists& u) {
            if (supplies && l.ctx->opts.auto_sink) {
                std::vector<ks_delta> sinks;
                for (size_t i : u.touched) append_auto_sink(l, i, sinks, sinks.size());
                if (!sinks.empty())
                    if (int rc = ks_apply_deltas(l.ctx, sinks.data(), sinks.size())) return rc;
            }
            if (supplies) recompute_toff(l);
            for (size_t i : u.touched) {
                uint64_t* out = left ? left[(size_t)l.graphs[i]] : nullptr;
                if (!out) continue;
                const uint64_t lo = (uint64_t)l.off[i];
                for (uint64_t j = u.task_goff[i]; j < u.task_goff[i + 1]; ++j) out[j - u.task_goff[i]] = hl[j] ? hl[j] - lo : 0;
            }
            return (int)KS_OK;
        });
}

// ---- the resource side of a round: one device's part of ks_batch_remove_resources (the roots in
// the union's numbering: O(k) on the host, which checks their range) and of ks_batch_add_resources
// (the two record arrays as the caller wrote them: their ids leave the graphs' numbering on the
// device, BatchView::node_goff / arc_goff). Everything is the call's input but nr and ne, which a
// removal's device call writes: its counts, kept here between the probing pass and the removing one.
struct UnionRes {
    std::vector<uint64_t> roots;
    std::vector<ks_res_node> nodes;
    std::vector<ks_res_arc> arcs;
    std::vector<uint64_t> node_goff, arc_goff;   // per graph of the device (+ total): its first node, its first edge
    bool touched = false;
    size_t nr = 0, ne = 0;                       // a removal: the nodes and the evictions the device counted
    ks::BatchView view;
};

int check_res_lists(ks_batch* b, size_t ngraphs, const ks_batch_res_list* lists, bool adding) {
    if (int rc = check_list_array(b, ngraphs, lists)) return rc;
    for (size_t g = 0; g < ngraphs; ++g) {
        const ks_batch_res_list& L = lists[g];
        const std::string who = in_graph(g);
        if (!adding && L.k && !L.roots) return b->fail(KS_E_INVALID, who + "null root array");
        if (adding && ((L.n && !L.nodes) || (L.m && !L.arcs))) return b->fail(KS_E_INVALID, who + "null node or edge array");
        if (L.k > (size_t)INT32_MAX / 16 || L.n > (size_t)INT32_MAX / 16 || L.m > (size_t)INT32_MAX / 16)
            return b->fail(KS_E_RANGE, who + "too many roots, resource nodes or edges");
    }
    return KS_OK;
}

// The lists of l's graphs as one union input. A root or a node id outside 1..span of its graph is
// KS_E_RANGE here (an edge's endpoint: on the device, before anything changes there).
int build_union_res(ks_batch* b, const ks_batch::Local& l, const ks_batch_res_list* lists, bool adding, UnionRes& u) {
    u.node_goff.assign(1, 0);
    u.arc_goff.assign(1, 0);
    for (size_t i = 0; i < l.graphs.size(); ++i) {
        const size_t g = (size_t)l.graphs[i];
        const ks_batch_res_list& L = lists[g];
        if (!adding) {
            if (int rc = to_union(b, l, i, "root", L.roots, L.k, u.roots)) return rc;
            u.touched |= L.k != 0;
        } else {
            for (size_t j = 0; j < L.n; ++j)
                if (L.nodes[j].id == 0 || L.nodes[j].id > span_of(l, i))
                    return outside_ids(b, g, "resource node id", L.nodes[j].id, span_of(l, i));
            if (L.n) u.nodes.insert(u.nodes.end(), L.nodes, L.nodes + L.n);
            if (L.m) u.arcs.insert(u.arcs.end(), L.arcs, L.arcs + L.m);
            if (u.nodes.size() > (size_t)INT32_MAX / 16 || u.arcs.size() > (size_t)INT32_MAX / 16)
                return b->fail(KS_E_RANGE, "too many resource nodes or edges on one device");
            u.touched |= L.n || L.m;
        }
        u.node_goff.push_back(u.nodes.size());
        u.arc_goff.push_back(u.arcs.size());
    }
    wire_view(u.view, l, u.arc_goff, &u.node_goff);
    return KS_OK;
}

// ---- class and resource arcs: one device's part of ks_batch_update_nodes. The tails in the
// union's numbering (O(k) on the host, which checks their range), the offsets rebased, the
// 24-byte arcs as the caller wrote them: their heads leave the graph's numbering on the device.
struct UnionNodes {
    std::vector<uint64_t> nodes, arc_off;
    std::vector<uint64_t> arc_goff;   // per graph of the device (+ total): its first arc
    std::vector<ks_node_arc> arcs;
    ks::BatchView view;
};

int check_node_lists(ks_batch* b, size_t ngraphs, const ks_batch_node_list* lists) {
    if (int rc = check_list_array(b, ngraphs, lists)) return rc;
    for (size_t g = 0; g < ngraphs; ++g) {
        const ks_batch_node_list& L = lists[g];
        if (!L.k) continue;
        if (!L.nodes || !L.arc_off) return b->fail(KS_E_INVALID, in_graph(g) + "null node or offset array");
        if (L.k > (size_t)INT32_MAX / 4) return b->fail(KS_E_RANGE, in_graph(g) + "too many nodes");
        if (int rc = check_offsets(b, g, L.k, L.arc_off, L.nodes, !L.arcs, "node")) return rc;
    }
    return KS_OK;
}

// The lists of l's graphs as one union input. A tail outside 1..span of its graph is KS_E_RANGE
// here (a head: on the device, before anything changes there).
int build_union_nodes(ks_batch* b, const ks_batch::Local& l, const ks_batch_node_list* lists, UnionNodes& u) {
    u.arc_goff.assign(1, 0);
    u.arc_off.assign(1, 0);
    for (size_t i = 0; i < l.graphs.size(); ++i) {
        const ks_batch_node_list& L = lists[(size_t)l.graphs[i]];
        if (L.k) {
            if (int rc = to_union(b, l, i, "node", L.nodes, L.k, u.nodes)) return rc;
            append_arcs(u.arc_off, u.arcs, L.k, L.arc_off, L.arcs);
            if (u.nodes.size() > (size_t)INT32_MAX / 4 || u.arcs.size() > (size_t)INT32_MAX / 4)
                return b->fail(KS_E_RANGE, "too many nodes or arcs on one device");
        }
        u.arc_goff.push_back(u.arcs.size());
    }
    wire_view(u.view, l, u.arc_goff);
    return KS_OK;
}

}  // namespace

extern "C" {

size_t ks_batch_slots(size_t ngraphs, int world) { return world < 1 ? 0 : kb_slots(ngraphs, world); }

int ks_batch_owner(size_t g, int world, int* rank, size_t* slot) {
    if (world < 1 || !rank || !slot) return KS_E_INVALID;
    *rank = (int)(g % (size_t)world);
    *slot = g / (size_t)world;
    return KS_OK;
}

size_t ks_batch_block_len(size_t ngraphs, int world, size_t max_tasks) {
    return world < 1 ? 0 : kb_block(ngraphs, world, max_tasks);
}

int ks_batch_unpack(const int64_t* gathered, size_t ngraphs, int world, size_t max_tasks, uint64_t* pu,
                    int64_t* cost, int64_t* flow) {
    if (!gathered || world < 1) return KS_E_INVALID;
    const size_t block = kb_block(ngraphs, world, max_tasks);
    for (int r = 0; r < world; ++r)
        if (gathered[(size_t)r * block] != 0) return (int)gathered[(size_t)r * block];   // a rank's status
    for (size_t g = 0; g < ngraphs; ++g) {
        int r = 0;
        size_t slot = 0;
        ks_batch_owner(g, world, &r, &slot);
        const int64_t* row = gathered + (size_t)r * block + kb_row_in_block(slot, max_tasks);
        if (cost) cost[g] = row[0];
        if (flow) flow[g] = row[1];
        if (pu) std::memcpy(pu + g * max_tasks, row + 2, max_tasks * sizeof(uint64_t));
    }
    return KS_OK;
}

int ks_batch_node_offsets(const uint64_t* maxid, size_t k, size_t spare, int64_t* off) {
    if (!off || (k && !maxid)) return KS_E_INVALID;
    off[0] = 0;
    for (size_t i = 0; i < k; ++i) off[i + 1] = off[i] + (int64_t)maxid[i] + (int64_t)spare;
    return KS_OK;
}

int ks_batch_translate_deltas(int64_t lo, int64_t hi, const ks_delta* in, size_t k, ks_delta* out) {
    if (lo < 0 || hi < lo || (k && (!in || !out))) return KS_E_INVALID;
    if (kb_first_bad(in, k, (uint64_t)(hi - lo)) < k) return KS_E_RANGE;   // before anything is written
    for (size_t i = 0; i < k; ++i) {
        ks_delta x = in[i];   // (a copy first: out may be in)
        if (kb_arc_kind(x.kind)) {
            x.src += (uint64_t)lo;
            x.dst += (uint64_t)lo;
        } else if (kb_node_kind(x.kind)) {
            x.id += (uint64_t)lo;
        }
        out[i] = x;
    }
    return KS_OK;
}

int ks_batch_unique_id(uint8_t* id) {
    std::string err;
    const Rccl* api = id ? comm_lib(err) : nullptr;
    if (!api) return KS_E_DEVICE;
    ncclUniqueId u;
    if (api->GetUniqueId(&u) != ncclSuccess) return KS_E_DEVICE;
    std::memcpy(id, u.internal, KS_UNIQUE_ID_BYTES);
    return KS_OK;
}

ks_batch* ks_batch_create(const int* devices, int ndev, const ks_opts* opts) {
    std::string err;
    const Rccl* api = devices && ndev >= 1 ? comm_lib(err) : nullptr;
    if (!api) return nullptr;
    std::vector<std::pair<int, int>> dr;
    for (int i = 0; i < ndev; ++i) dr.emplace_back(devices[i], i);
    ks_batch* b = make_batch(api, ndev, opts, dr);
    if (!b) return nullptr;
    std::vector<ncclComm_t> comms(ndev);
    if (api->CommInitAll(comms.data(), ndev, devices) != ncclSuccess) {
        ks_batch_destroy(b);
        return nullptr;
    }
    for (int i = 0; i < ndev; ++i) b->loc[i].comm = comms[i];
    return b;
}

ks_batch* ks_batch_create_rank(int device, int nranks, int rank, const uint8_t* id, const ks_opts* opts) {
    std::string err;
    const Rccl* api = id && nranks >= 1 && rank >= 0 && rank < nranks ? comm_lib(err) : nullptr;
    if (!api) return nullptr;
    ks_batch* b = make_batch(api, nranks, opts, {{device, rank}});
    if (!b) return nullptr;
    ncclUniqueId u;
    std::memcpy(u.internal, id, KS_UNIQUE_ID_BYTES);
    if (hipSetDevice(device) != hipSuccess || api->CommInitRank(&b->loc[0].comm, nranks, u, rank) != ncclSuccess) {
        ks_batch_destroy(b);
        return nullptr;
    }
    return b;
}

void ks_batch_destroy(ks_batch* b) {
    if (!b) return;
    for (auto& l : b->loc) {
        (void)hipSetDevice(l.device);
        if (l.comm) b->nccl->CommDestroy(l.comm);
        if (l.rows) (void)hipFree(l.rows);
        if (l.scratch) (void)hipFree(l.scratch);
        if (l.stat) (void)hipFree(l.stat);
        ks_destroy(l.ctx);
    }
    if (b->root_buf) {
        (void)hipSetDevice(b->loc[0].device);
        (void)hipFree(b->root_buf);
    }
    delete b;
}

const char* ks_batch_last_error(ks_batch* b) { return b ? b->err.c_str() : "null batch"; }

int ks_batch_load(ks_batch* b, size_t ngraphs, const ks_node* const* nodes, const size_t* n,
                  const ks_arc* const* arcs, const size_t* m) {
    if (!b) return KS_E_INVALID;
    if (ngraphs && (!nodes || !n || !arcs || !m)) return b->fail(KS_E_INVALID, "null graph arrays");
    b->ngraphs = ngraphs;
    for (auto& l : b->loc) {
        l.graphs.clear();
        for (size_t g = 0; g < ngraphs; ++g) {
            int r = 0;
            size_t slot = 0;
            ks_batch_owner(g, b->world, &r, &slot);
            if (r == l.grank) l.graphs.push_back((int)g);   // slot = its index in l.graphs
        }
        if (l.graphs.size() > 1024) return b->fail(KS_E_INVALID, "more than 1024 graphs on one device");
        // the disjoint union of this device's graphs: node ids offset per graph
        std::vector<ks_node> un;
        std::vector<ks_arc> ua;
        // every graph's id range in the union: its highest id plus the reserved ids
        std::vector<uint64_t> maxids;
        for (int g : l.graphs) {
            uint64_t mx = 0;
            for (size_t i = 0; i < n[g]; ++i) mx = std::max<uint64_t>(mx, nodes[g][i].id);
            maxids.push_back(mx);
        }
        l.off.assign(l.graphs.size() + 1, 0);
        if (int rc = ks_batch_node_offsets(maxids.data(), maxids.size(), b->spare, l.off.data()))
            return b->fail(rc, "the union's node ids exceed the supported range");
        l.toff.assign(1, 0);
        for (size_t gi = 0; gi < l.graphs.size(); ++gi) {
            const int g = l.graphs[gi];
            const uint64_t maxid = maxids[gi];
            const uint64_t base = (uint64_t)l.off[gi];
            int64_t tasks = 0;
            for (size_t i = 0; i < n[g]; ++i) {
                ks_node x = nodes[g][i];
                tasks += x.type == KS_NODE_TASK;
                x.id += base;
                un.push_back(x);
            }
            for (size_t i = 0; i < m[g]; ++i) {
                ks_arc a = arcs[g][i];
                // an arc must stay inside its own graph: past its max id it would land
                // on a node of the next graph in the union and couple two cells
                if (a.src == 0 || a.dst == 0 || a.src > maxid || a.dst > maxid)
                    return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + ": arc " + std::to_string(a.src) +
                                                     "->" + std::to_string(a.dst) + " outside its node id range");
                a.src += base;
                a.dst += base;
                ua.push_back(a);
            }
            l.toff.push_back(l.toff.back() + tasks);
        }
        const int rc = ks_load_graph(l.ctx, un.data(), un.size(), ua.data(), ua.size());
        if (rc) return b->fail(rc, ks_last_error(l.ctx));
        l.ctx->every_sink = true;   // one sink per graph: a commit's capacity refresh starts from all of them
        if (b->spare) {
            // the reserved ids are node slots from now on (dead until a stream adds them), and
            // the first build already has an edited graph's slack: round 1 lands in place
            ks_ctx* c = l.ctx;
            if (c->nodes.size() < (size_t)l.off.back() + 1) {
                c->nodes.resize((size_t)l.off.back() + 1);
                c->ids.resize((size_t)l.off.back() + 1);
            }
            if (int rc2 = c->eng.expect_deltas(l.off.back(), c->err)) {
                c->store_bad = true;
                return b->fail(rc2, c->err);
            }
        }
        // the union's cells: the cell solver runs each in its own workgroup (ks_cell.h)
        l.ctx->eng.set_cells(l.off.data(), l.graphs.size());
    }
    return KS_OK;
}

int ks_batch_solve(ks_batch* b, ks_result* results) {
    if (!b) return KS_E_INVALID;
    std::vector<int> rcs(b->loc.size(), KS_OK);
    std::vector<std::thread> th;
    for (size_t i = 0; i < b->loc.size(); ++i)
        th.emplace_back([&, i]() { rcs[i] = ks_solve(b->loc[i].ctx, &b->loc[i].res); });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < b->loc.size(); ++i) {
        if (results) results[i] = b->loc[i].res;
        if (rcs[i]) return b->fail(rcs[i], ks_last_error(b->loc[i].ctx));
    }
    return KS_OK;
}

int ks_batch_gather(ks_batch* b, size_t max_tasks, uint64_t* pu, int64_t* cost, int64_t* flow) {
    if (!b) return KS_E_INVALID;
    const size_t rowlen = kb_rowlen(max_tasks);
    const size_t block = kb_block(b->ngraphs, b->world, max_tasks);   // elements per rank
    bool has_root = false;
    int root_loc = -1;   // the local device of global rank 0 once its receive buffer is ready
    // 1. every device packs its block: [status][rows: cost, flow value, cell-local PU per task].
    //    A rank that fails here — a logical error or ANY HIP failure — still takes part
    //    in the collective below with its status word set, so its peers never wait for
    //    a send that is not posted (no early return before the status all-reduce).
    std::vector<int> status(b->loc.size(), KS_OK);
    std::string first_err;
    for (size_t li = 0; li < b->loc.size(); ++li) {
        auto& l = b->loc[li];
        ks_ctx* c = l.ctx;
        if (l.grank == 0) has_root = true;
        const size_t k = l.graphs.size();
        hipStream_t st = c->eng.stream();
        int rc = KS_OK;
        // a HIP failure: this rank's status, then on to the collective
#define KB_TRY(expr)                                                                          \
    do {                                                                                      \
        if (rc == KS_OK) {                                                                    \
            const hipError_t _e = (expr);                                                     \
            if (_e != hipSuccess) {                                                           \
                rc = KS_E_DEVICE;                                                             \
                c->err = std::string(#expr) + ": " + hipGetErrorString(_e);                   \
            }                                                                                 \
        }                                                                                     \
    } while (0)
        KB_TRY(hipSetDevice(l.device));
        if (b->fault_pack == (int)l.grank + 1) {   // TESTS ONLY: this rank's packing fails
            rc = KS_E_DEVICE;
            c->err = "injected pack failure";
        }
        if (rc == KS_OK && l.rows_cap < block) {
            if (l.rows) (void)hipFree(l.rows);
            l.rows = nullptr;
            l.rows_cap = 0;
            KB_TRY(hipMalloc(&l.rows, block * sizeof(long long)));
            if (rc == KS_OK) l.rows_cap = block;
        }
        KB_TRY(hipMemsetAsync(l.rows, 0, block * sizeof(long long), st));
        for (size_t i = 0; i < k && rc == KS_OK; ++i)
            if ((size_t)(l.toff[i + 1] - l.toff[i]) > max_tasks) {
                rc = KS_E_INVALID;
                c->err = "a graph has more tasks than max_tasks";
            }
        const size_t need = (size_t)l.toff.back() + 3 * (k + 1);
        if (rc == KS_OK && l.scratch_cap < need) {
            if (l.scratch) (void)hipFree(l.scratch);
            l.scratch = nullptr;
            l.scratch_cap = 0;
            KB_TRY(hipMalloc(&l.scratch, std::max<size_t>(need, 1) * sizeof(long long)));
            if (rc == KS_OK) l.scratch_cap = need;
        }
        if (rc == KS_OK && k) {
            long long* dcost = l.scratch + l.toff.back();
            long long* dflow = dcost + (k + 1);
            long long* doff = dflow + (k + 1);
            rc = c->eng.cell_sums(l.off.data(), k, (int64_t*)dcost, (int64_t*)dflow, c->err);
            size_t cnt = 0;
            if (rc == KS_OK) rc = ks_get_task_pu_device(c, (uint64_t*)l.scratch, (size_t)l.toff.back(), &cnt);
            long long* rows = l.rows + kb_row_in_block(0, max_tasks);
            KB_TRY(hipMemcpy2DAsync(rows, rowlen * sizeof(long long), dcost, sizeof(long long), sizeof(long long), k,
                                    hipMemcpyDeviceToDevice, st));
            KB_TRY(hipMemcpy2DAsync(rows + 1, rowlen * sizeof(long long), dflow, sizeof(long long), sizeof(long long),
                                    k, hipMemcpyDeviceToDevice, st));
            for (size_t i = 0; i < k; ++i) {
                const size_t t = (size_t)(l.toff[i + 1] - l.toff[i]);
                if (t)
                    KB_TRY(hipMemcpyAsync(l.rows + kb_row_in_block(i, max_tasks) + 2, l.scratch + l.toff[i],
                                          t * sizeof(long long), hipMemcpyDeviceToDevice, st));
            }
            KB_TRY(hipMemcpyAsync(doff, l.off.data(), k * sizeof(long long), hipMemcpyHostToDevice, st));
            if (rc == KS_OK)
                hipLaunchKernelGGL(k_localize, dim3(std::max<size_t>(1, std::min<size_t>(64, (rowlen + 255) / 256)), k),
                                   dim3(256), 0, st, (int)k, (int)rowlen, (const long long*)doff, l.rows);
            KB_TRY(hipGetLastError());
        }
        // rank 0 also holds the receive buffer of step 3: allocated (and its own block
        // copied in) here, so a failure is this rank's status word like any other and
        // nothing between the status all-reduce and the send/receive group can fail
        if (rc == KS_OK && l.grank == 0) {
            const size_t need = block * (size_t)b->world;
            if (b->fault_root) {   // TESTS ONLY: the root buffer's allocation fails
                rc = KS_E_DEVICE;
                c->err = "injected root buffer allocation failure";
            } else if (b->root_cap < need) {
                if (b->root_buf) (void)hipFree(b->root_buf);
                b->root_buf = nullptr;
                b->root_cap = 0;
                KB_TRY(hipMalloc(&b->root_buf, need * sizeof(long long)));
                if (rc == KS_OK) b->root_cap = need;
            }
            if (rc == KS_OK) root_loc = (int)li;
            KB_TRY(hipMemcpyAsync(b->root_buf, l.rows, block * sizeof(long long), hipMemcpyDeviceToDevice, st));
        }
        // always drain the stream, also after a failure: the memset, the copies and
        // k_localize must be finished before the status word is written or we return
        {
            const hipError_t se = hipStreamSynchronize(st);
            if (se != hipSuccess && rc == KS_OK) {
                rc = KS_E_DEVICE;
                c->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(se);
            }
        }
        if (rc != KS_OK) {
            status[li] = rc;
            if (first_err.empty()) first_err = "rank " + std::to_string(l.grank) + ": " + c->err;
            // the status word goes out in the block when the rows buffer exists
            // (written on the engine's stream, which the rows' producers used)
            if (l.rows) {
                const long long sw = rc;
                if (hipMemcpyAsync(l.rows, &sw, sizeof(long long), hipMemcpyHostToDevice, st) == hipSuccess)
                    (void)hipStreamSynchronize(st);
            }
        }
#undef KB_TRY
    }
    // 2. every rank learns whether any rank failed (min over the status words), so
    //    all of them return the same error instead of only the failing one
    if (b->world > 1) {
        for (size_t li = 0; li < b->loc.size(); ++li) {
            auto& l = b->loc[li];
            const long long sw = status[li];
            // (a failure to post the word is itself this rank's failure; it still enters)
            if ((hipSetDevice(l.device) != hipSuccess ||
                 hipMemcpy(l.stat, &sw, sizeof(long long), hipMemcpyHostToDevice) != hipSuccess) &&
                status[li] == KS_OK) {
                status[li] = KS_E_DEVICE;
                if (first_err.empty()) first_err = "rank " + std::to_string(l.grank) + ": status word not posted";
            }
        }
        {   // (the group is always closed: an RCCL error is returned after GroupEnd)
            ncclResult_t nr = b->nccl->GroupStart();
            for (auto& l : b->loc) {
                const ncclResult_t x = b->nccl->AllReduce(l.stat, l.stat, 1, ncclInt64, ncclMin, l.comm, l.ctx->eng.stream());
                if (nr == ncclSuccess) nr = x;
            }
            const ncclResult_t ge = b->nccl->GroupEnd();
            if (nr == ncclSuccess) nr = ge;
            if (nr != ncclSuccess) return b->fail(KS_E_DEVICE, std::string("status all-reduce: ") + b->nccl->GetErrorString(nr));
        }
        long long worst = 0;
        for (size_t li = 0; li < b->loc.size(); ++li) {
            auto& l = b->loc[li];
            long long sw = 0;
            if (hipSetDevice(l.device) != hipSuccess || hipStreamSynchronize(l.ctx->eng.stream()) != hipSuccess ||
                hipMemcpy(&sw, l.stat, sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess)
                sw = KS_E_DEVICE;
            worst = std::min<long long>(worst, std::min<long long>(sw, status[li]));
        }
        if (worst != 0)
            return b->fail((int)worst, first_err.empty() ? "another rank failed to pack its rows (status " +
                                                               std::to_string(worst) + ")"
                                                         : first_err);
    }
    // world 1: this process's own failure ends it here (no peer waits)
    for (int rc : status)
        if (rc != KS_OK) return b->fail(rc, first_err);
    // 3. one group: every rank's block to global rank 0. Nothing between the status
    //    all-reduce and GroupEnd returns early: an RCCL error is remembered and
    //    returned after the group, so no peer is left waiting in a send.
    long long* rbuf = root_loc >= 0 ? b->root_buf : nullptr;
    if (b->world > 1) {
        ncclResult_t nr = b->nccl->GroupStart();
        for (auto& l : b->loc) {
            hipStream_t st = l.ctx->eng.stream();
            if (l.grank == 0) {
                for (int r = 1; r < b->world; ++r) {
                    const ncclResult_t x = b->nccl->Recv(rbuf + (size_t)r * block, block, ncclInt64, r, l.comm, st);
                    if (nr == ncclSuccess) nr = x;
                }
            } else {
                const ncclResult_t x = b->nccl->Send(l.rows, block, ncclInt64, 0, l.comm, st);
                if (nr == ncclSuccess) nr = x;
            }
        }
        const ncclResult_t ge = b->nccl->GroupEnd();
        if (nr == ncclSuccess) nr = ge;
        if (nr != ncclSuccess) return b->fail(KS_E_DEVICE, std::string("ncclSend/ncclRecv group: ") + b->nccl->GetErrorString(nr));
    }
    for (auto& l : b->loc) {
        KB_HIP(hipSetDevice(l.device));
        KB_HIP(hipStreamSynchronize(l.ctx->eng.stream()));
    }
    for (int rc : status)
        if (rc != KS_OK) return b->fail(rc, first_err);   // this process's own failure, after the collective
    if (!has_root) return KS_OK;
    // 4. rank 0: every rank's status word, then the rows back in graph order
    std::vector<long long> host(block * (size_t)b->world);
    for (auto& l : b->loc)
        if (l.grank == 0) {
            KB_HIP(hipSetDevice(l.device));
            KB_HIP(hipMemcpy(host.data(), rbuf, host.size() * sizeof(long long), hipMemcpyDeviceToHost));
        }
    const int rc = ks_batch_unpack((const int64_t*)host.data(), b->ngraphs, b->world, max_tasks, pu, cost, flow);
    if (rc != KS_OK) return b->fail(rc, "a rank failed to pack its rows (status " + std::to_string(rc) + ")");
    return KS_OK;
}

// ---- batch rounds: deltas, the graph as it stands, bindings, commits ----

int ks_batch_reserve(ks_batch* b, size_t spare_ids) {
    if (!b) return KS_E_INVALID;
    if (spare_ids >= (size_t(1) << 30)) return b->fail(KS_E_RANGE, "reserved ids beyond the node id range");
    b->spare = spare_ids;
    return KS_OK;
}

int ks_batch_apply_deltas(ks_batch* b, size_t ngraphs, const ks_delta* const* deltas, const size_t* k) {
    if (!b) return KS_E_INVALID;
    if (ngraphs != b->ngraphs) return b->fail(KS_E_INVALID, "the stream count differs from the loaded graphs");
    if (ngraphs && (!deltas || !k)) return b->fail(KS_E_INVALID, "null stream arrays");
    // 1. every local device's union stream: its graphs' streams translated into their id
    //    ranges and concatenated in graph order (a record that leaves its graph's range
    //    stops the call here, before any device changed)
    std::vector<std::vector<ks_delta>> us(b->loc.size());
    for (size_t li = 0; li < b->loc.size(); ++li) {
        auto& l = b->loc[li];
        std::vector<ks_delta>& u = us[li];
        for (size_t i = 0; i < l.graphs.size(); ++i) {
            const size_t g = (size_t)l.graphs[i];
            if (!deltas[g] || !k[g]) continue;
            if (k[g] > (size_t)INT32_MAX - u.size()) return b->fail(KS_E_RANGE, "delta stream too long");
            const size_t at = u.size();
            u.resize(at + k[g]);
            const int rc = ks_batch_translate_deltas(l.off[i], l.off[i + 1], deltas[g], k[g], u.data() + at);
            if (rc == KS_E_RANGE) {
                const uint64_t span = (uint64_t)(l.off[i + 1] - l.off[i]);
                const size_t j = kb_first_bad(deltas[g], k[g], span);
                bool any = false;
                const uint64_t id = j < k[g] ? kb_bad_id(deltas[g][j], span, &any) : 0;
                return b->fail(rc, "graph " + std::to_string(g) + ": record " + std::to_string(j) + " names node id " +
                                       std::to_string(id) + ", outside the graph's ids 1.." + std::to_string(span) +
                                       " (its highest id at the load plus the reserved ids)");
            }
            if (rc) return b->fail(rc, "graph " + std::to_string(g) + ": bad delta stream");
            if (l.ctx->opts.auto_sink) append_auto_sink(l, i, u, at);
        }
    }
    // 2. one ks_apply_deltas per device (all or nothing there; no collective: a rank
    //    returns its own failure)
    for (size_t li = 0; li < b->loc.size(); ++li) {
        auto& l = b->loc[li];
        if (us[li].empty()) continue;
        const int rc = ks_apply_deltas(l.ctx, us[li].data(), us[li].size());
        if (rc) return b->fail(rc, "rank " + std::to_string(l.grank) + ": " + ks_last_error(l.ctx));
        recompute_toff(l);
    }
    return KS_OK;
}

int ks_batch_get_graph(ks_batch* b, size_t g, ks_node* nodes, size_t ncap, size_t* n, ks_arc* arcs, size_t acap,
                       size_t* m) {
    if (!b || !n || !m) return KS_E_INVALID;
    size_t i = 0;
    ks_batch::Local* l = owner_of(b, g, &i);
    if (!l) return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + " is not on this rank");
    ks_ctx* c = l->ctx;
    const uint64_t lo = (uint64_t)l->off[i], hi = (uint64_t)l->off[i + 1];
    size_t cnt = 0;
    for (uint64_t id = lo + 1; id <= hi && id < c->nodes.size(); ++id) {
        const NodeRec& r = c->nodes[id];
        if (!r.alive) continue;
        if (nodes && cnt < ncap) nodes[cnt] = ks_node{id - lo, r.excess, r.type, 0};
        ++cnt;
    }
    *n = cnt;
    // the union's live arcs (arc-slot order), this graph's kept
    if (c->store_bad) return b->fail(KS_E_INVALID, "the device graph store is inconsistent: reload the batch");
    std::vector<ks_arc> v;
    const int rc = c->eng.arcs(v, c->err);
    if (rc) return b->fail(rc, c->err);
    const size_t all = v.size();
    cnt = 0;
    for (size_t j = 0; j < all; ++j) {
        ks_arc a = v[j];
        if (a.src <= lo || a.src > hi) continue;
        a.src -= lo;
        a.dst -= lo;
        if (arcs && cnt < acap) arcs[cnt] = a;
        ++cnt;
    }
    *m = cnt;
    return KS_OK;
}

int ks_batch_set_bindings(ks_batch* b, size_t g, const uint64_t* task, const uint64_t* pu, size_t k) {
    if (!b) return KS_E_INVALID;
    if (k && (!task || !pu)) return b->fail(KS_E_INVALID, "null binding array");
    size_t i = 0;
    ks_batch::Local* l = owner_of(b, g, &i);
    if (!l) return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + " is not on this rank");
    const uint64_t lo = (uint64_t)l->off[i], span = (uint64_t)(l->off[i + 1] - l->off[i]);
    std::vector<uint64_t> t(k), p(k);
    for (size_t j = 0; j < k; ++j) {
        if (task[j] == 0 || task[j] > span || pu[j] > span)
            return b->fail(KS_E_RANGE, "graph " + std::to_string(g) + ": binding outside the graph's ids");
        t[j] = task[j] + lo;
        p[j] = pu[j] ? pu[j] + lo : 0;
    }
    const int rc = ks_set_bindings(l->ctx, t.data(), p.data(), k);
    if (rc) return b->fail(rc, ks_last_error(l->ctx));
    return KS_OK;
}

int ks_batch_commit_schedule(ks_batch* b, int32_t flags, int64_t continuation_cost, ks_batch_delta* out, size_t cap,
                             size_t* count, ks_commit_stats* stats) {
    return batch_commit(b, out, cap, count, stats,
                        [&](ks_ctx* c, ks_sched_delta* o, size_t ocap, size_t* n, ks_commit_stats* st) {
                            return ks_commit_schedule(c, flags, continuation_cost, nullptr, 0, o, ocap, n, st);
                        });
}

int ks_batch_commit_preemptive(ks_batch* b, int32_t flags, int64_t continuation_cost, int64_t preemption_cost,
                               ks_batch_delta* out, size_t cap, size_t* count, ks_preempt_stats* stats) {
    return batch_commit(b, out, cap, count, stats,
                        [&](ks_ctx* c, ks_sched_delta* o, size_t ocap, size_t* n, ks_preempt_stats* st) {
                            return ks_commit_preemptive(c, flags, continuation_cost, preemption_cost, nullptr, 0, o,
                                                        ocap, n, st);
                        });
}

// ---- batch rounds, the task side: arrivals, completions, refreshes, bindings, costs ----

int ks_batch_add_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                       int64_t unsched_sink_cost, ks_add_stats* stats) {
    return batch_task_call(b, ngraphs, lists, true, true, nullptr, stats,
                           [&](ks_ctx* c, const UnionLists& u, uint64_t*, ks_add_stats* st) {
                               return ks_add_tasks(c, flags, u.tasks.data(), u.tasks.size(), u.arc_off.data(),
                                                   u.arcs.data(), u.agg_ptr(), u.agg.size(), unsched_sink_cost, st);
                           });
}

int ks_batch_complete_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                            uint64_t* const* left, ks_complete_stats* stats) {
    // every k == 0 with the caps flag is the lone call's plain capacity refresh (what a round runs
    // after ks_batch_add_resources): it reaches every local device's union under the NULL rule
    bool listed = false;
    for (size_t g = 0; b && lists && ngraphs == b->ngraphs && g < ngraphs; ++g) listed |= lists[g].k != 0;
    return batch_task_call(b, ngraphs, lists, false, true, left, stats,
                           [&](ks_ctx* c, const UnionLists& u, uint64_t* hl, ks_complete_stats* st) {
                               return ks_complete_tasks(c, flags, u.tasks.data(), u.tasks.size(), u.agg_ptr(),
                                                        u.agg.size(), hl, st);
                           }, (flags & KS_COMPLETE_RESOURCE_CAPS) && !listed);
}

int ks_batch_update_tasks(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_task_list* lists,
                          int64_t unsched_sink_cost, ks_update_stats* stats) {
    return batch_task_call(b, ngraphs, lists, true, false, nullptr, stats,
                           [&](ks_ctx* c, const UnionLists& u, uint64_t*, ks_update_stats* st) {
                               return ks_update_tasks(c, flags, u.tasks.data(), u.tasks.size(), u.arc_off.data(),
                                                      u.arcs.data(), u.agg_ptr(), u.agg.size(), unsched_sink_cost, st);
                           });
}

int ks_batch_get_bindings(ks_batch* b, size_t g, const uint64_t* task, uint64_t* pu, size_t k) {
    if (!b) return KS_E_INVALID;
    if (k && (!task || !pu)) return b->fail(KS_E_INVALID, "null binding array");
    size_t i = 0;
    ks_batch::Local* l = owner_of(b, g, &i);
    if (!l) return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + " is not on this rank");
    const uint64_t lo = (uint64_t)l->off[i], span = (uint64_t)(l->off[i + 1] - l->off[i]);
    const std::vector<NodeRec>& nodes = l->ctx->nodes;
    std::vector<uint64_t> t(k);
    for (size_t j = 0; j < k; ++j) {
        if (task[j] == 0 || task[j] > span)
            return b->fail(KS_E_RANGE, "graph " + std::to_string(g) + ": binding outside the graph's ids");
        t[j] = task[j] + lo;
        if (t[j] >= nodes.size() || !nodes[t[j]].alive || nodes[t[j]].type != KS_NODE_TASK)
            return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + ": binding of a node that is not a live task: " +
                                             std::to_string(task[j]));
    }
    const int rc = ks_get_bindings(l->ctx, t.data(), pu, k);
    if (rc) return b->fail(rc, ks_last_error(l->ctx));
    for (size_t j = 0; j < k; ++j)
        if (pu[j]) pu[j] -= lo;
    return KS_OK;
}

int ks_batch_update_unsched_costs(ks_batch* b, size_t ngraphs, const ks_batch_task_list* lists, int32_t mode,
                                  int64_t cost, int64_t continuation_cost, size_t* changed) {
    if (!b) return KS_E_INVALID;
    if (changed) *changed = 0;
    if (lists && ngraphs != b->ngraphs) return b->fail(KS_E_INVALID, "the list count differs from the loaded graphs");
    // every local device's aggregators first (a bad id stops the call before any device changed)
    std::vector<std::vector<uint64_t>> ids(b->loc.size());
    for (size_t li = 0; lists && li < b->loc.size(); ++li) {
        const auto& l = b->loc[li];
        for (size_t i = 0; i < l.graphs.size(); ++i) {
            const size_t g = (size_t)l.graphs[i];
            const ks_batch_task_list& L = lists[g];
            if (!L.nu) continue;
            if (!L.unsched_ids) return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + ": null aggregator array");
            const uint64_t lo = (uint64_t)l.off[i], span = (uint64_t)(l.off[i + 1] - l.off[i]);
            for (size_t j = 0; j < L.nu; ++j) {
                const uint64_t id = L.unsched_ids[j];
                if (id == 0 || id > span)
                    return b->fail(KS_E_RANGE, "graph " + std::to_string(g) + ": unscheduled aggregator " + std::to_string(id) +
                                                   " is outside the graph's ids 1.." + std::to_string(span));
                if (id + lo >= l.ctx->nodes.size() || !l.ctx->nodes[id + lo].alive)
                    return b->fail(KS_E_INVALID, "graph " + std::to_string(g) + ": unscheduled aggregator " +
                                                     std::to_string(id) + " is not a live node");
                ids[li].push_back(id + lo);
            }
        }
    }
    size_t total = 0;
    for (size_t li = 0; li < b->loc.size(); ++li) {
        auto& l = b->loc[li];
        if (lists && ids[li].empty()) continue;
        size_t ch = 0;
        const int rc = ks_update_unsched_costs(l.ctx, lists ? ids[li].data() : nullptr, ids[li].size(), mode, cost,
                                               continuation_cost, &ch);
        if (rc) return b->fail(rc, "rank " + std::to_string(l.grank) + ": " + ks_last_error(l.ctx));
        total += ch;
    }
    if (changed) *changed = total;
    return KS_OK;
}

// ---- batch rounds, the resource side: machines and racks leave and join ----

int ks_batch_remove_resources(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_res_list* lists,
                              uint64_t* removed, size_t rcap, size_t* nremoved, size_t* removed_off,
                              ks_batch_delta* evicted, size_t ecap, size_t* nevicted, ks_remove_stats* stats) {
    if (!b || !nremoved || !nevicted) return KS_E_INVALID;
    *nremoved = *nevicted = 0;
    if (flags & ~(KS_REMOVE_RESOURCE_CAPS | KS_REMOVE_PREEMPTIVE)) return b->fail(KS_E_INVALID, "unknown remove flag");
    if ((flags & KS_REMOVE_PREEMPTIVE) && !(flags & KS_REMOVE_RESOURCE_CAPS))
        return b->fail(KS_E_INVALID, "KS_REMOVE_PREEMPTIVE selects a capacity rule: it needs KS_REMOVE_RESOURCE_CAPS");
    if (int rc = check_res_lists(b, ngraphs, lists, false)) return rc;
    const bool probe = !removed && !evicted;
    if (!probe && ((!removed && rcap) || (!evicted && ecap)))
        return b->fail(KS_E_INVALID, "a null output buffer with room in it");
    if (!removed) rcap = 0;
    if (!evicted) ecap = 0;
    // every local device's roots first (a root outside its graph stops the call before any device is asked)
    const size_t nl = b->loc.size();
    std::vector<UnionRes> us(nl);
    for (size_t li = 0; li < nl; ++li)
        if (int rc = build_union_res(b, b->loc[li], lists, false, us[li])) return rc;
    auto touched = [](const ks_batch::Local&, const UnionRes& u) { return u.touched; };
    auto totals = [&]() {
        *nremoved = *nevicted = 0;
        for (const UnionRes& u : us) *nremoved += u.nr, *nevicted += u.ne;
    };
    // a probe, and with several local devices the count of every device before any of them
    // changes: a buffer that is too small or a root any device refuses changes none
    if (probe || nl > 1) {
        const int rc = each_device(b, us, (ks_remove_stats*)nullptr, touched,
                                   [&](ks_batch::Local& l, UnionRes& u, ks_remove_stats*) {
                                       return ks_remove_resources(l.ctx, flags, u.roots.data(), u.roots.size(), nullptr, 0,
                                                                  &u.nr, nullptr, 0, &u.ne, nullptr);
                                   }, nothing_after);
        if (rc) return rc;
        totals();
        if (probe) return KS_OK;
        if (rcap < *nremoved || ecap < *nevicted)
            return b->fail(KS_E_INVALID, rcap < *nremoved ? "removed buffer smaller than the removed nodes"
                                                          : "evicted buffer smaller than the evicted tasks");
    }
    ks_remove_stats sum;
    std::vector<std::vector<uint64_t>> per_graph(ngraphs);
    std::vector<ks_batch_delta> all;
    // what the device being called removed and evicted, in the union's numbering: filled by a device's
    // call, read by its after-step, then reused for the next device (valid only between the two)
    std::vector<uint64_t> rm;
    std::vector<ks_sched_delta> ev;
    const int rc = each_device(
        b, us, &sum, touched,
        [&](ks_batch::Local& l, UnionRes& u, ks_remove_stats* st) {
            // (one local device: its own call counts and checks the room; no removal exceeds the node table)
            const size_t cap_r = nl > 1 ? u.nr : std::min(rcap, l.ctx->nodes.size());
            const size_t cap_e = nl > 1 ? u.ne : std::min(ecap, l.ctx->nodes.size());
            rm.assign(cap_r + 1, 0);
            ev.assign(cap_e + 1, ks_sched_delta{});
            const int rc = ks_remove_resources(l.ctx, flags, u.roots.data(), u.roots.size(), rm.data(), cap_r, &u.nr,
                                               ev.data(), cap_e, &u.ne, st);
            if (nl == 1) totals();
            return rc;
        },
        [&](ks_batch::Local& l, UnionRes& u) {
            for (size_t j = 0; j < u.nr; ++j) {   // ascending in the union: ascending within each graph
                const size_t i = graph_index(l, rm[j]);
                per_graph[(size_t)l.graphs[i]].push_back(rm[j] - (uint64_t)l.off[i]);
            }
            ev.resize(u.ne);
            localize_deltas(l, ev, all);
            return (int)KS_OK;
        });
    if (rc) return rc;
    size_t at = 0;
    for (size_t g = 0; g < ngraphs; ++g) {
        if (removed_off) removed_off[g] = at;
        for (uint64_t id : per_graph[g]) removed[at++] = id;
    }
    if (removed_off) removed_off[ngraphs] = at;
    // grouped by graph, ascending; within a graph in task order (a device's evictions come in slot order)
    std::stable_sort(all.begin(), all.end(),
                     [](const ks_batch_delta& x, const ks_batch_delta& y) { return x.graph < y.graph; });
    if (!all.empty()) std::memcpy(evicted, all.data(), all.size() * sizeof(ks_batch_delta));
    if (stats) *stats = sum;
    return KS_OK;
}

int ks_batch_add_resources(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_res_list* lists,
                           ks_grow_stats* stats) {
    if (!b) return KS_E_INVALID;
    if (flags) return b->fail(KS_E_INVALID, "unknown flag (flags is reserved: pass 0)");
    if (int rc = check_res_lists(b, ngraphs, lists, true)) return rc;
    // every local device's records first (a node id outside its graph stops the call before any device changed)
    std::vector<UnionRes> us(b->loc.size());
    for (size_t li = 0; li < b->loc.size(); ++li)
        if (int rc = build_union_res(b, b->loc[li], lists, true, us[li])) return rc;
    return each_device(b, us, stats, [](const ks_batch::Local&, const UnionRes& u) { return u.touched; },
                       [&](ks_batch::Local& l, const UnionRes& u, ks_grow_stats* st) {
                           return ks_add_resources(l.ctx, 0, u.nodes.data(), u.nodes.size(), u.arcs.data(), u.arcs.size(), st);
                       }, nothing_after);
}

// ---- batch rounds, class and resource arcs: the rest of the cost model's sweep ----

int ks_batch_update_nodes(ks_batch* b, int32_t flags, size_t ngraphs, const ks_batch_node_list* lists,
                          ks_node_stats* stats) {
    if (!b) return KS_E_INVALID;
    if (flags & ~KS_NODES_KEEP_UNLISTED) return b->fail(KS_E_INVALID, "unknown update flag");
    if (int rc = check_node_lists(b, ngraphs, lists)) return rc;
    // every local device's tails first (a tail outside its graph stops the call before any device is asked)
    std::vector<UnionNodes> us(b->loc.size());
    for (size_t li = 0; li < b->loc.size(); ++li)
        if (int rc = build_union_nodes(b, b->loc[li], lists, us[li])) return rc;
    return each_device(b, us, stats, [](const ks_batch::Local&, const UnionNodes& u) { return !u.nodes.empty(); },
                       [&](ks_batch::Local& l, const UnionNodes& u, ks_node_stats* st) {
                           return ks_update_nodes(l.ctx, flags, u.nodes.data(), u.nodes.size(), u.arc_off.data(),
                                                  u.arcs.data(), st);
                       }, nothing_after);
}

}  // extern "C"
