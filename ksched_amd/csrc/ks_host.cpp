// ks_host.cpp — host runtime and C-ABI of libksmcmf (include/ksmcmf.h).
//
// Mirrors the reference's solver boundary, scheduling/flow/placement/solver.go:
//   ks_create         ↔ NewSolver (:49-55) + startSolver (:92-109)
//   ks_load_graph     ↔ writeGraph → dimacs.Export (:111-116, dimacs/export.go:11-29)
//   ks_apply_deltas   ↔ writeIncremental → dimacs.ExportIncremental (:118-123)
//   ks_solve          ↔ the Flowlessly solve
//   ks_get_flows      ↔ the "f" lines consumed by readFlowGraph (:134-179)
//   ks_get_task_mapping ↔ parseFlowToMapping (:183-269)
// The graph itself lives on the device (ks_store.h): arc table, (src, dst) hash
// index and residual CSR, edited in place by ks_apply_deltas. The host keeps only
// node-level state — liveness, supply, type per NodeID (flowgraph/graph.go:27-182
// semantics: ids index slots, REMOVE_NODE drops incident arcs, ids are reused) —
// which is all a stream needs to be validated in order, sequentially, before the
// device resolves it in parallel.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ksmcmf.h"
#include "ks_ctx.h"

namespace {




constexpr uint64_t kMaxId = (1ULL << 30);

inline uint64_t arc_key(uint64_t s, uint64_t d) { return (s << 32) | d; }

// (src, dst) → record index for ks_coalesce_deltas: open addressing with linear
// probing and backward-shift deletion (no tombstones), power-of-two capacity
// kept under 1/2 load. Keys are never 0 (node ids start at 1), so 0 marks an
// empty bucket.
class ArcIndex {
public:
    void clear() {
        keys_.assign(16, 0);
        vals_.assign(16, -1);
        size_ = 0;
    }
    void reserve(size_t n) {
        size_t cap = 16;
        while (cap < 2 * n + 2) cap <<= 1;
        if (cap > keys_.size()) rehash(cap);
    }
    int find(uint64_t k) const {
        size_t i = slot(k);
        while (keys_[i]) {
            if (keys_[i] == k) return vals_[i];
            i = (i + 1) & mask();
        }
        return -1;
    }
    void insert(uint64_t k, int v) {   // k must be absent
        if (2 * (size_ + 1) > keys_.size()) rehash(keys_.size() * 2);
        size_t i = slot(k);
        while (keys_[i]) i = (i + 1) & mask();
        keys_[i] = k;
        vals_[i] = v;
        ++size_;
    }
    void erase(uint64_t k) {
        size_t i = slot(k);
        while (keys_[i] && keys_[i] != k) i = (i + 1) & mask();
        if (!keys_[i]) return;
        // backward shift: pull later members of the probe run into the hole
        size_t j = i;
        for (;;) {
            j = (j + 1) & mask();
            if (!keys_[j]) break;
            const size_t h = slot(keys_[j]);
            const bool between = (i <= j) ? (i < h && h <= j) : (i < h || h <= j);
            if (between) continue;
            keys_[i] = keys_[j];
            vals_[i] = vals_[j];
            i = j;
        }
        keys_[i] = 0;
        vals_[i] = -1;
        --size_;
    }

private:
    std::vector<uint64_t> keys_ = std::vector<uint64_t>(16, 0);
    std::vector<int> vals_ = std::vector<int>(16, -1);
    size_t size_ = 0;
    size_t mask() const { return keys_.size() - 1; }
    size_t slot(uint64_t k) const {
        k ^= k >> 33;
        k *= 0xff51afd7ed558ccdULL;
        k ^= k >> 33;
        return (size_t)k & mask();
    }
    void rehash(size_t cap) {
        std::vector<uint64_t> ok;
        std::vector<int> ov;
        ok.swap(keys_);
        ov.swap(vals_);
        keys_.assign(cap, 0);
        vals_.assign(cap, -1);
        size_ = 0;
        for (size_t i = 0; i < ok.size(); ++i)
            if (ok[i]) insert(ok[i], ov[i]);
    }
};

}  // namespace

namespace {

void ensure_node(ks_ctx* c, uint64_t id) {
    if (id >= c->nodes.size()) {
        c->nodes.resize(id + 1);
        c->ids.resize(id + 1);
    }
}

bool node_alive(const ks_ctx* c, uint64_t id) { return id < c->nodes.size() && c->nodes[id].alive; }

// Node-level aggregates (auto-sink demand, task count) follow every change.
void account(ks_ctx* c, uint64_t id, const NodeRec& r, int sign) {
    if (!r.alive) return;
    if (r.type == KS_NODE_SINK) {
        c->n_sinks += sign;
        if (sign > 0) c->sink_id = id;
    } else {
        c->sum_others += sign * r.excess;
    }
    if (r.type == KS_NODE_TASK) c->n_tasks += sign;
}

// Validate one arc against a node table (the context's, or a load's new one).
int check_arc(ks_ctx* c, const std::vector<NodeRec>& tab, uint64_t s, uint64_t d, uint64_t low, uint64_t cap,
              int64_t cost) {
    auto alive = [&](uint64_t id) { return id < tab.size() && tab[id].alive; };
    if (s == 0 || d == 0 || s >= kMaxId || d >= kMaxId) return c->fail(KS_E_RANGE, "arc endpoint id out of range");
    if (!alive(s) || !alive(d))
        return c->fail(KS_E_INVALID, "arc " + std::to_string(s) + "->" + std::to_string(d) + " has a missing endpoint");
    if (s == d) return c->fail(KS_E_INVALID, "self-loop arc at node " + std::to_string(s));
    if (low > (uint64_t)INT64_MAX || cap > (uint64_t)INT64_MAX) return c->fail(KS_E_RANGE, "arc bound exceeds int64");
    if (low > cap)
        return c->fail(KS_E_INVALID, "arc " + std::to_string(s) + "->" + std::to_string(d) + " has low > cap");
    if (cap > (uint64_t(1) << 53) || cost > (int64_t(1) << 40) || cost < -(int64_t(1) << 40))
        return c->fail(KS_E_RANGE, "arc capacity or cost outside the supported range");
    return KS_OK;
}
int check_arc(ks_ctx* c, uint64_t s, uint64_t d, uint64_t low, uint64_t cap, int64_t cost) {
    return check_arc(c, c->nodes, s, d, low, cap, cost);
}

// A device-side failure inside an apply or a load leaves the device store in an
// unknown state: every call that would read it refuses until the next load.
int store_guard(ks_ctx* c) {
    if (!c->store_bad) return KS_OK;
    return c->fail(KS_E_INVALID, "the device graph store is inconsistent after a failed load or apply: "
                                 "reload the graph (ks_load_graph)");
}

// The node table's side of one record stream (ks_apply_deltas, ks_remove_resources). Every
// node the stream touches is saved at its first touch, so the stream applies entirely or
// not at all; edits() turns the touched nodes into the store's node edits and moves the
// aggregates, rollback_applied() undoes both after a device failure.
struct NodeTxn {
    ks_ctx* c;
    std::vector<std::pair<uint64_t, NodeRec>> saved;   // first-touch state of every touched node
    int64_t sum0 = 0, sinks0 = 0, tasks0 = 0, dsink0 = 0;
    uint64_t sink0 = 0;

    explicit NodeTxn(ks_ctx* ctx) : c(ctx) {
        if (++c->epoch == 0) {   // epoch wrapped: forget old stamps
            for (auto& st : c->ids) st.epoch = 0;
            c->epoch = 1;
        }
    }
    void touch(uint64_t id) {
        ensure_node(c, id);
        if (c->ids[id].epoch != c->epoch) {
            c->ids[id].epoch = c->epoch;
            c->ids[id].lastrm = -1;
            saved.emplace_back(id, c->nodes[id]);
        }
    }
    // ADD_NODE (ks_apply_deltas, ks_add_tasks): the id in range and not a live node (graph.go:95-98)
    int add(uint64_t id, int64_t excess, int32_t type) {
        if (id == 0 || id >= kMaxId) return c->fail(KS_E_RANGE, ks::id_name(c->view, "node id", id) + " out of range");
        if (node_alive(c, id)) return c->fail(KS_E_INVALID, ks::id_name(c->view, "node", id) + " already present");
        touch(id);
        c->nodes[id] = NodeRec{excess, type, true, true};
        return KS_OK;
    }
    void remove(uint64_t id, int32_t pos) {   // REMOVE_NODE at stream position pos
        touch(id);
        c->nodes[id] = NodeRec{};
        c->ids[id].lastrm = pos;
    }
    void rollback_nodes() {
        for (auto it = saved.rbegin(); it != saved.rend(); ++it) c->nodes[it->first] = it->second;
    }
    void edits(std::vector<ks::NodeEdit>& out) {
        out.reserve(saved.size());
        sum0 = c->sum_others, sinks0 = c->n_sinks, tasks0 = c->n_tasks, dsink0 = c->dev_sink_supply;
        sink0 = c->sink_id;
        for (const auto& sv : saved) {
            const uint64_t id = sv.first;
            const NodeRec& now = c->nodes[id];
            account(c, id, sv.second, -1);
            account(c, id, now, 1);
            ks::NodeEdit e;
            std::memset(&e, 0, sizeof(e));
            e.slot = (int32_t)(id - 1);
            e.last_rm = c->ids[id].lastrm;
            e.supply = now.alive ? now.excess : 0;
            e.alive = now.alive ? 1 : 0;
            e.type = (uint8_t)std::min<int32_t>(std::max<int32_t>(now.type, 0), 255);
            e.was_alive = sv.second.alive ? 1 : 0;
            out.push_back(e);
            if (now.alive && now.type == KS_NODE_SINK) c->dev_sink_supply = now.excess;
        }
    }
    void rollback_applied() {
        rollback_nodes();
        c->sum_others = sum0;
        c->n_sinks = sinks0;
        c->n_tasks = tasks0;
        c->sink_id = sink0;
        c->dev_sink_supply = dsink0;
        c->store_bad = true;
    }
};

// ---- what the scheduler-side calls share: their argument checks and their epilogues

// The slot of the graph's one sink, −1 with none or several; every_sink: a partition's one
// sink per cell counts as Engine::kEverySink.
int64_t sink_slot(const ks_ctx* c, bool every_sink = false) {
    return c->n_sinks == 1                                    ? (int64_t)c->sink_id - 1
           : (every_sink && c->every_sink && c->n_sinks > 1) ? ks::Engine::kEverySink
                                                              : -1;
}

int check_aggregators(ks_ctx* c, const uint64_t* ids, size_t k) {
    for (size_t i = 0; ids && i < k; ++i)
        if (!node_alive(c, ids[i]))
            return c->fail(KS_E_INVALID, ks::id_name(c->view, "unscheduled aggregator", ids[i]) + " is not a live node");
    return KS_OK;
}

// The task lists of ks_add_tasks and ks_update_tasks (k > 0): offsets from 0 that never fall,
// and an arc array where they name an arc.
int check_task_lists(ks_ctx* c, const uint64_t* tasks, size_t k, const uint64_t* arc_off, const ks_task_arc* arcs) {
    if (arc_off[0] != 0) return c->fail(KS_E_INVALID, "arc_off[0] must be 0");
    for (size_t i = 0; i < k; ++i)
        if (arc_off[i + 1] < arc_off[i])
            return c->fail(KS_E_INVALID, "arc_off decreases at " + ks::id_name(c->view, "task", tasks[i]));
    if (arc_off[k] && !arcs) return c->fail(KS_E_INVALID, "null arc array");
    return KS_OK;
}

int check_sink_cost(ks_ctx* c, int64_t cost) {
    if (cost > (int64_t(1) << 40) || cost < -(int64_t(1) << 40))
        return c->fail(KS_E_RANGE, "unscheduled sink cost outside the supported range");
    return KS_OK;
}

// The graph changed (as after ks_apply_deltas): the solution no longer stands.
void drop_solution(ks_ctx* c) {
    c->have_solution = c->map_fresh = c->flows_fresh = false;
}

// A call that needed the residual CSR may have rebuilt it, and the solution in place went with it.
void follow_rebuild(ks_ctx* c) {
    if (!c->eng.solved()) drop_solution(c);
}

// A device delta call failed with rc. With a node transaction: its edits were made when dirty (the
// stream may be half applied: reload first), else only the node table moved. Without one a dirty
// store is marked bad. The stats of a call that may have written some read zero.
int delta_failed(ks_ctx* c, int rc, NodeTxn* txn, bool dirty) {
    if (txn && dirty) txn->rollback_applied();
    else if (txn) txn->rollback_nodes();
    else if (dirty) c->store_bad = true;
    return rc;
}
template <class Stats>
int delta_failed(ks_ctx* c, int rc, NodeTxn* txn, bool dirty, Stats* stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return delta_failed(c, rc, txn, dirty);
}

}  // namespace

extern "C" {

int ks_abi_version(void) { return KSMCMF_ABI_VERSION; }

void ks_default_opts(ks_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->alpha = 0;   // the library's size-dependent default (ks_engine.hip)
    o->verify = 1;
    o->auto_sink = 1;
    o->price_refine = 1;
    o->gu_interval = 24;   // 24 vs 32 on config 3: ≈ 2 ms lower median; config 5 ≈ 3 % faster (profiles/r01f_gu_interval.txt)
    o->warm_start = 0;
}

ks_ctx* ks_create(int device, const ks_opts* opts) {
    ks_ctx* c = new (std::nothrow) ks_ctx;
    if (!c) return nullptr;
    if (opts) c->opts = *opts;
    else ks_default_opts(&c->opts);
    std::string err;
    if (c->eng.init(device, c->opts, err) != KS_OK) {
        delete c;
        return nullptr;
    }
    c->nodes.resize(1);
    c->ids.resize(1);
    return c;
}

void ks_destroy(ks_ctx* c) { delete c; }

const char* ks_last_error(ks_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ks_load_graph(ks_ctx* c, const ks_node* nodes, size_t n, const ks_arc* arcs, size_t m) {
    if (!c) return KS_E_INVALID;
    if ((n && !nodes) || (m && !arcs)) return c->fail(KS_E_INVALID, "null input array");
    uint64_t maxid = 0;
    for (size_t i = 0; i < n; ++i) {
        if (nodes[i].id == 0 || nodes[i].id >= kMaxId)
            return c->fail(KS_E_RANGE, "node id " + std::to_string(nodes[i].id) + " out of range");
        maxid = std::max<uint64_t>(maxid, nodes[i].id);
    }
    std::vector<NodeRec> fresh(maxid + 1);
    for (size_t i = 0; i < n; ++i) {
        NodeRec& r = fresh[nodes[i].id];
        if (r.alive)   // graph.go:95-98
            return c->fail(KS_E_INVALID, "node " + std::to_string(nodes[i].id) + " already present");
        r = NodeRec{nodes[i].excess, nodes[i].type, true, true};
    }
    // every arc is checked against the new table BEFORE anything changes: a bad
    // arc leaves the context (host and device) exactly as it was
    for (size_t i = 0; i < m; ++i) {
        const ks_arc& a = arcs[i];
        int rc = check_arc(c, fresh, a.src, a.dst, a.low, a.cap, a.cost);
        if (rc) return rc;
    }
    c->nodes.swap(fresh);
    c->ids.assign(maxid + 1, ks_ctx::IdStamp{});
    c->sum_others = c->n_sinks = c->n_tasks = 0;
    c->sink_id = 0;
    for (uint64_t id = 1; id <= maxid; ++id) account(c, id, c->nodes[id], 1);
    drop_solution(c);
    std::vector<int64_t> supply(maxid);
    std::vector<uint8_t> type(maxid), alive(maxid);
    for (uint64_t id = 1; id <= maxid; ++id) {
        const NodeRec& r = c->nodes[id];
        supply[id - 1] = r.alive ? r.excess : 0;
        type[id - 1] = (uint8_t)std::min<int32_t>(std::max<int32_t>(r.type, 0), 255);
        alive[id - 1] = r.alive ? 1 : 0;
    }
    c->dev_sink_supply = (c->n_sinks == 1) ? c->nodes[c->sink_id].excess : 0;
    c->eng.set_cells(nullptr, 0);   // a plain load is one graph (ks_batch_load sets its cells after)
    c->every_sink = false;
    const int rc = c->eng.load((int64_t)maxid, supply.data(), type.data(), alive.data(), arcs, m, c->err);
    c->store_bad = rc != KS_OK;   // the upload failed part-way: nothing may read the store
    return rc;
}

// Validate the stream in order against node liveness (graph.go / the change
// manager's preconditions), all or nothing: on an error the host state is rolled
// back and nothing reaches the device. The device then resolves the records.
int ks_apply_deltas(ks_ctx* c, const ks_delta* d, size_t k) {
    if (!c) return KS_E_INVALID;
    if (k && !d) return c->fail(KS_E_INVALID, "null delta array");
    if (k > (size_t)INT32_MAX) return c->fail(KS_E_RANGE, "delta stream too long");
    if (int g = store_guard(c)) return g;
    const auto t_in = std::chrono::steady_clock::now();
    NodeTxn txn(c);
    auto touch = [&](uint64_t id) { txn.touch(id); };
    int rc = KS_OK;
    for (size_t i = 0; i < k && rc == KS_OK; ++i) {
        const ks_delta& x = d[i];
        switch (x.kind) {
            case KS_ADD_NODE:
                rc = txn.add(x.id, x.excess, x.type);
                break;
            case KS_REMOVE_NODE:
                if (!node_alive(c, x.id)) {
                    rc = c->fail(KS_E_INVALID, "remove of missing node " + std::to_string(x.id));
                    break;
                }
                txn.remove(x.id, (int32_t)i);
                break;
            case KS_ADD_ARC:
                rc = check_arc(c, x.src, x.dst, x.low, x.cap, x.cost);
                break;
            case KS_UPDATE_ARC:
                if (x.low == 0 && x.cap == 0) {   // DeleteArc / ChangeArc(0,0): the arc goes
                    if (x.src == 0 || x.dst == 0 || x.src >= kMaxId || x.dst >= kMaxId)
                        rc = c->fail(KS_E_RANGE, "arc endpoint id out of range");
                    else if (!node_alive(c, x.src) || !node_alive(c, x.dst))
                        rc = c->fail(KS_E_INVALID, "update of arc with a missing endpoint");
                    break;
                }
                rc = check_arc(c, x.src, x.dst, x.low, x.cap, x.cost);
                break;
            case KS_SET_EXCESS:
                if (!node_alive(c, x.id)) {
                    rc = c->fail(KS_E_INVALID, "excess of missing node " + std::to_string(x.id));
                    break;
                }
                touch(x.id);
                c->nodes[x.id].excess = x.excess;
                break;
            default:
                rc = c->fail(KS_E_INVALID, "unknown delta kind " + std::to_string(x.kind));
        }
    }
    if (rc) {   // roll back: the stream is applied entirely or not at all
        txn.rollback_nodes();
        return rc;
    }
    std::vector<ks::NodeEdit> edits;
    txn.edits(edits);
    drop_solution(c);
    const auto t_dev = std::chrono::steady_clock::now();
    rc = c->eng.apply(edits.data(), edits.size(), d, k, c->nslots(), c->err);
    if (c->opts.log_cycles) {   // (ks_opts.log_cycles: the host's and the device's share of an apply)
        const auto t_out = std::chrono::steady_clock::now();
        std::fprintf(stderr, "apply: %zu records, %zu node edits, host %.3f ms, device %.3f ms\n", k, edits.size(),
                     std::chrono::duration<double, std::milli>(t_dev - t_in).count(),
                     std::chrono::duration<double, std::milli>(t_out - t_dev).count());
    }
    if (rc) {
        // the device may have applied part of the stream: the host goes back to its
        // state before the call (nodes and aggregates) and the store is marked
        // unusable until the next ks_load_graph
        txn.rollback_applied();
    }
    return rc;
}

// Coalescing follows the store's semantics above: ADD_ARC and UPDATE_ARC are both
// upserts of the full (low, cap, cost, type) and UPDATE_ARC 0/0 deletes, so the
// last record of an arc decides its state (mergeChangesToSameArc and
// removeDuplicateChanges); REMOVE_NODE drops every incident arc, so arc and
// excess records touching the node before its removal are dead
// (purgeChangesBeforeNodeRemoval). Survivors keep their relative order and a
// kept record sits at its own position, after the ADD_NODEs of its endpoints.
int ks_coalesce_deltas(const ks_delta* in, size_t k, ks_delta* out, size_t cap, size_t* count) {
    if (!count || (k && !in) || k > (size_t)INT32_MAX) return KS_E_INVALID;
    for (size_t i = 0; i < k; ++i) {             // ids as the store accepts them (hash keys ≠ 0)
        const ks_delta& x = in[i];
        const bool arc = x.kind == KS_ADD_ARC || x.kind == KS_UPDATE_ARC;
        const uint64_t a = arc ? x.src : x.id, b = arc ? x.dst : 1;
        if (a == 0 || b == 0 || a >= kMaxId || b >= kMaxId) return KS_E_INVALID;
    }
    std::vector<uint8_t> keep(k, 1);
    ArcIndex last_arc;                           // (src, dst) → index of its live record
    last_arc.reserve(k);
    // node id → slot: direct when ids are dense (the FIFO-reused ids of a cell), else hashed
    uint64_t max_id = 0;
    for (size_t i = 0; i < k; ++i) {
        const ks_delta& x = in[i];
        const bool arc = x.kind == KS_ADD_ARC || x.kind == KS_UPDATE_ARC;
        max_id = std::max(max_id, arc ? std::max(x.src, x.dst) : x.id);
    }
    const bool direct = max_id <= 4 * (uint64_t)k + 65536;
    ArcIndex slot_of;                            // sparse ids: id → slot (key (id, 0))
    std::vector<int> head(direct ? max_id + 1 : 0, -1);   // slot → newest record touching it
    std::vector<int> last_exc(direct ? max_id + 1 : 0, -1);  // slot → live SET_EXCESS record
    std::vector<int> link(2 * k, -1);            // record i: next older record at src (2i) / dst (2i+1)
    auto slot = [&](uint64_t id) -> int {
        if (direct) return (int)id;
        int s = slot_of.find(arc_key(id, 0));
        if (s < 0) {
            s = (int)head.size();
            slot_of.insert(arc_key(id, 0), s);
            head.push_back(-1);
            last_exc.push_back(-1);
        }
        return s;
    };
    // the list entry 2i+e belongs to node (e ? dst : src) of record i
    auto push = [&](int s, int i, int e) {
        link[2 * i + e] = head[s];
        head[s] = 2 * i + e;
    };
    for (size_t i = 0; i < k; ++i) {
        const ks_delta& x = in[i];
        switch (x.kind) {
            case KS_ADD_ARC:
            case KS_UPDATE_ARC: {
                const uint64_t key = arc_key(x.src, x.dst);
                const int j = last_arc.find(key);
                if (j >= 0) {
                    keep[j] = 0;
                    last_arc.erase(key);
                }
                last_arc.insert(key, (int)i);
                push(slot(x.src), (int)i, 0);
                if (x.dst != x.src) push(slot(x.dst), (int)i, 1);
                break;
            }
            case KS_SET_EXCESS: {
                const int s = slot(x.id);
                if (last_exc[s] >= 0) keep[last_exc[s]] = 0;
                last_exc[s] = (int)i;
                break;
            }
            case KS_REMOVE_NODE: {
                const int s = slot(x.id);
                for (int e = head[s]; e >= 0; e = link[e]) {
                    const int j = e >> 1;
                    if (!keep[j]) continue;
                    keep[j] = 0;
                    last_arc.erase(arc_key(in[j].src, in[j].dst));
                }
                head[s] = -1;
                if (last_exc[s] >= 0) keep[last_exc[s]] = 0;
                last_exc[s] = -1;
                break;
            }
            default:
                break;                           // ADD_NODE and unknown kinds pass through
        }
    }
    size_t n = 0;
    for (size_t i = 0; i < k; ++i) {
        if (!keep[i]) continue;
        if (out && n < cap) out[n] = in[i];      // n ≤ i: in-place (out == in) is safe
        ++n;
    }
    *count = n;
    return KS_OK;
}

int ks_solve(ks_ctx* c, ks_result* out) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) {
        if (out) {
            std::memset(out, 0, sizeof(*out));
            out->status = g;
        }
        return g;
    }
    ks_result r;
    std::memset(&r, 0, sizeof(r));
    drop_solution(c);
    int rc = KS_OK;
    // auto-sink: the sink absorbs every other supply (its demand drifts without a
    // message in the reference, graph_manager.go:640, 808)
    if (c->opts.auto_sink && c->n_sinks == 1 && c->dev_sink_supply != -c->sum_others) {
        ks::NodeEdit e;
        std::memset(&e, 0, sizeof(e));
        e.slot = (int32_t)(c->sink_id - 1);
        e.last_rm = -1;
        e.supply = -c->sum_others;
        e.alive = 1;
        e.type = KS_NODE_SINK;
        e.was_alive = 1;
        rc = c->eng.set_nodes(&e, 1, c->err);
        if (rc == KS_OK) c->dev_sink_supply = -c->sum_others;
    }
    if (rc == KS_OK) rc = c->eng.solve(r, c->opts.warm_start != 0, c->err);
    c->map_fresh = false;
    if (rc == KS_OK) c->have_solution = true;   // r.flow_value: measured on device from the resident flow
    r.status = rc;
    if (out) *out = r;
    return rc;
}

int ks_solve_many(ks_ctx* const* ctxs, size_t k, int workers, ks_result* results) {
    if (k && !ctxs) return KS_E_INVALID;
    for (size_t i = 0; i < k; ++i)
        if (!ctxs[i]) return KS_E_INVALID;
    std::vector<int> rcs(k, KS_OK);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < k;) rcs[i] = ks_solve(ctxs[i], results ? &results[i] : nullptr);
    };
    size_t nw = workers > 0 ? (size_t)workers : 4;
    nw = std::min(nw, k);
    std::vector<std::thread> pool;
    for (size_t w = 1; w < nw; ++w) pool.emplace_back(work);
    if (nw) work();
    for (auto& t : pool) t.join();
    for (int rc : rcs)
        if (rc != KS_OK) return rc;
    return KS_OK;
}

int ks_get_flows(ks_ctx* c, ks_flow* out, size_t cap, size_t* count) {
    if (!c || !count) return KS_E_INVALID;
    if (!c->have_solution) return c->fail(KS_E_INVALID, "no successful solve on this context");
    if (!c->flows_fresh) {
        int rc = c->eng.flows(c->flows, c->err);
        if (rc) return rc;
        c->flows_fresh = true;
    }
    if (out) std::memcpy(out, c->flows.data(), std::min(cap, c->flows.size()) * sizeof(ks_flow));
    *count = c->flows.size();
    return KS_OK;
}

// Pairs from the device decomposition (Engine::task_pu): the i-th live task slot
// in slot order ↔ the i-th entry of the device vector.
int ks_get_task_mapping(ks_ctx* c, uint64_t* task, uint64_t* pu, size_t cap, size_t* count) {
    if (!c || !count) return KS_E_INVALID;
    if (!c->have_solution) return c->fail(KS_E_INVALID, "no successful solve on this context");
    // one device decomposition per solve: the usual count-then-fill call pair
    // reuses it
    if (!c->map_fresh) {
        size_t nt = 0;
        int rc = c->eng.task_pu(nullptr, 0, &nt, c->n_tasks, c->err);
        if (rc) return rc;
        uint64_t* dev = nullptr;
        rc = c->eng.scratch(&dev, nt, c->err);
        if (rc == KS_OK) rc = c->eng.task_pu(dev, nt, &nt, c->n_tasks, c->err);
        c->map_dense.resize(nt);
        if (rc == KS_OK) rc = c->eng.download(c->map_dense.data(), dev, nt * sizeof(uint64_t), c->err);
        if (rc) return rc;
        c->map_fresh = true;
    }
    const std::vector<uint64_t>& dense = c->map_dense;
    const size_t nt = dense.size();
    size_t k = 0, ti = 0;
    for (uint64_t id = 1; id < c->nodes.size() && ti < nt; ++id) {
        const NodeRec& r = c->nodes[id];
        if (!r.alive || r.type != KS_NODE_TASK) continue;
        const uint64_t p = dense[ti++];
        if (!p) continue;
        if (task && pu && k < cap) {
            task[k] = id;
            pu[k] = p;
        }
        ++k;
    }
    *count = k;
    return KS_OK;
}

int ks_get_task_pu_device(ks_ctx* c, uint64_t* dev_out, size_t cap, size_t* count) {
    if (!c || !count) return KS_E_INVALID;
    if (!c->have_solution) return c->fail(KS_E_INVALID, "no successful solve on this context");
    return c->eng.task_pu(dev_out, cap, count, c->n_tasks, c->err);
}

int ks_set_bindings(ks_ctx* c, const uint64_t* task, const uint64_t* pu, size_t k) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (k && (!task || !pu)) return c->fail(KS_E_INVALID, "null binding array");
    for (size_t i = 0; i < k; ++i) {
        if (!node_alive(c, task[i]) || c->nodes[task[i]].type != KS_NODE_TASK)
            return c->fail(KS_E_INVALID, "binding of a node that is not a live task: " + std::to_string(task[i]));
        if (pu[i] && (!node_alive(c, pu[i]) || c->nodes[pu[i]].type != KS_NODE_PU))
            return c->fail(KS_E_INVALID, "binding to a node that is not a live PU: " + std::to_string(pu[i]));
    }
    return c->eng.set_bindings(task, pu, k, c->err);
}

int ks_scheduling_deltas(ks_ctx* c, int commit, ks_sched_delta* out, size_t cap, size_t* count) {
    if (!c || !count) return KS_E_INVALID;
    if (!c->have_solution) return c->fail(KS_E_INVALID, "no successful solve on this context");
    size_t n = 0;
    int rc = c->eng.sched_deltas(0, nullptr, &n, c->n_tasks, c->err);   // count (nothing committed)
    if (rc || !out) {
        *count = n;
        return rc;
    }
    if (cap < n) {
        *count = n;
        return c->fail(KS_E_INVALID, "output buffer smaller than the delta count");
    }
    std::vector<ks_sched_delta> v;
    rc = c->eng.sched_deltas(commit, &v, &n, c->n_tasks, c->err);
    if (rc) return rc;
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(ks_sched_delta));
    *count = v.size();
    return KS_OK;
}

int ks_update_unsched_costs(ks_ctx* c, const uint64_t* ids, size_t k, int32_t mode, int64_t unsched_cost,
                            int64_t continuation_cost, size_t* changed) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (mode != KS_COST_SET && mode != KS_COST_ADD) return c->fail(KS_E_INVALID, "unknown cost mode");
    const int64_t lim = int64_t(1) << 40;
    if (unsched_cost > lim || unsched_cost < -lim || continuation_cost > lim || continuation_cost < -lim)
        return c->fail(KS_E_RANGE, "cost outside the supported range");
    if (int rc = check_aggregators(c, ids, k)) return rc;
    size_t ch = 0;
    int rc = c->eng.unsched_costs(ids, ids ? k : 0, mode, unsched_cost, continuation_cost, &ch, c->err);
    if (rc == KS_OK && ch) drop_solution(c);
    if (changed) *changed = ch;
    return rc;
}

int ks_topology_stats(ks_ctx* c, uint64_t max_tasks_per_pu, const uint64_t* pu_ids, const uint64_t* pu_running,
                      size_t k, uint64_t* slots_below, uint64_t* running_below, size_t cap, size_t* count) {
    if (!c || !count) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    const size_t n = (size_t)c->nslots();
    *count = n;
    if (!slots_below || !running_below) return KS_OK;
    if (cap < n) return c->fail(KS_E_INVALID, "output buffers smaller than the node id range");
    if (pu_ids && k && !pu_running) return c->fail(KS_E_INVALID, "null running-count array");
    for (size_t i = 0; pu_ids && i < k; ++i)
        if (!node_alive(c, pu_ids[i]) || c->nodes[pu_ids[i]].type != KS_NODE_PU)
            return c->fail(KS_E_INVALID, "running count for a node that is not a live PU");
    int rc = c->eng.topology_stats(max_tasks_per_pu, pu_ids, pu_running, pu_ids ? k : 0, sink_slot(c), slots_below,
                                   running_below, c->err);
    follow_rebuild(c);
    return rc;
}

// Both commits: the checks, the count-only call and the bookkeeping around
// run(sink slot, &deltas, &dirty), the engine call of the mode with its own stats type.
extern "C++" {
template <class Run>
static int commit_call(ks_ctx* c, int32_t flags, int64_t continuation_cost, int64_t preemption_cost,
                       const uint64_t* ids, size_t k, ks_sched_delta* out, size_t* count, Run run) {
    if (!c || !count) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (!c->have_solution) return c->fail(KS_E_INVALID, "no successful solve on this context");
    if (flags & ~KS_COMMIT_RESOURCE_CAPS) return c->fail(KS_E_INVALID, "unknown commit flag");
    const int64_t lim = int64_t(1) << 40;
    if (continuation_cost > lim || continuation_cost < -lim || preemption_cost > lim || preemption_cost < -lim)
        return c->fail(KS_E_RANGE, "cost outside the supported range");
    if (int rc = check_aggregators(c, ids, k)) return rc;
    if (!out) {   // count only
        size_t n = 0;
        const int rc = c->eng.sched_deltas(0, nullptr, &n, c->n_tasks, c->err);
        *count = n;
        return rc;
    }
    std::vector<ks_sched_delta> v;
    bool dirty = false;
    const int rc = run(sink_slot(c, true), &v, &dirty);
    if (rc) return delta_failed(c, rc, nullptr, dirty);   // (the engine writes the stats on success only)
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(ks_sched_delta));
    *count = v.size();
    drop_solution(c);
    return KS_OK;
}
}  // extern "C++"

int ks_commit_schedule(ks_ctx* c, int32_t flags, int64_t continuation_cost, const uint64_t* ids, size_t k,
                       ks_sched_delta* out, size_t cap, size_t* count, ks_commit_stats* stats) {
    return commit_call(c, flags, continuation_cost, 0, ids, k, out, count,
                       [&](int64_t sink, std::vector<ks_sched_delta>* v, bool* dirty) {
                           return c->eng.commit_schedule(flags, continuation_cost, ids, ids ? k : 0, sink, c->n_tasks,
                                                         cap, v, count, stats, dirty, c->err);
                       });
}

int ks_commit_preemptive(ks_ctx* c, int32_t flags, int64_t continuation_cost, int64_t preemption_cost,
                         const uint64_t* ids, size_t k, ks_sched_delta* out, size_t cap, size_t* count,
                         ks_preempt_stats* stats) {
    return commit_call(c, flags, continuation_cost, preemption_cost, ids, k, out, count,
                       [&](int64_t sink, std::vector<ks_sched_delta>* v, bool* dirty) {
                           return c->eng.commit_preemptive(flags, continuation_cost, preemption_cost, ids,
                                                           ids ? k : 0, sink, c->n_tasks, cap, v, count, stats, dirty,
                                                           c->err);
                       });
}

// DeregisterResource (flowscheduler/scheduler.go:162-210). The device finds the subtree, the
// evictions and the capacity records; the host's part is the node table: the removed ids
// come back before anything changes, each must be a live node that is no task and no sink
// (the roots were checked on the device, and the walk enters resources only), and they
// leave the table as the REMOVE_NODE records at stream positions 0 … n − 1 would make them.
int ks_remove_resources(ks_ctx* c, int32_t flags, const uint64_t* roots, size_t k, uint64_t* removed, size_t rcap,
                        size_t* nremoved, ks_sched_delta* evicted, size_t ecap, size_t* nevicted,
                        ks_remove_stats* stats) {
    if (!c || !nremoved || !nevicted) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (k && !roots) return c->fail(KS_E_INVALID, "null root array");
    if (flags & ~(KS_REMOVE_RESOURCE_CAPS | KS_REMOVE_PREEMPTIVE)) return c->fail(KS_E_INVALID, "unknown remove flag");
    if ((flags & KS_REMOVE_PREEMPTIVE) && !(flags & KS_REMOVE_RESOURCE_CAPS))
        return c->fail(KS_E_INVALID, "KS_REMOVE_PREEMPTIVE selects a capacity rule: it needs KS_REMOVE_RESOURCE_CAPS");
    const bool probe = !removed && !evicted;
    if (!probe && ((!removed && rcap) || (!evicted && ecap)))
        return c->fail(KS_E_INVALID, "a null output buffer with room in it");
    std::optional<NodeTxn> txn;
    int64_t pus = 0;
    auto make_edits = [&](const uint64_t* ids, size_t n, std::vector<ks::NodeEdit>* edits, std::string& err) {
        for (size_t i = 0; i < n; ++i) {
            const uint64_t id = ids[i];
            if (!node_alive(c, id) || c->nodes[id].type == KS_NODE_TASK || c->nodes[id].type == KS_NODE_SINK ||
                (i && ids[i - 1] >= id)) {
                err = "the device removes " + ks::id_name(c->view, "node", id) + ", which the host's node table does not hold as a "
                      "live resource";
                return KS_E_DEVICE;
            }
        }
        txn.emplace(c);
        for (size_t i = 0; i < n; ++i) {
            pus += c->nodes[ids[i]].type == KS_NODE_PU;
            txn->remove(ids[i], (int32_t)i);
        }
        txn->edits(*edits);
        return KS_OK;
    };
    std::vector<uint64_t> rm;
    std::vector<ks_sched_delta> ev;
    bool dirty = false;
    const int rc = c->eng.remove_resources(flags, roots, k, sink_slot(c, true), probe, removed ? rcap : 0,
                                           evicted ? ecap : 0, &rm, &ev, nremoved, nevicted, stats, make_edits, &dirty,
                                           c->err, c->view);
    follow_rebuild(c);
    // (a transaction was made only behind the device's checks, and the engine writes the stats on success only)
    if (rc) return delta_failed(c, rc, txn ? &*txn : nullptr, dirty);
    if (probe) return KS_OK;
    if (!rm.empty()) std::memcpy(removed, rm.data(), rm.size() * sizeof(uint64_t));
    if (!ev.empty()) std::memcpy(evicted, ev.data(), ev.size() * sizeof(ks_sched_delta));
    if (stats) stats->pus_removed = pus;
    drop_solution(c);
    return KS_OK;
}

// HandleTaskCompletion (flowscheduler/scheduler.go:106-132) → TaskCompleted
// (flowmanager/graph_manager.go:389-405). The device checks the ids, reads their bindings and
// generates the records; the host's part is the node table: the distinct ids come back
// ascending before anything changes, each must be a live task here too, and they leave the
// table as the REMOVE_NODE records at stream positions 0 … n − 1 would make them (n_tasks and
// the sink's auto demand follow through the edits).
int ks_complete_tasks(ks_ctx* c, int32_t flags, const uint64_t* tasks, size_t k, const uint64_t* unsched_ids, size_t nu,
                      uint64_t* left, ks_complete_stats* stats) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (k && !tasks) return c->fail(KS_E_INVALID, "null task array");
    if (flags & ~(KS_COMPLETE_RESOURCE_CAPS | KS_COMPLETE_PREEMPTIVE)) return c->fail(KS_E_INVALID, "unknown complete flag");
    if ((flags & KS_COMPLETE_PREEMPTIVE) && !(flags & KS_COMPLETE_RESOURCE_CAPS))
        return c->fail(KS_E_INVALID, "KS_COMPLETE_PREEMPTIVE selects a capacity rule: it needs KS_COMPLETE_RESOURCE_CAPS");
    if (int rc = check_aggregators(c, unsched_ids, nu)) return rc;
    std::optional<NodeTxn> txn;
    auto make_edits = [&](const uint64_t* ids, size_t n, std::vector<ks::NodeEdit>* edits, std::string& err) {
        for (size_t i = 0; i < n; ++i) {
            const uint64_t id = ids[i];
            if (!node_alive(c, id) || c->nodes[id].type != KS_NODE_TASK || (i && ids[i - 1] >= id)) {
                err = "the device completes node " + std::to_string(id) + ", which the host's node table does not hold as a "
                      "live task";
                return KS_E_DEVICE;
            }
        }
        txn.emplace(c);
        for (size_t i = 0; i < n; ++i) txn->remove(ids[i], (int32_t)i);
        txn->edits(*edits);
        return KS_OK;
    };
    bool dirty = false, changed = false;
    const int rc = c->eng.complete_tasks(flags, tasks, k, unsched_ids, unsched_ids ? nu : 0, sink_slot(c, true), left,
                                         stats, make_edits, &dirty, &changed, c->err, c->view);
    follow_rebuild(c);
    if (rc) return delta_failed(c, rc, txn ? &*txn : nullptr, dirty, stats);   // (as in ks_remove_resources)
    if (changed) drop_solution(c);
    return KS_OK;
}

// AddOrUpdateJobNodes (flowmanager/graph_manager.go:166-208). The ids are the host's part: each
// enters the node table through the ADD_NODE rule of ks_apply_deltas (NodeTxn::add), so a live
// id and an id listed twice are refused alike. The device checks the arcs' heads and costs,
// counts the aggregators' gains and generates the records; a refusal it finds takes the new
// nodes out of the table again.
int ks_add_tasks(ks_ctx* c, int32_t flags, const uint64_t* tasks, size_t k, const uint64_t* arc_off,
                 const ks_task_arc* arcs, const uint64_t* unsched_ids, size_t nu, int64_t unsched_sink_cost,
                 ks_add_stats* stats) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (flags) return c->fail(KS_E_INVALID, "unknown add flag (flags is reserved: pass 0)");
    if (k && (!tasks || !arc_off)) return c->fail(KS_E_INVALID, "null task or offset array");
    if (int rc = check_sink_cost(c, unsched_sink_cost)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!k) return KS_OK;   // nothing arrives: the solution stands
    if (int rc = check_task_lists(c, tasks, k, arc_off, arcs)) return rc;
    if (int rc = check_aggregators(c, unsched_ids, nu)) return rc;
    NodeTxn txn(c);
    for (size_t i = 0; i < k; ++i)
        if (int rc = txn.add(tasks[i], 1, KS_NODE_TASK)) {
            txn.rollback_nodes();
            return rc;
        }
    bool dirty = false;
    auto make_edits = [&](std::vector<ks::NodeEdit>* edits) { txn.edits(*edits); };
    // (a union's aggregators gain on their own cells' sinks: kEverySink; a lone context with several refuses)
    const int rc = c->eng.add_tasks(tasks, k, arc_off, arcs, unsched_ids, unsched_ids ? nu : 0, sink_slot(c, true),
                                    unsched_sink_cost, c->nslots(), stats, make_edits, &dirty, c->err, c->view);
    if (rc) return delta_failed(c, rc, &txn, dirty, stats);
    drop_solution(c);
    return KS_OK;
}

// AddResourceTopology (flowmanager/graph_manager.go:238-251). The nodes are the host's part: each
// id enters the node table through the ADD_NODE rule of ks_apply_deltas (NodeTxn::add), then its
// type and values are checked; a repeated (parent, child) pair is found by a sort. The device
// checks the edges, sums the new slots up the tree edges and generates the records; a refusal
// it finds takes the new nodes out of the table again.
int ks_add_resources(ks_ctx* c, int32_t flags, const ks_res_node* nodes, size_t n, const ks_res_arc* arcs, size_t m,
                     ks_grow_stats* stats) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (flags) return c->fail(KS_E_INVALID, "unknown flag (flags is reserved: pass 0)");
    if ((n && !nodes) || (m && !arcs)) return c->fail(KS_E_INVALID, "null node or edge array");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n && !m) return KS_OK;   // nothing joins: the solution stands
    NodeTxn txn(c);
    auto refuse = [&](int code, const std::string& msg) {
        txn.rollback_nodes();
        return c->fail(code, msg);
    };
    // under a batch view the records are graph-local (node i belongs to the last graph whose
    // node_goff is ≤ i); the node table takes the union's id
    const ks::BatchView* bv = c->view;
    auto graph_of = [&](const uint64_t* goff, size_t j) {
        return (size_t)(std::upper_bound(goff, goff + bv->ng, (uint64_t)j) - goff) - 1;
    };
    uint64_t total = 0;
    bool pu = false;
    for (size_t i = 0; i < n; ++i) {
        const ks_res_node& x = nodes[i];
        uint64_t id = x.id;
        std::string who = "resource node " + std::to_string(x.id);
        if (bv) {
            const size_t gi = graph_of(bv->node_goff, i);
            const uint64_t span = (uint64_t)(bv->off[gi + 1] - bv->off[gi]);
            who = "graph " + std::to_string(bv->graph[gi]) + ": " + who;
            if (x.id == 0 || x.id > span)
                return refuse(KS_E_RANGE, who + " is outside the graph's ids 1.." + std::to_string(span) +
                                              " (its highest id at the load plus the reserved ids)");
            id += (uint64_t)bv->off[gi];
        }
        if (int rc = txn.add(id, 0, x.type)) {
            txn.rollback_nodes();
            return rc;
        }
        if (x.type != KS_NODE_PU && x.type != KS_NODE_MACHINE && x.type != KS_NODE_INTERMEDIATE && x.type != KS_NODE_OTHER)
            return refuse(KS_E_INVALID, who + " has type " + std::to_string(x.type) + ": not a resource type");
        if (x.type == KS_NODE_PU ? x.slots == 0 : (x.slots != 0 || x.sink_cost != 0))
            return refuse(KS_E_INVALID, x.type == KS_NODE_PU ? who + " is a PU without slots"
                                                             : who + " is no PU: its slots and sink cost must be 0");
        if (x.slots > (uint64_t(1) << 53) || x.sink_cost > (int64_t(1) << 40) || x.sink_cost < -(int64_t(1) << 40))
            return refuse(KS_E_RANGE, who + ": slots or sink cost outside the supported range");
        total += x.slots;
        if (total > (uint64_t(1) << 53)) return refuse(KS_E_RANGE, who + ": the new slots summed exceed the supported range");
        pu |= x.type == KS_NODE_PU;
    }
    // (a union's PUs join their own cells' sinks: kEverySink, and the device refuses a cell without
    // exactly one; a lone context with several sinks refuses here)
    const bool every_sink = c->every_sink && c->n_sinks >= 1;
    if (pu && c->n_sinks != 1 && !every_sink)
        return refuse(KS_E_INVALID, "a new PU's arc into the sink needs exactly one sink");
    size_t first_pair = m;   // the first edge in input order that repeats an earlier (parent, child)
    {
        // (graph-local pairs: equal ones in two graphs are no repeat, so the graph leads the key)
        std::vector<size_t> order(m), eg(bv ? m : 0);
        for (size_t j = 0; j < m; ++j) order[j] = j;
        for (size_t j = 0; j < eg.size(); ++j) eg[j] = graph_of(bv->arc_goff, j);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            if (bv && eg[a] != eg[b]) return eg[a] < eg[b];
            if (arcs[a].parent != arcs[b].parent) return arcs[a].parent < arcs[b].parent;
            if (arcs[a].child != arcs[b].child) return arcs[a].child < arcs[b].child;
            return a < b;
        });
        for (size_t q = 1; q < m; ++q)
            if (arcs[order[q]].parent == arcs[order[q - 1]].parent && arcs[order[q]].child == arcs[order[q - 1]].child &&
                (!bv || eg[order[q]] == eg[order[q - 1]]))
                first_pair = std::min(first_pair, order[q]);
    }
    bool dirty = false, changed = false;
    auto make_edits = [&](std::vector<ks::NodeEdit>* edits) { txn.edits(*edits); };
    const int rc = c->eng.add_resources(nodes, n, arcs, m, first_pair,
                                        every_sink ? ks::Engine::kEverySink : sink_slot(c), c->nslots(), stats, make_edits,
                                        &dirty, &changed, c->err, bv);
    if (rc) return delta_failed(c, rc, &txn, dirty, stats);
    if (changed) drop_solution(c);
    return KS_OK;
}

// UpdateTimeDependentCosts (flowmanager/graph_manager.go:211-213) → updateTaskNode (:1183-1192).
// No node is edited, so there is no NodeTxn: the host's part is the argument, flag and range
// checks, the offsets, and the one refusal the device's index cannot see, a head listed twice
// for one task whose arc the store does not hold (found by a sort of each task's heads, as
// ks_add_resources finds a repeated pair). The device checks the ids, the heads and the costs
// and generates the records.
int ks_update_tasks(ks_ctx* c, int32_t flags, const uint64_t* tasks, size_t k, const uint64_t* arc_off,
                    const ks_task_arc* arcs, const uint64_t* unsched_ids, size_t nu, int64_t unsched_sink_cost,
                    ks_update_stats* stats) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (flags & ~KS_UPDATE_KEEP_UNLISTED) return c->fail(KS_E_INVALID, "unknown update flag");
    if (k && (!tasks || !arc_off)) return c->fail(KS_E_INVALID, "null task or offset array");
    if (int rc = check_sink_cost(c, unsched_sink_cost)) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!k) return KS_OK;   // nothing is refreshed: the solution stands
    if (int rc = check_task_lists(c, tasks, k, arc_off, arcs)) return rc;
    if (int rc = check_aggregators(c, unsched_ids, nu)) return rc;
    const size_t na = (size_t)arc_off[k];
    size_t first_pair = na;   // the first arc in input order that repeats an earlier head of its own task
    {
        std::vector<std::pair<uint64_t, size_t>> heads;
        for (size_t i = 0; i < k; ++i) {
            heads.clear();
            for (size_t j = (size_t)arc_off[i]; j < (size_t)arc_off[i + 1]; ++j) heads.emplace_back(arcs[j].dst, j);
            std::sort(heads.begin(), heads.end());
            for (size_t q = 1; q < heads.size(); ++q)
                if (heads[q].first == heads[q - 1].first) first_pair = std::min(first_pair, heads[q].second);
            if (first_pair < na) break;   // (a later task's arcs come later in input order)
        }
    }
    bool dirty = false, changed = false;
    const int rc = c->eng.update_tasks(flags, tasks, k, arc_off, arcs, first_pair, unsched_ids, unsched_ids ? nu : 0,
                                       sink_slot(c, true), unsched_sink_cost, stats, &dirty, &changed, c->err, c->view);
    follow_rebuild(c);
    if (rc) return delta_failed(c, rc, nullptr, dirty, stats);
    if (changed) drop_solution(c);
    return KS_OK;
}

// The rest of updateFlowGraph (flowmanager/graph_manager.go:1012-1033): updateEquivClassNode
// (:931-1010) and updateResourceNode (:1094-1129). No node is edited, so there is no NodeTxn: the
// host's part is the argument and flag checks, the offsets, the two range checks and a head
// listed twice for one tail (a sort of each tail's heads, as in ks_update_tasks). The device
// checks the ids and the heads and generates the records.
int ks_update_nodes(ks_ctx* c, int32_t flags, const uint64_t* nodes, size_t k, const uint64_t* arc_off,
                    const ks_node_arc* arcs, ks_node_stats* stats) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (flags & ~KS_NODES_KEEP_UNLISTED) return c->fail(KS_E_INVALID, "unknown update flag");
    if (k && (!nodes || !arc_off)) return c->fail(KS_E_INVALID, "null node or offset array");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!k) return KS_OK;   // nothing is refreshed: the solution stands
    if (arc_off[0] != 0) return c->fail(KS_E_INVALID, "arc_off[0] must be 0");
    for (size_t i = 0; i < k; ++i)
        if (arc_off[i + 1] < arc_off[i])
            return c->fail(KS_E_INVALID, "arc_off decreases at node " + std::to_string(nodes[i]));
    if (arc_off[k] && !arcs) return c->fail(KS_E_INVALID, "null arc array");
    const size_t na = (size_t)arc_off[k];
    // the first arc in input order that repeats an earlier head of its own tail, and the first
    // whose cost and whose capacity leave the range
    size_t first_pair = na, first_cost = na, first_cap = na;
    for (size_t j = 0; j < na && (first_cost == na || first_cap == na); ++j) {
        if (first_cost == na && (arcs[j].cost > (int64_t(1) << 40) || arcs[j].cost < -(int64_t(1) << 40))) first_cost = j;
        if (first_cap == na && arcs[j].cap != KS_CAP_KEEP && arcs[j].cap > (uint64_t(1) << 53)) first_cap = j;
    }
    {
        std::vector<std::pair<uint64_t, size_t>> heads;
        for (size_t i = 0; i < k; ++i) {
            heads.clear();
            for (size_t j = (size_t)arc_off[i]; j < (size_t)arc_off[i + 1]; ++j) heads.emplace_back(arcs[j].dst, j);
            std::sort(heads.begin(), heads.end());
            for (size_t q = 1; q < heads.size(); ++q)
                if (heads[q].first == heads[q - 1].first) first_pair = std::min(first_pair, heads[q].second);
            if (first_pair < na) break;   // (a later tail's arcs come later in input order)
        }
    }
    bool dirty = false, changed = false;
    const int rc = c->eng.update_nodes(flags, nodes, k, arc_off, arcs, first_pair, first_cost, first_cap, stats, &dirty,
                                       &changed, c->err, c->view);
    follow_rebuild(c);
    if (rc) return delta_failed(c, rc, nullptr, dirty, stats);
    if (changed) drop_solution(c);
    return KS_OK;
}

int ks_get_bindings(ks_ctx* c, const uint64_t* task, uint64_t* pu, size_t k) {
    if (!c) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    if (k && (!task || !pu)) return c->fail(KS_E_INVALID, "null binding array");
    for (size_t i = 0; i < k; ++i)
        if (!node_alive(c, task[i]) || c->nodes[task[i]].type != KS_NODE_TASK)
            return c->fail(KS_E_INVALID, "binding of a node that is not a live task: " + std::to_string(task[i]));
    return c->eng.get_bindings(task, pu, k, c->err);
}

int ks_get_graph(ks_ctx* c, ks_node* nodes, size_t ncap, size_t* n, ks_arc* arcs, size_t acap, size_t* m) {
    if (!c || !n || !m) return KS_E_INVALID;
    if (int g = store_guard(c)) return g;
    size_t k = 0;
    for (uint64_t id = 1; id < c->nodes.size(); ++id) {
        const NodeRec& r = c->nodes[id];
        if (!r.alive) continue;
        if (nodes && k < ncap) nodes[k] = ks_node{id, r.excess, r.type, 0};
        ++k;
    }
    *n = k;
    std::vector<ks_arc> v;
    int rc = c->eng.arcs(v, c->err);
    if (rc) return rc;
    if (arcs) std::memcpy(arcs, v.data(), std::min(acap, v.size()) * sizeof(ks_arc));
    *m = v.size();
    return KS_OK;
}

int ks_get_store_stats(ks_ctx* c, ks_store_stats* out) {
    if (!c || !out) return KS_E_INVALID;
    c->eng.store_stats(out);
    return KS_OK;
}

}  // extern "C"
