"""A test-side reference of the device-resident graph store (ks_store.hip) with
the counters of ks_store_stats, for the CPU and GPU suites.

The graph state is the one graphs.apply_deltas_to_arcs keeps — nodes {id: [excess,
type]}, arcs {(s, d): (low, cap, cost)} — and that function is what edits it here,
so the two restatements cannot drift; StoreRef adds the arc type (clamped to
0..255, as the store keeps it in one byte) and, per stream, the counters
include/ksmcmf.h documents. Nothing here reads kernel state: the counters are
derived from the records and from the state before and after the stream.
"""
from __future__ import annotations

import numpy as np

from graphs import apply_deltas_to_arcs, graph_from_store

KS_REMOVE_NODE, KS_ADD_ARC, KS_UPDATE_ARC = 1, 2, 3


def _clamp_type(t: int) -> int:
    return 0 if t < 0 else (255 if t > 255 else t)


def _is_delete(x) -> bool:
    return int(x["kind"]) == KS_UPDATE_ARC and int(x["low"]) == 0 and int(x["cap"]) == 0


class StoreRef:
    """nodes {id: [excess, type]}, arcs {(s, d): (low, cap, cost)}, atype {(s, d): type}."""

    def __init__(self, nodes: dict, arcs: dict, atype: dict | None = None):
        self.nodes = nodes
        self.arcs = arcs
        self.atype = {k: 0 for k in arcs} if atype is None else atype
        assert set(self.atype) == set(self.arcs)

    @classmethod
    def from_graph(cls, g) -> "StoreRef":
        """The store after ks_load_graph(g): every node of g alive, every arc present
        (zero-capacity arcs too: only an UPDATE 0/0 record removes an arc)."""
        nodes = {i + 1: [int(g.supply[i]), int(g.ntype[i])] for i in range(g.n)}
        keys = list(zip(g.src.tolist(), g.dst.tolist()))
        arcs = {k: (int(lo), int(c), int(w)) for k, lo, c, w in zip(keys, g.low, g.cap, g.cost)}
        atype = {k: _clamp_type(int(t)) for k, t in zip(keys, g.arc_types())}
        assert len(arcs) == g.m, "one arc per ordered (src, dst) pair"
        return cls(nodes, arcs, atype)

    def copy(self) -> "StoreRef":
        return StoreRef({k: list(v) for k, v in self.nodes.items()}, dict(self.arcs), dict(self.atype))

    def graph(self):
        """The full graph a load of this state would give (auto_sink demand filled in)."""
        return graph_from_store(self.nodes, self.arcs)

    def apply(self, deltas) -> dict:
        """Apply one stream; → the ks_store_stats it must leave (include/ksmcmf.h):
          superseded       arc records followed in the stream by another arc record
                           for the same (src, dst)
          killed           keys in the store before the stream and absent after it
          live_arcs        keys after the stream
          upserts_new      keys whose last record upserts and that are new or had an
                           endpoint removed earlier in the stream (their residual
                           positions are inserted: ks_store_stats.inserted)
          upserts_inplace  keys present before and after whose last record upserts,
                           no endpoint removed in the stream (ks_store_stats.updated)
        inserted / updated equal the last two when the stream met a valid CSR and fit
        its slack (the next solve reports rebuilt == 0); otherwise they are at most
        those (an overflowed insert is left to the rebuild)."""
        before = set(self.arcs)
        apply_deltas_to_arcs(self.nodes, self.arcs, deltas)
        return self.account(before, deltas)

    def account(self, before: set, deltas) -> dict:
        """The second half of apply, for a stream that apply_deltas_to_arcs has already
        applied to this state (graphs.random_stream applies each record as it emits
        it): before is the set of arc keys the stream met."""
        after = set(self.arcs)
        last: dict = {}
        count: dict = {}
        last_rm: dict = {}
        for i, x in enumerate(deltas):
            k = int(x["kind"])
            if k == KS_REMOVE_NODE:   # (its arcs' types go below: a key is re-created only by an upsert)
                last_rm[int(x["id"])] = i
            elif k in (KS_ADD_ARC, KS_UPDATE_ARC):
                key = (int(x["src"]), int(x["dst"]))
                last[key] = i
                count[key] = count.get(key, 0) + 1
                if _is_delete(x):
                    self.atype.pop(key, None)
                else:
                    self.atype[key] = _clamp_type(int(x["type"]))
        assert after <= set(self.atype), "arc types drifted from apply_deltas_to_arcs"
        for key in set(self.atype) - after:
            del self.atype[key]
        new = inplace = 0
        for key, i in last.items():
            up = not _is_delete(deltas[i]) and all(last_rm.get(v, -1) < i for v in key)
            assert up == (key in after), key   # the LAST record decides, unless a later removal kills it
            if not up:
                continue
            if key in before and not any(v in last_rm for v in key):
                inplace += 1
            else:
                new += 1
        return {"superseded": sum(count.values()) - len(count), "killed": len(before - after),
                "live_arcs": len(after), "upserts_new": new, "upserts_inplace": inplace}

    def arc_rows(self) -> list:
        return sorted((s, d, *self.arcs[(s, d)], self.atype[(s, d)]) for s, d in self.arcs)

    def node_rows(self) -> list:
        return sorted((i, t, e) for i, (e, t) in self.nodes.items())


def same_store(ctx, ref: StoreRef) -> None:
    """ks_get_graph equals the reference exactly: the arcs as sorted (src, dst, low,
    cap, cost, type) rows, zero-capacity arcs included, and the nodes as the set of
    live ids with type and supply.

    The store leaves out one class of arc by documented design — an arc whose LAST
    record is UPDATE 0/0 (include/ksmcmf.h) — and the reference mirrors that in its
    state (apply_deltas_to_arcs pops the key), not here. A node's supply is the one
    last stated for it (load, ADD_NODE, SET_EXCESS): under auto_sink the sink's
    demand is recomputed at solve time on the device and ks_get_graph keeps
    returning the stated value, as the reference state does."""
    nodes, arcs = ctx.graph()
    dev = sorted(zip(arcs["src"].tolist(), arcs["dst"].tolist(), arcs["low"].tolist(), arcs["cap"].tolist(),
                     arcs["cost"].tolist(), arcs["type"].tolist()))
    want = ref.arc_rows()
    if dev != want:   # (a readable failure: the rows on one side only)
        ds, ws = set(dev), set(want)
        raise AssertionError(f"store arcs differ: {len(dev)} on device, {len(want)} expected; device only "
                             f"{sorted(ds - ws)[:8]}, reference only {sorted(ws - ds)[:8]}, "
                             f"repeated on device {len(dev) - len(ds)}")
    dn = sorted(zip(nodes["id"].tolist(), nodes["type"].tolist(), nodes["excess"].tolist()))
    assert dn == ref.node_rows()


def check_counters(stats: dict, want: dict, exact: bool) -> None:
    """ks_get_store_stats read right after ks_apply_deltas (a solve's auto-sink edit
    is a stream of its own and resets the per-stream counters) against
    StoreRef.apply's expectation. exact: the stream met a valid CSR and the next solve
    reported rebuilt == 0."""
    for k in ("live_arcs", "killed", "superseded"):
        assert stats[k] == want[k], (k, stats, want)
    if exact:
        assert (stats["inserted"], stats["updated"]) == (want["upserts_new"], want["upserts_inplace"]), (stats, want)
    else:
        assert 0 <= stats["inserted"] <= want["upserts_new"], (stats, want)
        assert 0 <= stats["updated"] <= want["upserts_inplace"], (stats, want)


def delta(**x):
    """One ks_delta record (native.DELTA_DT) from keywords."""
    from ksched_amd import native
    r = np.zeros(1, native.DELTA_DT)
    for k, v in x.items():
        r[0][k] = v
    return r[0]


def stream(rows) -> np.ndarray:
    from ksched_amd import native
    return np.array(list(rows), native.DELTA_DT)
