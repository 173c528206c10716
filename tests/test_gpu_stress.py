"""Differential stress: medium general graphs with hubs (tests/graphs.py
random_hub_graphs: 300–6,000 nodes, one to four nodes joined to a quarter to all
of the others, antiparallel and zero-capacity arcs, large capacities, lower
bounds out of sources, several sources and sinks) through both solver paths,
against the oracle's successive shortest path (the reference's algorithm,
placement/solver.go:32). Bit-exact cost and flow value, the oracle's verifier
on the downloaded flows, no certificate repair; an infeasible graph must fail
with KS_E_INFEASIBLE."""
import numpy as np
import pytest

from graphs import ADVERSARIAL_SEEDS, graph_from_store, random_hub_graphs, random_stream
from ksched_amd import native
from oracle import ko
from store_ref import StoreRef, check_counters, same_store
from test_gpu_parity import flows_by_arc, solve_and_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [2026, 2027])
def test_random_hub_graphs_vs_oracle(any_ctx, seed, request):
    ctx = any_ctx
    feasible = infeasible = on_cell = 0
    for trial, g in random_hub_graphs(seed, 16):
        st, cost, fv, _, _ = ko.ssp(g)
        if st == 0:
            r = solve_and_check(ctx, g, cost, fv)
            feasible += 1
            on_cell += r.raw["solver"] == 1
        else:
            ctx.load_graph(g)
            with pytest.raises(native.KsError) as ei:
                ctx.solve()
            assert ei.value.code == native.KS_E_INFEASIBLE, f"trial {trial}"
            infeasible += 1
    assert feasible >= 8 and infeasible >= 1
    # the cell path really ran the cell solver (one workgroup per graph), the engine path never
    assert on_cell == (feasible if request.node.callspec.params["any_ctx"] == "cell" else 0)


def test_resolve_is_repeatable(ctx_engine):
    """The same hub graph solved five times in a row on one context: every solve
    starts from the loaded state, so every result is the oracle's (a race in the
    hub paths would show as a different cost or a verifier failure)."""
    for trial, g in random_hub_graphs(99, 6, n_lo=4000, n_hi=6000):
        st, cost, fv, _, _ = ko.ssp(g)
        if st != 0:
            continue
        ctx_engine.load_graph(g)
        for _ in range(5):
            r = ctx_engine.solve()
            assert (r.cost, r.flow) == (cost, fv)
            assert r.raw["recoveries"] == 0


def _run_streams(ctx, seed, nrec, adversarial=False, solve_first=True):
    """Four rounds of random_stream on a feasible hub graph. After every
    ks_apply_deltas the store read back (ks_get_graph) equals the reference state and
    the path-independent counters equal its expectation (store_ref); the solve equals
    the oracle on the restated graph, its downloaded flows pass the oracle's verifier
    at that cost, or both are infeasible. → rounds solved."""
    rng = np.random.default_rng(seed)
    g = next(g for _, g in random_hub_graphs(seed, 20, n_lo=1500, n_hi=4000) if ko.ssp(g)[0] == 0)
    ref = StoreRef.from_graph(g)
    nodes, arcs = ref.nodes, ref.arcs   # the generator applies each record to them as it emits it
    ctx.load_graph(g)
    if solve_first:
        ctx.solve()
    solved = 0
    for rnd in range(4):
        before = set(arcs)
        stream = random_stream(rng, nodes, arcs, nrec, g.hubs, adversarial)
        ctx.apply_deltas(stream)
        want = ref.account(before, stream)
        same_store(ctx, ref)
        check_counters(ctx.store_stats(), want, exact=False)
        h = graph_from_store(nodes, arcs)
        st, cost, fv, _, _ = ko.ssp(h)
        if st == 0:
            r = ctx.solve()
            assert (r.cost, r.flow) == (cost, fv), f"round {rnd}"
            assert r.raw["recoveries"] == 0
            vst, vcost, _ = ko.verify(h, flows_by_arc(ctx, h))
            assert vst == 0 and vcost == cost, f"round {rnd}: the oracle's verifier rejected the downloaded flows"
            solved += 1
        else:
            with pytest.raises(native.KsError) as ei:
                ctx.solve()
            assert ei.value.code == native.KS_E_INFEASIBLE, f"round {rnd}"
    return solved


@pytest.mark.parametrize("seed,nrec", [(5, 2000), (6, 2000), (7, 20000)])
def test_random_delta_streams_match_full_graph(any_ctx, seed, nrec):
    """Random delta streams (four rounds of 2,000 or of 20,000 records) on a hub
    graph: after ks_apply_deltas the store equals the test-side restatement
    (graphs.apply_deltas_to_arcs, store_ref) arc by arc and counter by counter, and
    the device solve equals the oracle on the full graph that restatement builds,
    or both are infeasible."""
    assert _run_streams(any_ctx, seed, nrec) >= 2


@pytest.mark.parametrize("seed,solve_first", ADVERSARIAL_SEEDS)
def test_adversarial_delta_streams_match_full_graph(any_ctx, seed, solve_first):
    """The same with streams of 2,000 records that also remove a hub of the generator
    (hundreds of arcs, among removed nodes of a few) and pairs of adjacent nodes
    (graphs.random_stream, adversarial); one case applies its first stream before the
    first solve, where the removals go through the store's scan of every arc slot
    instead of the removed nodes' CSR segments. The seeds were checked on the CPU
    against the oracle to keep at least two of the four rounds feasible."""
    assert _run_streams(any_ctx, seed, 2000, adversarial=True, solve_first=solve_first) >= 2


@pytest.mark.parametrize("bad", ["missing_endpoint", "self_loop", "remove_missing", "add_present"])
def test_large_stream_error_rolls_back(ctx_engine, bad):
    """A 20,000-record stream with one bad record near its end: the call fails,
    nothing of the stream is applied (host or device: all or nothing, ks_host.cpp),
    and the valid stream alone then solves as the oracle says."""
    rng = np.random.default_rng(11)
    g = next(g for _, g in random_hub_graphs(11, 20, n_lo=3000, n_hi=5000) if ko.ssp(g)[0] == 0)
    nodes = {i + 1: [int(g.supply[i]), int(g.ntype[i])] for i in range(g.n)}
    arcs = {(int(s), int(d)): (int(lo), int(c), int(k))
            for s, d, lo, c, k in zip(g.src, g.dst, g.low, g.cap, g.cost)}
    ref = StoreRef.from_graph(g)
    ctx_engine.load_graph(g)
    ctx_engine.solve()
    before = (dict((k, list(v)) for k, v in nodes.items()), dict(arcs))
    good = random_stream(rng, nodes, arcs, 20000)
    alive = sorted(nodes)
    row = np.zeros(1, native.DELTA_DT)
    if bad == "missing_endpoint":   # (an id past every node ever present)
        row[0]["kind"], row[0]["src"], row[0]["dst"], row[0]["cap"] = native.KS_ADD_ARC, max(nodes) + 10, alive[0], 1
    elif bad == "self_loop":
        row[0]["kind"], row[0]["src"], row[0]["dst"], row[0]["cap"] = native.KS_ADD_ARC, alive[0], alive[0], 1
    elif bad == "remove_missing":
        row[0]["kind"], row[0]["id"] = native.KS_REMOVE_NODE, max(nodes) + 10
    else:
        row[0]["kind"], row[0]["id"] = native.KS_ADD_NODE, alive[1]
    stream = np.concatenate([good[:19000], row, good[19000:]])
    with pytest.raises(native.KsError) as ei:
        ctx_engine.apply_deltas(stream)
    assert ei.value.code in (native.KS_E_INVALID, native.KS_E_RANGE)
    same_store(ctx_engine, ref)   # the store read back: untouched, node table and arcs
    # nothing applied: the original graph still solves as before
    nodes, arcs = before
    h = graph_from_store(nodes, arcs)
    st, cost, fv, _, _ = ko.ssp(h)
    r = ctx_engine.solve()
    assert (r.cost, r.flow) == (cost, fv)
    # and the valid stream alone applies and solves as the restatement says
    ctx_engine.apply_deltas(good)
    from graphs import apply_deltas_to_arcs
    apply_deltas_to_arcs(nodes, arcs, good)
    h = graph_from_store(nodes, arcs)
    st, cost, fv, _, _ = ko.ssp(h)
    if st == 0:
        r = ctx_engine.solve()
        assert (r.cost, r.flow) == (cost, fv)
