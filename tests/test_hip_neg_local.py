"""The local draw of the negative sampler on the device (csrc/mgv_neg_draw.h: neg_draw_slot_local; csrc/neg_partition.hip:
mgv_neg_draw_local, mgv_neg_partition_local; sampling.negative_sampling_device(graph_ptr=, reverse=); FunctionalModel.
set_negative_sampling; Trainer with --neg_scope / --neg_reverse) against tests/neg_local_ref.py, the numpy restatement.

Every comparison is integer equality at both SEEDS: the draw probe slot by slot, the partition entry on all five arrays of NegativeEdges
at every admissible block size.  The shapes: one graph (where the entry must give mgv_neg_partition's arrays), a batch of nine graphs
whose boundaries fall inside node blocks at every shift, batches on which every attempt fails (1-node graphs, complete 2-node graphs),
empty graphs in the table, 4,096 and 4,097 graphs (the table in LDS and in memory), reversed shares of 0, 1, a quarter and all slots,
and a hub whose negative in-list passes a finishing trip (the status record shows the output-row path)."""
import functools
import itertools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neg_local_ref as L  # noqa: E402
import neg_sample_ref as R  # noqa: E402

PAD = 16                                    # guard entries behind every output and behind the workspace
SENT = -0x5A5A5A5B                          # what the workspace and the outputs hold before the call
BASES = (0, 1234)                           # torch seeds of the surface cases
CAP, CHUNK, MAX_BLOCKS, MAX_SHIFT = 16384, 16384, 2048, 12        # csrc/neg_partition.hip


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _dev_arr(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)             # (a copy: the shared cases are read-only)


def _plan_from(dev, N, pos):
    from deepgate.graph_plan import GraphPlan
    plan = GraphPlan(_dev_arr(pos, dev), N)
    plan._check_status()
    in_src, in_dst = L.plan_in_lists(pos)                    # the order the restatement reads the positive list in
    assert np.array_equal(plan.in_src.cpu().numpy(), in_src) and np.array_equal(plan.in_dst.cpu().numpy(), in_dst)
    return plan


def _local_args(dev, plan, gp, R_):
    from deepgate._hip import ptr
    table = _dev_arr(np.asarray(gp, dtype=np.int32), dev)
    return table, (R_, len(gp) - 1, ptr(table), plan.E, ptr(plan.in_src), ptr(plan.in_dst))


def _run_draw(dev, plan, N, gp, E, R_, seed):
    """mgv_neg_draw_local into sentinel-filled rows with guard entries -> (src, dst)."""
    from deepgate import _hip
    from deepgate._hip import ptr
    table, (R_, G, p_gp, Epos, p_is, p_id) = _local_args(dev, plan, gp, R_)
    out = torch.full((2, E + PAD), SENT, dtype=torch.int64, device=dev)
    _hip.call('mgv_neg_draw_local', N, E, seed, R_, G, p_gp, ptr(plan.out_ptr), ptr(plan.out_dst), Epos, p_is, p_id, ptr(out[0]), ptr(out[1]))
    torch.cuda.synchronize()
    assert bool((out[:, E:] == SENT).all()), 'the guard behind the pair rows was written'
    return out[0, :E].cpu().numpy(), out[1, :E].cpu().numpy()


def _run_part(dev, plan, N, gp, E, R_, seed, shift, entry='mgv_neg_partition_local'):
    """The partition entry into sentinel-filled outputs with guard entries and a sentinel-filled workspace.
    -> (the five arrays, status[4]); the guards and the entries behind the workspace are checked here."""
    from deepgate import _hip
    from deepgate._hip import ptr
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', N, E)
    ws = torch.full((n_ws + PAD,), SENT, dtype=torch.int32, device=dev)
    ei = torch.full((2 * E + PAD,), SENT, dtype=torch.int64, device=dev)
    out_ptr, in_ptr = (torch.full((N + 1 + PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(2))
    out_dst, in_src = (torch.full((E + PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(2))
    table, local = _local_args(dev, plan, gp, R_)
    mid = local if entry == 'mgv_neg_partition_local' else ()
    _hip.call(entry, N, E, seed, shift, ptr(plan.out_ptr), ptr(plan.out_dst), *mid, ptr(ei), ptr(out_ptr), ptr(out_dst), ptr(in_ptr),
              ptr(in_src), ptr(ws), n_ws)
    torch.cuda.synchronize()
    for t, n, what in ((ei, 2 * E, 'edge_index'), (out_ptr, N + 1, 'out_ptr'), (in_ptr, N + 1, 'in_ptr'), (out_dst, E, 'out_dst'),
                       (in_src, E, 'in_src')):
        assert bool((t[n:] == SENT).all()), 'the guard behind %s was written' % what
    assert bool((ws[n_ws:] == SENT).all()), 'entries behind the workspace were written'
    got = (ei[:2 * E].view(2, E).cpu().numpy(), out_ptr[:N + 1].cpu().numpy(), out_dst[:E].cpu().numpy(), in_ptr[:N + 1].cpu().numpy(),
           in_src[:E].cpu().numpy())
    return got, ws[:4].cpu().numpy()


def _shifts(N):
    return [s for s in range(MAX_SHIFT + 1) if -(-N // (1 << s)) <= MAX_BLOCKS]


def _trips(ptr, N, shift):
    """(finishing trips, lists finished in their output rows) of one side, from the restatement's pointer row (as
    tests/test_hip_neg_partition.py counts them)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    trips = wide = 0
    for node0 in range(0, N, 1 << shift):
        lo, end = node0, min(node0 + (1 << shift), N)
        while lo < end:
            if ptr[lo + 1] - ptr[lo] > CAP:
                hi, wide = lo + 1, wide + 1
            else:
                hi = lo + int(np.searchsorted(ptr[lo + 1:end + 1], ptr[lo] + CAP, side='right'))
            lo, trips = hi, trips + 1
    return trips, wide


@functools.lru_cache(maxsize=None)
def _one_graph_cases():
    N = 3000
    return {'3,000 nodes, three chunks and five slots': dict(N=N, E=3 * CHUNK + 5, pos=np.random.default_rng(51).integers(0, N, size=(2, 2 * N)).astype(np.int64)),
            '2 nodes complete (the cap)': dict(N=2, E=1000, pos=R.COMPLETE2)}


# ---- which cases reach the cap: no GPU ----

def test_the_cases_of_this_file_reach_the_cap_and_stay_clear_of_it():
    seed = R.SEEDS[0]
    peak = {}
    for name, c in _one_graph_cases().items():
        peak[name] = int(L.draw_local(c['N'], c['E'], seed, c['pos'], [0, c['N']], 0)[2].max())
    for name, c in L.batches().items():
        peak[name] = int(L.ref(name, L.count_of(c['N'], c['pos']), 0, seed)[0][2].max())
    c = L.hub_case()
    peak['hub'] = int(L.ref('hub', c['E'], c['R'], seed)[0][2].max())
    print(peak)
    assert [n for n, a in peak.items() if a == R.CAP] == ['2 nodes complete (the cap)', 'two 1-node graphs', 'complete 2-node graphs']
    assert peak['3,000 nodes, three chunks and five slots'] < R.CAP and peak['nine graphs'] < R.CAP and peak['hub'] < R.CAP
    assert L.GRAPH_LDS == 4096 and {len(L.batches()['%d small graphs' % G]['gp']) - 1 for G in (4096, 4097)} == {L.GRAPH_LDS, L.GRAPH_LDS + 1}
    assert int(np.diff(L.batches()['4097 small graphs']['gp']).max()) == 3 and sorted(L.DESIGNED_SIZES) == list(L.DESIGNED_SIZES)
    gp = L.batches()['nine graphs']['gp']
    for s in _shifts(int(gp[-1])):                           # a boundary inside a node block at every shift that has blocks of two nodes or more
        assert s == 0 or bool((gp[1:-1] % (1 << s) != 0).any())


# ---- 1. one graph, no reversed slot: today's entry, today's arrays ----

@pytest.mark.gpu
@pytest.mark.parametrize('seed', R.SEEDS)
@pytest.mark.parametrize('name', list(_one_graph_cases()))
def test_one_graph_and_no_reversed_slot_give_the_arrays_of_mgv_neg_partition(name, seed):
    dev = _dev()
    from deepgate import sampling
    c = _one_graph_cases()[name]
    N, E, pos = c['N'], c['E'], c['pos']
    plan = _plan_from(dev, N, pos)
    want = R.draw(N, E, seed, pos)
    R.assert_same_draw(_run_draw(dev, plan, N, [0, N], E, 0, seed), want)
    shift = sampling.partition_shift(N, E)
    new, st_new = _run_part(dev, plan, N, [0, N], E, 0, seed, shift)
    old, st_old = _run_part(dev, plan, N, [0, N], E, 0, seed, shift, entry='mgv_neg_partition')
    for a, b in zip(new, old):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(st_new, st_old)
    R.assert_same_buckets(new, R.buckets(want[0], want[1], N))


# ---- 2. / 3. the designed batches: the draw slot by slot, the partition entry at every admissible shift ----

@pytest.mark.gpu
@pytest.mark.parametrize('seed', R.SEEDS)
@pytest.mark.parametrize('name', list(L.batches()))
def test_the_designed_batches_equal_the_restatement(name, seed):
    dev = _dev()
    c = L.batches()[name]
    N, gp, pos = c['N'], c['gp'], c['pos']
    plan = _plan_from(dev, N, pos)
    for E in L.slot_counts(c):
        d, want = L.ref(name, E, 0, seed)
        R.assert_same_draw(_run_draw(dev, plan, N, gp, E, 0, seed), d)
        for shift in _shifts(N):
            got, status = _run_part(dev, plan, N, gp, E, 0, seed, shift)
            R.assert_same_buckets(got, want)
            if E:
                assert int(status[0]) == -(-N // (1 << shift))
                trips, wide = (sum(x) for x in zip(_trips(want[1], N, shift), _trips(want[3], N, shift)))
                assert (int(status[2]), int(status[3])) == (trips, wide)


# ---- 4. reversed slots ----

@pytest.mark.gpu
@pytest.mark.parametrize('seed', R.SEEDS)
def test_reversed_shares_of_none_one_a_quarter_and_all(seed):
    dev = _dev()
    from deepgate import sampling
    name = 'nine graphs'
    c = L.batches()[name]
    N, gp, pos = c['N'], c['gp'], c['pos']
    E = L.count_of(N, pos)
    plan = _plan_from(dev, N, pos)
    shift = sampling.partition_shift(N, E)
    seen = []
    for R_ in (0, 1, E // 4, E):
        d, want = L.ref(name, E, R_, seed)
        R.assert_same_draw(_run_draw(dev, plan, N, gp, E, R_, seed), d)
        got, _ = _run_part(dev, plan, N, gp, E, R_, seed, shift)
        R.assert_same_buckets(got, want)
        seen.append(got[0])
    assert not any(np.array_equal(a, b) for a, b in itertools.combinations(seen, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', R.SEEDS)
def test_a_hubs_negative_in_list_is_finished_in_its_output_rows(seed):
    dev = _dev()
    from deepgate import sampling
    c = L.hub_case()
    N, gp, pos, E, R_ = c['N'], c['gp'], c['pos'], c['E'], c['R']
    plan = _plan_from(dev, N, pos)
    d, want = L.ref('hub', E, R_, seed)
    assert int(np.diff(want[3])[L.HUB]) > CAP and int(np.bincount(pos[0], minlength=N)[L.HUB]) == L.HUB_OUT == 20000
    R.assert_same_draw(_run_draw(dev, plan, N, gp, E, R_, seed), d)
    shift = sampling.partition_shift(N, E)
    got, status = _run_part(dev, plan, N, gp, E, R_, seed, shift)
    R.assert_same_buckets(got, want)
    trips, wide = (sum(x) for x in zip(_trips(want[1], N, shift), _trips(want[3], N, shift)))
    print('hub: shift %d, %d blocks, largest %d pairs, %d trips, %d lists finished in their rows' % (shift, *status))
    assert (int(status[2]), int(status[3])) == (trips, wide) and wide == 1 and trips > 2 * int(status[0])


# ---- 5. repeats and refusals ----

@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    dev = _dev()
    name, seed = 'nine graphs', R.SEEDS[1]
    c = L.batches()[name]
    E = L.count_of(c['N'], c['pos'])
    plan = _plan_from(dev, c['N'], c['pos'])
    runs = [(_run_draw(dev, plan, c['N'], c['gp'], E, E // 4, seed), _run_part(dev, plan, c['N'], c['gp'], E, E // 4, seed, 5)) for _ in range(2)]
    for a, b in zip(runs[0][0] + runs[0][1][0] + (runs[0][1][1],), runs[1][0] + runs[1][1][0] + (runs[1][1][1],)):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_the_entries_refuse_what_the_header_says_and_write_nothing():
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import ptr
    N, E = 8, 100
    pos = R.tiny_graph(8, 20)
    plan = _plan_from(dev, N, pos)
    gp = np.array([0, 3, 8])
    table = _dev_arr(gp.astype(np.int32), dev)
    i32 = dict(dtype=torch.int32, device=dev)
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', N, E)
    ws = torch.full((n_ws,), SENT, **i32)
    ei = torch.full((2, E), SENT, dtype=torch.int64, device=dev)
    pairs = torch.full((2, E), SENT, dtype=torch.int64, device=dev)
    out_ptr, in_ptr, out_dst, in_src = (torch.full((n,), SENT, **i32) for n in (N + 1, N + 1, E, E))
    local = dict(R=25, G=2, graph_ptr=ptr(table), Epos=plan.E, pos_in_src=ptr(plan.in_src), pos_in_dst=ptr(plan.in_dst))
    part = dict(N=N, E=E, seed=R.SEEDS[0], shift=0, pos_ptr=ptr(plan.out_ptr), pos_dst=ptr(plan.out_dst), **local, ei=ptr(ei),
                out_ptr=ptr(out_ptr), out_dst=ptr(out_dst), in_ptr=ptr(in_ptr), in_src=ptr(in_src), ws=ptr(ws), ws_ints=n_ws)
    draw = dict(N=N, E=E, seed=R.SEEDS[0], R=25, G=2, graph_ptr=ptr(table), pos_ptr=ptr(plan.out_ptr), pos_dst=ptr(plan.out_dst), Epos=plan.E,
                pos_in_src=ptr(plan.in_src), pos_in_dst=ptr(plan.in_dst), neg_src=ptr(pairs[0]), neg_dst=ptr(pairs[1]))
    own = [dict(G=0), dict(R=-1), dict(R=E + 1), dict(Epos=0), dict(graph_ptr=None), dict(pos_in_src=None), dict(pos_in_dst=None)]
    sizes = [dict(N=1), dict(N=1 << 31), dict(E=-1, R=0), dict(E=1 << 28), dict(pos_ptr=None)]
    for change in own + sizes + [dict(ws_ints=n_ws - 1)] + [{k: None} for k in ('ei', 'out_ptr', 'out_dst', 'in_ptr', 'in_src', 'ws')]:
        with pytest.raises(_hip.HipLibraryError, match='MGV_EINVAL'):
            _hip.call('mgv_neg_partition_local', *dict(part, **change).values())
    for shift in (-1, MAX_SHIFT + 1):
        with pytest.raises(_hip.HipLibraryError, match='MGV_EUNSUPPORTED'):
            _hip.call('mgv_neg_partition_local', *dict(part, shift=shift).values())
    for change in own + sizes + [dict(neg_src=None), dict(neg_dst=None)]:
        with pytest.raises(_hip.HipLibraryError, match='MGV_EINVAL'):
            _hip.call('mgv_neg_draw_local', *dict(draw, **change).values())
    torch.cuda.synchronize()
    for t in (ws, ei, pairs, out_ptr, in_ptr, out_dst, in_src):
        assert bool((t == SENT).all())                       # a refused call writes nothing
    # and the good calls are good
    _hip.call('mgv_neg_partition_local', *part.values())
    _hip.call('mgv_neg_draw_local', *draw.values())
    torch.cuda.synchronize()
    d = L.draw_local(N, E, R.SEEDS[0], pos, gp, 25)
    R.assert_same_draw((pairs[0].cpu().numpy(), pairs[1].cpu().numpy()), d)
    R.assert_same_buckets((ei.cpu().numpy(), out_ptr.cpu().numpy(), out_dst.cpu().numpy(), in_ptr.cpu().numpy(), in_src.cpu().numpy()),
                          R.buckets(d[0], d[1], N))


# ---- 6. the Python surface ----

def _arrays(neg):
    return [neg.edge_index.cpu().numpy()] + [t.cpu().numpy() for t in neg.csr]


@pytest.mark.gpu
@pytest.mark.parametrize('partition', (True, False))
@pytest.mark.parametrize('base', BASES)
def test_the_sampler_equals_the_restatement_on_both_routes(base, partition, monkeypatch):
    dev = _dev()
    from deepgate import _hip, sampling
    name = 'nine graphs'
    c = L.batches()[name]
    N, pos = c['N'], c['pos']
    gp = torch.from_numpy(np.array(c['gp']))
    plan = _plan_from(dev, N, pos)
    monkeypatch.setattr(sampling, 'PARTITION', partition)
    called = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda entry, *a: (called.append(entry), real(entry, *a))[1])
    E = L.count_of(N, pos)
    for call, (num, rev) in enumerate(((None, 0.25), (1000, 1.0), (None, 0.0), (0, 0.5))):
        monkeypatch.setattr(sampling, '_CALLS', itertools.count(call))
        torch.manual_seed(base)
        neg = sampling.negative_sampling_device(plan, num_neg_samples=num, graph_ptr=gp, reverse=rev)
        torch.cuda.synchronize()
        assert next(sampling._CALLS) == call + 1             # one call, one number
        n = E if num is None else num
        d = L.draw_local(N, n, R.seed_of(base, call), pos, c['gp'], L.reverse_count(rev, n))
        assert neg.edge_index.dtype == torch.int64 and all(t.dtype == torch.int32 for t in neg.csr)
        R.assert_same_buckets(_arrays(neg), R.buckets(d[0], d[1], N))
    assert ('mgv_neg_partition_local' in called) == partition and 'mgv_neg_draw_local' in called      # (an empty draw takes the draw entry)
    assert 'mgv_neg_partition' not in called and 'mgv_neg_sample' not in called
    assert plan._graph_ptr_i32[0] is gp and plan._graph_ptr_i32[1].dtype == torch.int32              # uploaded once, kept on the plan
    # reverse alone: the batch as one graph
    monkeypatch.setattr(sampling, '_CALLS', itertools.count(0))
    torch.manual_seed(base)
    neg = sampling.negative_sampling_device(plan, reverse=0.5)
    d = L.draw_local(N, E, R.seed_of(base, 0), pos, [0, N], L.reverse_count(0.5, E))
    R.assert_same_buckets(_arrays(neg), R.buckets(d[0], d[1], N))
    with pytest.raises(ValueError, match='graph_ptr'):
        sampling.negative_sampling_device(plan, graph_ptr=torch.tensor([0, 5, N - 1]))
    with pytest.raises(ValueError, match='reverse'):
        sampling.negative_sampling_device(plan, graph_ptr=gp, reverse=1.5)


@pytest.mark.gpu
@pytest.mark.parametrize('base', BASES)
def test_the_defaults_make_todays_calls_and_todays_arrays(base, monkeypatch):
    dev = _dev()
    from deepgate import _hip, sampling
    c = L.batches()['nine graphs']
    N, pos = c['N'], c['pos']
    plan = _plan_from(dev, N, pos)
    called = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda entry, *a: (called.append(entry), real(entry, *a))[1])
    monkeypatch.setattr(sampling, '_CALLS', itertools.count(0))
    torch.manual_seed(base)
    neg = sampling.negative_sampling_device(plan, graph_ptr=None, reverse=0.0)
    assert next(sampling._CALLS) == 1 and called == ['mgv_neg_partition']
    d = R.draw(N, L.count_of(N, pos), R.seed_of(base, 0), pos)
    R.assert_same_buckets(_arrays(neg), R.buckets(d[0], d[1], N))
    assert not hasattr(plan, '_graph_ptr_i32')


def _aig_model(dev, seed=5):
    import deepgate
    torch.manual_seed(seed)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=64, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


@functools.lru_cache(maxsize=None)
def _graphs():
    """Three 150-gate synthetic circuits without fixed negatives: the sampler draws them."""
    from deepgate import synthetic as syn
    graphs = [syn.make_graph('aig', 150, 8, 9100 + i, n_inputs=22) for i in range(3)]
    for g in graphs:
        g.pop('neg_edge_index', None)
    return graphs


def _batch(dev):
    import deepgate
    from deepgate import synthetic as syn
    return deepgate.CircuitBatch.from_arrays(syn.collate(_graphs()), device=dev)


@pytest.mark.gpu
def test_recon_loss_hands_the_sampler_its_setting_and_is_the_loss_of_those_pairs(monkeypatch):
    dev = _dev()
    from deepgate import _model_base, ops, sampling
    model = _aig_model(dev).train()
    batch = _batch(dev)
    assert getattr(batch, 'neg_edge_index', None) is None and batch.graph_ptr.tolist() == [0, 150, 300, 450]
    with torch.no_grad():
        hs, _ = model(batch)
    plan = batch._mgv_plan
    seen = []

    def spy(*args, **kw):
        out = sampling.negative_sampling_device(*args, **kw)
        seen.append((args, kw, out))
        return out

    monkeypatch.setattr(_model_base, 'negative_sampling_device', spy)
    loss0, _, _ = model.recon_loss(hs, batch.edge_index, want_pred=False, plan=plan, graph_ptr=batch.graph_ptr)
    assert seen[-1][:2] == ((plan,), {})                      # the default: today's call, the table ignored
    assert model.set_negative_sampling('graph', 0.25) is model
    with pytest.raises(ValueError, match='graph_ptr'):
        model.recon_loss(hs, batch.edge_index, want_pred=False, plan=plan)
    with pytest.raises(ValueError, match='graph_ptr'):
        model.link_metrics(hs, batch.edge_index, plan=plan)
    assert len(seen) == 1
    loss, _, _ = model.recon_loss(hs, batch.edge_index, want_pred=False, plan=plan, graph_ptr=batch.graph_ptr, want_rank=True)
    args, kw, neg = seen[-1]
    assert args == (plan,) and set(kw) == {'graph_ptr', 'reverse'} and kw['graph_ptr'] is batch.graph_ptr and kw['reverse'] == 0.25
    st = ops.linear(hs, model.hs_decompose.weight, model.hs_decompose.bias)
    direct = ops.ReconLossFn.apply(st, batch.edge_index, neg.edge_index, False, plan, neg.csr, 1.0)[0]
    assert torch.equal(loss, direct) and bool(torch.isfinite(loss)) and not torch.equal(loss, loss0)
    # want_rank ranks the same local negatives; link_metrics draws its own the same way
    assert torch.equal(model.last_link_metrics.view(torch.int64), ops.link_record(st, None, batch.edge_index, neg.edge_index).view(torch.int64))
    rec = model.link_metrics(hs, batch.edge_index, plan=plan, graph_ptr=batch.graph_ptr)
    assert seen[-1][1]['graph_ptr'] is batch.graph_ptr and int(rec.view(torch.int64)[4]) == neg.edge_index.shape[1]
    # the drawn pairs are local and a quarter of them reversed links
    ei, gp = neg.edge_index.cpu().numpy(), batch.graph_ptr.numpy()
    pos = batch.edge_index.cpu().numpy()
    keys = set((pos[0] * 450 + pos[1]).tolist())
    is_rev = np.array([k in keys for k in (ei[1] * 450 + ei[0]).tolist()])
    assert bool((np.searchsorted(gp, ei[0], 'right') == np.searchsorted(gp, ei[1], 'right'))[~is_rev].all())
    assert int(is_rev.sum()) >= L.reverse_count(0.25, ei.shape[1])
    # scope='batch' with a reversed share: no table handed on
    model.set_negative_sampling('batch', 0.5)
    model.recon_loss(hs, batch.edge_index, want_pred=False, plan=plan, graph_ptr=batch.graph_ptr)
    assert seen[-1][1] == {'graph_ptr': None, 'reverse': 0.5}


# ---- 7. the Trainer ----

def _train_two_steps(dev, tmp_path, tid, **flags):
    import deepgate
    from deepgate import sampling
    sampling._CALLS = itertools.count()
    model = _aig_model(dev).train()
    torch.manual_seed(11)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE', **flags), model, training_id=tid, save_dir=str(tmp_path), lr=1e-3,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=3, distributed=False)
    batch = _batch(dev)
    losses = [tr.train_step(batch)['recon_loss'].item() for _ in range(2)]
    torch.cuda.synchronize()
    return tr.optimizer.flat_buffers()['param'].detach().cpu().numpy().tobytes(), losses


@pytest.mark.gpu
def test_train_steps_with_the_flags_repeat_bit_for_bit_and_differ_from_the_batch_scope(tmp_path, monkeypatch):
    dev = _dev()
    from deepgate import sampling
    monkeypatch.setattr(sampling, '_CALLS', itertools.count())          # (restored afterwards; _train_two_steps resets it per run)
    a, la = _train_two_steps(dev, tmp_path, 'a', neg_scope='graph', neg_reverse=0.25)
    b, lb = _train_two_steps(dev, tmp_path, 'b', neg_scope='graph', neg_reverse=0.25)
    c, lc = _train_two_steps(dev, tmp_path, 'c')
    assert a == b and la == lb and all(np.isfinite(la + lc))
    assert a != c and la != lc


@pytest.mark.gpu
def test_val_auc_prints_its_line_under_the_flags(tmp_path):
    dev = _dev()
    import deepgate
    model = _aig_model(dev)
    args = types.SimpleNamespace(model='DG_AE', val_auc=True, neg_scope='graph', neg_reverse=0.25)
    tr = deepgate.Trainer(args, model, training_id='v', save_dir=str(tmp_path), lr=1e-4, rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0',
                          batch_size=3, distributed=False)
    assert (model._neg_scope, model._neg_reverse) == ('graph', 0.25)
    tr.train(1, list(_graphs()), list(_graphs()))
    val = [ln for ln in open(tr.log_path).read().splitlines() if ln.startswith('val|')]
    assert len(val) == 1
    m = re.search(r' \|AUC: (\d\.\d{4}) \|AP: (\d\.\d{4})$', val[0])
    assert m, val[0]
    assert 0.0 <= float(m.group(1)) <= 1.0 and 0.0 < float(m.group(2)) <= 1.0
