"""GPU checks of the fused negative sampler (csrc/neg_sample.hip) and of the CSR-only reconstruction-loss backward.

The reference draws negatives with torch_geometric.utils.negative_sampling (dg_ae_model_aig.py:115-119); what can be
checked of a random draw: the pairs are never edges or self loops, there are |E| + N of them, the two CSRs describe
exactly the returned pairs, sources are spread uniformly, two calls differ, and the atomic-free backward equals the
atomic one on the same pairs.

Below those three, the draw is held to tests/neg_sample_ref.py, its restatement in numpy: slot i of a call is a pure function of
(seed, i, N, the positive out-lists), and after the per-list sort so is every array of NegativeEdges.  Everything there is integer
equality, through the C ABI (mgv_neg_sample, mgv_neg_bucket, mgv_sort_lists_i32) and through sampling.negative_sampling_device."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neg_sample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _plan(dev, n_graphs=4, nodes=2048):
    import deepgate
    from deepgate import synthetic as syn
    graphs = [syn.make_graph('aig', nodes, 24, 300 + i, n_inputs=128) for i in range(n_graphs)]
    batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)
    return batch, deepgate.data.plan_of(batch, [1, 2])


def test_device_sampler_draws_valid_pairs_and_consistent_buckets():
    dev = _dev()
    from deepgate import sampling
    batch, plan = _plan(dev)
    N, E = plan.N, plan.E
    neg = sampling.negative_sampling_device(plan)
    ei = neg.edge_index.cpu().numpy()
    assert ei.shape == (2, E + N)                                   # the synthetic DAGs have no self loops
    assert ei.min() >= 0 and ei.max() < N
    assert not np.any(ei[0] == ei[1])
    pos = set((batch.edge_index[0].cpu().numpy() * N + batch.edge_index[1].cpu().numpy()).tolist())
    keys = ei[0] * N + ei[1]
    assert not any(int(k) in pos for k in keys)
    # grouped by source, and the CSRs are those pairs
    assert np.all(np.diff(ei[0]) >= 0)
    out_ptr, out_dst, in_ptr, in_src = [t.cpu().numpy() for t in neg.csr]
    assert out_ptr[0] == 0 and out_ptr[-1] == ei.shape[1] and in_ptr[-1] == ei.shape[1]
    np.testing.assert_array_equal(np.bincount(ei[0], minlength=N), np.diff(out_ptr))
    np.testing.assert_array_equal(np.bincount(ei[1], minlength=N), np.diff(in_ptr))
    np.testing.assert_array_equal(out_dst[:ei.shape[1]], ei[1])
    by_dst = np.repeat(np.arange(N), np.diff(in_ptr)) * N + in_src[:ei.shape[1]]       # (dst, src) pairs of the in-CSR
    np.testing.assert_array_equal(np.sort(by_dst), np.sort(ei[1] * N + ei[0]))
    # uniform sources: chi-square of the per-source counts against a flat expectation stays near its mean
    cnt = np.bincount(ei[0], minlength=N).astype(np.float64)
    lam = ei.shape[1] / N
    chi = ((cnt - lam) ** 2 / lam).sum()
    assert abs(chi - N) < 8 * np.sqrt(2 * N), (chi, N)
    # a second call draws other pairs
    other = sampling.negative_sampling_device(plan).edge_index.cpu().numpy()
    assert np.mean(np.sort(other[0] * N + other[1]) == np.sort(keys)) < 0.01


def test_same_seed_and_call_number_give_identical_buckets(monkeypatch):
    """The buckets are filled through atomic cursors and then sorted per list: the same draw comes out in the same order."""
    dev = _dev()
    import itertools
    from deepgate import sampling
    batch, plan = _plan(dev, n_graphs=8, nodes=2048)
    draws = []
    for _ in range(3):
        monkeypatch.setattr(sampling, '_CALLS', itertools.count())
        torch.manual_seed(1234)
        neg = sampling.negative_sampling_device(plan)
        draws.append([neg.edge_index.clone()] + [t.clone() for t in neg.csr])
    for other in draws[1:]:
        for a, b in zip(draws[0], other):
            assert torch.equal(a, b)
    ei = draws[0][0].cpu().numpy()
    out_ptr = draws[0][1].cpu().numpy()
    for n in np.random.Generator(np.random.PCG64(0)).integers(0, plan.N, size=200):
        assert np.all(np.diff(ei[1][out_ptr[n]:out_ptr[n + 1]]) >= 0)          # ascending inside a list


def test_csr_backward_equals_atomic_backward():
    dev = _dev()
    from deepgate import ops, sampling
    batch, plan = _plan(dev)
    N, H = plan.N, 64
    torch.manual_seed(3)
    st0 = (torch.randn(N, 2 * H, device=dev) * 0.3)
    neg = sampling.negative_sampling_device(plan)
    outs = []
    for csr in (neg.csr, None):
        st = st0.clone().requires_grad_(True)
        loss, counts, _ = ops.ReconLossFn.apply(st, batch.edge_index, neg.edge_index, False, plan, csr)
        (loss * 1.7).backward()
        outs.append((float(loss), st.grad.clone(), counts.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    scale = float(outs[1][1].abs().max())
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 2e-6 * max(scale, 1e-6) + 1e-9


# ---- the draw and its buckets against tests/neg_sample_ref.py ----

PAD = 16                                    # guard entries behind every output: a write past the end shows
SEEDS3 = R.SEEDS + (R.HIGH_SEED,)
ABI = [(name, k) for name in R.abi_cases(R.SEEDS[0]) for k in (0, 1)] + [('tiny 8/20', 2), ('three passes', 0)]


def _dev_arr(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan_from(dev, N, pos):
    from deepgate.graph_plan import GraphPlan
    plan = GraphPlan(_dev_arr(pos, dev), N)
    plan._check_status()
    return plan


def _abi_buffers(dev, N, E):
    return dict(src=torch.full((E + PAD,), -1, dtype=torch.int64, device=dev), dst=torch.full((E + PAD,), -1, dtype=torch.int64, device=dev),
                cnt_out=torch.zeros(N + PAD, dtype=torch.int32, device=dev), cnt_in=torch.zeros(N + PAD, dtype=torch.int32, device=dev),
                rank_out=torch.full((E + PAD,), -1, dtype=torch.int32, device=dev),
                rank_in=torch.full((E + PAD,), -1, dtype=torch.int32, device=dev))


def _abi_sample(plan, N, E, seed, b, **swap):
    from deepgate import _hip
    from deepgate._hip import ptr
    a = {k: ptr(v) for k, v in b.items()}
    a.update(swap)
    _hip.call('mgv_neg_sample', N, E, seed, ptr(plan.out_ptr), ptr(plan.out_dst), a['src'], a['dst'], a['cnt_out'], a['cnt_in'],
              a['rank_out'], a['rank_in'])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items()}


def _untouched(got, N, E, upto_E=0):
    """The guard entries (and with upto_E = 0 everything) still hold what the caller put there."""
    for k in ('src', 'dst', 'rank_out', 'rank_in'):
        assert bool((got[k][upto_E:] == -1).all()), k
    for k in ('cnt_out', 'cnt_in'):
        assert bool((got[k][(N if upto_E else 0):] == 0).all()), k


@pytest.mark.parametrize('name,k', ABI)
def test_neg_sample_equals_the_restatement_slot_by_slot(name, k):
    dev = _dev()
    seed = SEEDS3[k]
    c, ref = R.case_draw(name, seed)
    N, E = c['N'], c['E']
    plan = _plan_from(dev, N, c['pos'])
    if name == 'long out-list':             # the entry an edge walk one short would miss is the list's last on the device as well
        op = plan.out_ptr.cpu().numpy()
        assert op[R.LONG_NODE + 1] - op[R.LONG_NODE] == R.LONG_LEN and int(plan.out_dst[int(op[R.LONG_NODE + 1]) - 1]) == c['t']
        assert int(ref[2][c['slot']]) >= 1
    got = _abi_sample(plan, N, E, seed, _abi_buffers(dev, N, E))
    _untouched(got, N, E, upto_E=E)
    if E == 0:
        return _untouched(got, N, E)        # returned OK and wrote nothing
    R.assert_same_draw((got['src'][:E], got['dst'][:E]), ref)
    assert got['src'][:E].min() >= 0 and got['dst'][:E].min() >= 0          # no -1 is left
    for idx, cnt, rank in ((ref[0], got['cnt_out'][:N], got['rank_out'][:E]), (ref[1], got['cnt_in'][:N], got['rank_in'][:E])):
        np.testing.assert_array_equal(cnt, np.bincount(idx, minlength=N))
        order = np.lexsort((rank, idx))     # inside every bucket the ranks are a permutation of 0 .. count-1
        np.testing.assert_array_equal(rank[order], np.arange(E) - R._ptr(idx, N)[:-1].astype(np.int64)[idx[order]])


def _bucket_and_sort(dev, N, src, dst, rank_out, rank_in):
    """mgv_neg_bucket on given ranks, then the two list sorts, as negative_sampling_device strings them together.
    -> (the five arrays after the bucket pass, the five arrays after the sorts), numpy."""
    from deepgate import _hip
    from deepgate._hip import ptr
    E = int(src.size)
    ptrs = [_dev_arr(R._ptr(src, N), dev), _dev_arr(R._ptr(dst, N), dev)]
    s, d, ro, ri = (_dev_arr(a, dev) for a in (src, dst, rank_out, rank_in))
    srt = torch.full((2, E + PAD), -1, dtype=torch.int64, device=dev)
    out_dst, in_src = (torch.full((E + PAD,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    _hip.call('mgv_neg_bucket', E, ptr(s), ptr(d), ptr(ptrs[0]), ptr(ptrs[1]), ptr(ro), ptr(ri), ptr(srt[0]), ptr(srt[1]), ptr(out_dst), ptr(in_src))
    torch.cuda.synchronize()
    for t in (srt[0], srt[1], out_dst, in_src):
        assert bool((t[E:] == -1).all())
    filled = (srt[:, :E].cpu().numpy(), ptrs[0].cpu().numpy(), out_dst[:E].cpu().numpy(), ptrs[1].cpu().numpy(), in_src[:E].cpu().numpy())
    ss = torch.randint(-2 ** 31, 2 ** 31 - 1, (N + 1 + E,), dtype=torch.int64, device=dev).to(torch.int32)     # garbage scratch
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ptrs[0]), ptr(out_dst), ptr(ss), ss.numel())
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ptrs[1]), ptr(in_src), ptr(ss), ss.numel())
    torch.cuda.synchronize()
    assert bool((out_dst[E:] == -1).all()) and bool((in_src[E:] == -1).all())
    ei = np.stack([filled[0][0], out_dst[:E].cpu().numpy().astype(np.int64)])
    return filled, (ei, filled[1], out_dst[:E].cpu().numpy(), filled[3], in_src[:E].cpu().numpy())


@pytest.mark.parametrize('name', ('count with loops and duplicates', 'lists of 32 and 33', 'rank path'))
def test_arrival_order_does_not_reach_the_buckets(name):
    dev = _dev()
    c, d, want = R.surface_ref(name)
    N, rng = c['N'], np.random.default_rng(3)
    for how in ('ascending', 'reversed', 'random'):
        ro, ri = R.ranks(d[0], N, how, rng), R.ranks(d[1], N, how, rng)
        filled, done = _bucket_and_sort(dev, N, d[0], d[1], ro, ri)
        for g, r, what in zip(filled, R.fill(d[0], d[1], N, ro, ri), ('pairs', 'out_ptr', 'out_dst', 'in_ptr', 'in_src')):
            np.testing.assert_array_equal(g, r, err_msg='%s after the bucket pass, %s ranks' % (what, how))
        R.assert_same_buckets(done, want)


def _sort_lists(dev, ptr_np, vals_np):
    from deepgate import _hip
    from deepgate._hip import ptr
    N, E = len(ptr_np) - 1, int(vals_np.size)
    p = _dev_arr(ptr_np, dev)
    vals = torch.full((E + PAD,), -1, dtype=torch.int32, device=dev)
    vals[:E] = _dev_arr(vals_np, dev)
    ss = torch.randint(-2 ** 31, 2 ** 31 - 1, (N + 1 + E,), dtype=torch.int64, device=dev).to(torch.int32)
    _hip.call('mgv_sort_lists_i32', N, E, ptr(p), ptr(vals), ptr(ss), ss.numel())
    torch.cuda.synchronize()
    assert bool((vals[E:] == -1).all())
    return vals[:E].cpu().numpy()


@pytest.mark.parametrize('hi', (50, 2 ** 31 - 1))
def test_sort_lists_equals_a_sort_of_every_list(hi):
    """On its own, at a list on either side of every length where the path changes, with nearly all values equal (hi = 50: the
    sampler's lists hold duplicates, the plan builder's edge ids never do) and over the whole int32 range below the pad value."""
    dev = _dev()
    rng = np.random.default_rng(hi % 1000)
    for ptr_np in (R.sort_case_lengths()[0], R.many_heavy_ptr()):
        vals = rng.integers(0, hi, size=int(ptr_np[-1])).astype(np.int32)
        want = R.sort_lists(ptr_np, vals)
        got = _sort_lists(dev, ptr_np, vals)
        bad = np.flatnonzero(got != want)
        if bad.size:
            n = int(np.searchsorted(ptr_np, bad[0], side='right') - 1)
            raise AssertionError('list %d (%d entries) differs at its entry %d: %d, np.sort %d' % (n, ptr_np[n + 1] - ptr_np[n], bad[0] - ptr_np[n],
                                                                                                 got[bad[0]], want[bad[0]]))
        np.testing.assert_array_equal(_sort_lists(dev, ptr_np, vals), got)          # a repeated call is bit-identical
        np.testing.assert_array_equal(_sort_lists(dev, ptr_np, got), got)           # and sorted lists stay as they are


def test_sort_lists_with_nothing_to_sort_leaves_the_values():
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import ptr
    vals = torch.tensor([5, 3, 9, 1], dtype=torch.int32, device=dev)
    ss = torch.zeros(16, dtype=torch.int32, device=dev)
    _hip.call('mgv_sort_lists_i32', 0, 4, None, ptr(vals), None, 0)                  # no lists
    _hip.call('mgv_sort_lists_i32', 3, 0, ptr(torch.zeros(4, dtype=torch.int32, device=dev)), ptr(vals), ptr(ss), ss.numel())
    _hip.call('mgv_sort_lists_i32', 3, 0, ptr(torch.zeros(4, dtype=torch.int32, device=dev)), None, ptr(ss), ss.numel())
    torch.cuda.synchronize()
    assert vals.tolist() == [5, 3, 9, 1] and not bool(ss.any())
    with pytest.raises(_hip.HipLibraryError, match='MGV_EINVAL'):                   # scratch one int short
        _hip.call('mgv_sort_lists_i32', 2, 4, ptr(torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)), ptr(vals), ptr(ss), 2 + 1 + 4 - 1)
    torch.cuda.synchronize()
    assert vals.tolist() == [5, 3, 9, 1]


def _arrays(neg):
    return [neg.edge_index.cpu().numpy()] + [t.cpu().numpy() for t in neg.csr]


def _check_surface(N, neg, draw):
    from deepgate import sampling
    want = R.buckets(draw[0], draw[1], N)
    got = _arrays(neg)
    R.assert_same_buckets(got, want)
    again = sampling.bucket_negatives(neg.edge_index, N)                            # the second, independent builder
    R.assert_same_buckets(_arrays(again), want)
    assert got[2].dtype == np.int32 and got[0].dtype == np.int64


@pytest.mark.parametrize('name', list(R.surface_cases()))
def test_the_python_surface_equals_the_restatement(name, monkeypatch):
    dev = _dev()
    from deepgate import sampling
    c, draw, want = R.surface_ref(name)
    plan = _plan_from(dev, c['N'], c['pos'])
    monkeypatch.setattr(sampling, '_CALLS', itertools.count(c['call']))
    torch.manual_seed(c['base'])
    neg = sampling.negative_sampling_device(plan, num_neg_samples=c['num'])
    if c['num'] is None:
        loops = int((c['pos'][0] == c['pos'][1]).sum())
        assert loops > 0 and neg.edge_index.shape[1] == c['pos'].shape[1] - loops + c['N']
    _check_surface(c['N'], neg, draw)


def test_the_seed_comes_from_the_generator_and_the_call_counter(monkeypatch):
    dev = _dev()
    from deepgate import sampling
    N, pos = 64, R.tiny_graph(64, 600)
    E = R.count_of(N, pos)
    plan = _plan_from(dev, N, pos)
    # generator= : its initial_seed(), whatever torch's own seed is; 2^63 + 5 has the top bit set on the way in
    monkeypatch.setattr(sampling, '_CALLS', itertools.count(3))
    torch.manual_seed(1)
    neg = sampling.negative_sampling_device(plan, generator=torch.Generator().manual_seed(2 ** 63 + 5))
    _check_surface(N, neg, R.draw(N, E, R.seed_of(2 ** 63 + 5, 3), pos))
    # two calls on one counter: call numbers 0 and 1
    monkeypatch.setattr(sampling, '_CALLS', itertools.count())
    torch.manual_seed(1234)
    first, second = sampling.negative_sampling_device(plan), sampling.negative_sampling_device(plan)
    _check_surface(N, first, R.surface_ref('count with loops and duplicates')[1])
    _check_surface(N, second, R.draw(N, E, R.seed_of(1234, 1), pos))


def test_no_negatives_asked_for_gives_empty_buckets():
    dev = _dev()
    from deepgate import sampling
    plan = _plan_from(dev, 8, R.tiny_graph(8, 20))
    neg = sampling.negative_sampling_device(plan, num_neg_samples=0)
    assert neg.edge_index.shape == (2, 0) and neg.edge_index.dtype == torch.int64
    assert not bool(neg.out_ptr.any()) and not bool(neg.in_ptr.any()) and neg.out_ptr.numel() == 9


def test_neg_sample_refuses_what_it_cannot_draw_and_launches_nothing():
    dev = _dev()
    from deepgate import _hip
    plan = _plan_from(dev, 8, R.tiny_graph(8, 20))
    for N, swap in ((1, {}), (2 ** 31, {}), (8, dict(cnt_out=None)), (8, dict(cnt_in=None))):
        b = _abi_buffers(dev, 8, 100)
        with pytest.raises(_hip.HipLibraryError, match='MGV_EINVAL'):
            _abi_sample(plan, N, 100, R.SEEDS[0], b, **swap)
        torch.cuda.synchronize()
        _untouched({k: v.cpu().numpy() for k, v in b.items()}, 8, 100)
