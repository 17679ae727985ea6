"""tests/neg_local_ref.py pinned on the CPU: the local draw's restatement against neg_sample_ref.draw where the two must agree, its
pairs against what the header promises (one graph per local pair, a listed edge behind every reversed pair), its distribution against
a chi-square, planted defects against the comparison helper the GPU file uses; then the host side: the graph-table validation, R from
`reverse`, the torch route, the flags, the header's declarations and every refusal of the two entries as a return code (no GPU).

The statistical bound is that of tests/test_neg_sample_spec.py: z = (chi^2 - (cells - 1)) / sqrt(2 (cells - 1)), |z| <= 4, per graph over
its allowed cells (s, d - graph_ptr[g]) and once over the batch with every cell weighted 1 / n_g (the proposal draws s over the batch,
d over the n_g nodes of s's graph, and starts afresh after a rejection).  Measured once on graphs of 4 / 6 / 9 / 13 nodes, 200,000
draws (per graph, then the batch's 248 cells; the seeds seed_of(1234, 0), seed_of(0, 7), seed_of(2^63 + 5, 3)):

      -0.58   1.88  -0.75  -0.07   -0.04
       1.43  -0.11  -1.19  -0.43   -0.41
       0.26  -1.11   0.46   0.43    0.30

No input had to be changed to stay inside the bound."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neg_local_ref as L  # noqa: E402
import neg_sample_ref as R  # noqa: E402

from deepgate import _hip  # noqa: E402

CHI_SEEDS = (R.seed_of(1234, 0), R.seed_of(0, 7), R.seed_of(2 ** 63 + 5, 3))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _graph_of(gp, ids):
    return np.searchsorted(gp, ids, side='right') - 1


def test_one_graph_and_no_reversed_slot_is_todays_draw():
    for N, P, E in R.TINY:
        pos = R.tiny_graph(N, P)
        for seed in R.SEEDS + (R.HIGH_SEED,):
            want = R.draw(N, E // 10, seed, pos)
            got = L.draw_local(N, E // 10, seed, pos, [0, N], 0)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
    for seed in R.SEEDS:                                      # the cap case and the long out-list as well
        for name in ('2 nodes complete (the cap)', 'long out-list', 'E=0'):
            c, want = R.case_draw(name, seed)
            got = L.draw_local(c['N'], c['E'], seed, c['pos'], [0, c['N']], 0)
            R.assert_same_draw(got, want)
            assert np.array_equal(got[2], want[2])


def test_every_accepted_local_pair_lies_in_one_graph_and_every_reversed_pair_reverses_a_listed_edge():
    for name, c in L.batches().items():
        gp, N, pos = c['gp'], c['N'], c['pos']
        keys = set((pos[0] * N + pos[1]).tolist())
        E = L.count_of(N, pos)
        for R_ in (0, E // 4) if pos.shape[1] else (0,):
            for seed in R.SEEDS:
                (s, d, a), _ = L.ref(name, E, R_, seed)
                assert s.min() >= 0 and s.max() < N and d.min() >= 0 and d.max() < N
                loc = np.arange(E) >= R_
                assert np.array_equal(_graph_of(gp, s[loc]), _graph_of(gp, d[loc])), name          # capped slots included
                acc = a < R.CAP
                assert not bool((s[acc] == d[acc]).any()) and not any(k in keys for k in (s[acc] * N + d[acc]).tolist())
                assert all(k in keys for k in (d[~loc] * N + s[~loc]).tolist()), name             # (d, s) is a listed edge, capped or not
    # the hub: every slot reversed
    c = L.hub_case()
    (s, d, a), b = L.ref('hub', c['E'], c['R'], R.SEEDS[0])
    keys = set((c['pos'][0] * c['N'] + c['pos'][1]).tolist())
    assert all(k in keys for k in (d * c['N'] + s).tolist())
    assert int(np.diff(b[3])[L.HUB]) > L.NP_CAP                                                  # node 5's negative in-list passes a trip


def test_the_cases_reach_the_cap_and_stay_clear_of_it():
    """From the restatement's attempts: which cases keep the pair of attempt 64 and which accept every slot before it."""
    at_cap, clear = [], []
    for name, c in L.batches().items():
        E = L.count_of(c['N'], c['pos'])
        a = L.ref(name, E, 0, R.SEEDS[0])[0][2]
        (at_cap if int(a.max()) == R.CAP else clear).append(name)
        print('%-28s E=%-6d attempts up to %d' % (name, E, a.max()))
    # (a rejected slot draws its source afresh: the 1- and 2-node graphs of the nine cost an attempt or two, not the cap)
    assert at_cap == ['two 1-node graphs', 'complete 2-node graphs'] and 'nine graphs' in clear and 'empty graphs in the table' in clear
    for name in ('two 1-node graphs', 'complete 2-node graphs'):                                  # every slot runs all 65 attempts
        c = L.batches()[name]
        assert bool((L.ref(name, L.count_of(c['N'], c['pos']), 0, R.SEEDS[0])[0][2] == R.CAP).all())


def test_the_local_draw_is_uniform_inside_every_graph():
    gp = L.table_of((4, 6, 9, 13))
    N, E = int(gp[-1]), 200000
    pos = L.edges_inside(gp, 1, np.random.default_rng(41))
    assert bool((pos[0] == pos[1]).any()) and np.unique(pos[0] * N + pos[1]).size < pos.shape[1]   # self loops and duplicates left in
    n_of = np.diff(gp)[_graph_of(gp, np.arange(N))]
    allowed = _graph_of(gp, np.arange(N))[:, None] == _graph_of(gp, np.arange(N))[None, :]
    allowed[pos[0], pos[1]] = False
    allowed[np.arange(N), np.arange(N)] = False
    weight = np.where(allowed, 1.0 / n_of[:, None], 0.0)
    for k, seed in enumerate(CHI_SEEDS):
        s, d, a = L.draw_local(N, E, seed, pos, gp, 0)
        cnt = np.bincount(s * N + d, minlength=N * N).reshape(N, N)
        assert int(cnt[~allowed].sum()) == 0 and int(a.max()) < R.CAP
        zs = []
        for g in range(gp.size - 1):
            blk = (slice(gp[g], gp[g + 1]),) * 2
            c_g, ok = cnt[blk][allowed[blk]], int(allowed[blk].sum())
            lam = c_g.sum() / ok
            zs.append((((c_g - lam) ** 2 / lam).sum() - (ok - 1)) / np.sqrt(2 * (ok - 1)))
        lam = E * weight[allowed] / weight.sum()
        cells = int(allowed.sum())
        zs.append((((cnt[allowed] - lam) ** 2 / lam).sum() - (cells - 1)) / np.sqrt(2 * (cells - 1)))
        print('seed %d: z per graph %s, over the batch (%d cells) %.2f' % (k, ' '.join('%.2f' % z for z in zs[:-1]), cells, zs[-1]))
        assert all(abs(z) <= 4 for z in zs), (k, zs)


def _raises(fn, *args):
    with pytest.raises(AssertionError) as info:
        fn(*args)
    return str(info.value)


def test_planted_defects_change_the_draw_on_the_shared_cases():
    name = 'nine graphs'
    c = L.batches()[name]
    E = L.count_of(c['N'], c['pos'])
    for seed in R.SEEDS:
        for R_ in (0, E // 4):
            want = L.ref(name, E, R_, seed)[0]
            R.assert_same_draw(L.draw_local(c['N'], E, seed, c['pos'], c['gp'], R_), want)
            for defect in L.DEFECTS:
                got = L.draw_local(c['N'], E, seed, c['pos'], c['gp'], R_, defect=defect)
                reversed_only = defect in ('not_reversed', 'e_from_lo', 'rev_le_R')
                if reversed_only and R_ == 0 and defect != 'rev_le_R':
                    R.assert_same_draw(got, want)            # no reversed slot, nothing to get wrong: stated, not hidden
                else:
                    _raises(R.assert_same_draw, got, want)
        # slot R itself is the first that 'rev_le_R' changes
        got = L.draw_local(c['N'], E, seed, c['pos'], c['gp'], E // 4, defect='rev_le_R')
        assert 'slot %d of' % (E // 4) in _raises(R.assert_same_draw, got, L.ref(name, E, E // 4, seed)[0])
    # the boundary id: a source that is the first node of its graph is what a lower bound files under the graph before
    c = L.batches()['empty graphs in the table']
    got = L.draw_local(9, 2000, R.SEEDS[0], c['pos'], c['gp'], 0, defect='lower_bound')
    want = L.draw_local(9, 2000, R.SEEDS[0], c['pos'], c['gp'], 0)
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    first = bad[want[2][bad] == 0]                           # accepted at attempt 0: only the graph lookup can have moved them
    assert first.size and bool(np.isin(want[0][first], (0, 5)).all())
    assert set(L.DEFECTS) == {'d_global', 'graph_from_d', 'next_ptr', 'lower_bound', 'not_reversed', 'e_from_lo', 'rev_le_R'}


# ---- the host side ----

def test_the_host_validates_the_graph_table_and_reverse():
    from deepgate import sampling
    gp = sampling.check_graph_ptr(torch.tensor([0, 0, 5, 5, 9]), 9)
    assert gp.dtype == torch.int64 and gp.tolist() == [0, 0, 5, 5, 9]
    assert sampling.check_graph_ptr(np.array([0, 9]), 9).tolist() == [0, 9] and sampling.check_graph_ptr([0, 4, 9], 9).tolist() == [0, 4, 9]
    for bad, N in (([0], 0), ([], 0), ([1, 9], 9), ([0, 8], 9), ([0, 10], 9), ([0, 5, 4, 9], 9), ([0, -1, 9], 9)):
        with pytest.raises(ValueError, match='graph_ptr'):
            sampling.check_graph_ptr(torch.tensor(bad, dtype=torch.int64), N)
    for rev, E, want in ((0.0, 100, 0), (1.0, 100, 100), (0.25, 10, 3), (0.25, 9, 2), (0.24, 10, 2), (0.5, 1, 1), (0.49, 1, 0), (0.3, 0, 0)):
        assert sampling.reverse_count(rev, E) == want == L.reverse_count(rev, E), (rev, E)
    for rev in (-0.01, 1.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='reverse'):
            sampling.reverse_count(rev, 10)
    import inspect
    p = inspect.signature(sampling.negative_sampling_device).parameters
    assert list(p) == ['plan', 'num_neg_samples', 'generator', 'graph_ptr', 'reverse'] and p['graph_ptr'].default is None and p['reverse'].default == 0.0
    p = inspect.signature(sampling.negative_sampling).parameters
    assert p['graph_ptr'].default is None and p['reverse'].default == 0.0


def test_the_torch_route_draws_inside_the_graphs_and_reverses_listed_edges():
    from deepgate import sampling
    c = L.batches()['nine graphs']
    gp, N, pos = c['gp'], c['N'], torch.from_numpy(np.array(c['pos']))
    keys = set((pos[0] * N + pos[1]).tolist())
    want = L.count_of(N, c['pos'])
    g = torch.Generator().manual_seed(5)
    neg = sampling.negative_sampling(pos, N, generator=g, graph_ptr=torch.from_numpy(np.array(gp)), reverse=0.25).numpy()
    R_ = L.reverse_count(0.25, want)
    assert neg.shape == (2, want) and neg.dtype == np.int64 and neg.min() >= 0 and neg.max() < N
    assert not bool((neg[0] == neg[1]).any()) and not any(k in keys for k in (neg[0] * N + neg[1]).tolist())
    assert all(k in keys for k in (neg[1][:R_] * N + neg[0][:R_]).tolist())
    assert np.array_equal(_graph_of(gp, neg[0][R_:]), _graph_of(gp, neg[1][R_:]))
    sizes = np.bincount(_graph_of(gp, neg[0][R_:]), minlength=9)
    assert sizes[-1] > 0.35 * (want - R_) and sizes[-2] > 0.35 * (want - R_)                     # sources over the batch: the two large graphs
    # the defaults are the batch-wide draw of the same generator, call for call
    a = sampling.negative_sampling(pos, N, generator=torch.Generator().manual_seed(9))
    b = sampling.negative_sampling(pos, N, generator=torch.Generator().manual_seed(9), graph_ptr=None, reverse=0.0)
    assert torch.equal(a, b) and bool((torch.from_numpy(_graph_of(gp, a[0].numpy())) != torch.from_numpy(_graph_of(gp, a[1].numpy()))).any())
    with pytest.raises(ValueError, match='graph_ptr'):
        sampling.negative_sampling(pos, N, graph_ptr=[0, N - 1])
    with pytest.raises(ValueError, match='reverse'):
        sampling.negative_sampling(pos, N, reverse=1.5)


def test_the_models_setting_is_checked_and_stays_out_of_the_state_dict():
    import deepgate
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=16, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=16)
    before = set(model.state_dict())
    assert (model._neg_scope, model._neg_reverse) == ('batch', 0.0)
    assert model.set_negative_sampling('graph', 0.25) is model and (model._neg_scope, model._neg_reverse) == ('graph', 0.25)
    assert set(model.state_dict()) == before
    for scope, rev in (('node', 0.0), ('graph', -0.1), ('graph', 1.5), (None, 0.0)):
        with pytest.raises(ValueError):
            model.set_negative_sampling(scope, rev)
    assert (model._neg_scope, model._neg_reverse) == ('graph', 0.25)
    # scope='graph' without the table names the argument, on the torch route as on the device's
    pos = torch.from_numpy(R.tiny_graph(8, 20))
    with pytest.raises(ValueError, match='graph_ptr'):
        model._draw_negatives(torch.zeros(8, 16), pos, None)
    neg = model._draw_negatives(torch.zeros(8, 16), pos, None, graph_ptr=torch.tensor([0, 3, 8]))
    assert neg.shape[0] == 2 and bool(((neg[0] < 3) == (neg[1] < 3))[L.reverse_count(0.25, neg.shape[1]):].all())


def test_the_new_flags_defaults_and_parsing():
    from config import get_parse_args
    a = get_parse_args(['--type', 'aig'])
    assert a.neg_scope == 'batch' and a.neg_reverse == 0.0
    a = get_parse_args(['--type', 'aig', '--neg_scope', 'graph', '--neg_reverse', '0.25'])
    assert a.neg_scope == 'graph' and a.neg_reverse == 0.25 and a.val_auc is False
    with pytest.raises(SystemExit):
        get_parse_args(['--type', 'aig', '--neg_scope', 'node'])
    import inspect

    import config
    text = inspect.getsource(config)
    assert text.count('dg_ae_model_aig.py:115-119') >= 2                                          # both help texts cite the reference's draw


def test_the_header_declares_both_entries_with_their_reference_lines_and_refusals():
    sigs = _hip.parse_header()
    assert len(sigs['mgv_neg_draw_local']) == 14 and len(sigs['mgv_neg_partition_local']) == 20
    assert len(sigs['mgv_neg_partition']) == 14 and len(sigs['mgv_neg_sample']) == 12            # the entries beside them are as they were
    text = open(_hip.HEADER_PATH).read()
    at = text.index('negative sampling inside each circuit')
    block = text[at:text.index('int mgv_neg_partition_local(')]
    assert 'dg_ae_model_aig.py:115-119' in block and 'int mgv_neg_draw_local(' in block
    order = ['G < 1', 'R < 0 or R > E', 'R > 0 with Epos < 1', 'a NULL\n * graph_ptr', 'a NULL pos_in_src or pos_in_dst with R > 0']
    places = [block.index(w) for w in order]
    assert places == sorted(places) and 'MGV_EINVAL' in block and 'MGV_EUNSUPPORTED' in block
    assert 'clamped into [0, N]' in block and '4,096 graphs' in block
    lib = _hip.load()
    assert hasattr(lib, 'mgv_neg_draw_local') and hasattr(lib, 'mgv_neg_partition_local')


def P(k):
    return ctypes.c_void_p(64 * k)


def _call(name, good, over):
    assert set(over) <= {k for k, _ in good}, over
    return getattr(_hip.load(), name)(*[over.get(k, v) for k, v in good], None)


def test_every_refusal_of_both_entries_is_a_return_code():
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', 8, 100)
    local = [('R', 25), ('G', 2), ('graph_ptr', P(3)), ('Epos', 20), ('pos_in_src', P(4)), ('pos_in_dst', P(5))]
    draw = [('N', 8), ('E', 100), ('seed', 1)] + local[:3] + [('pos_out_ptr', P(1)), ('pos_out_dst', P(2))] + local[3:] + [('neg_src', P(6)), ('neg_dst', P(7))]
    part = ([('N', 8), ('E', 100), ('seed', 1), ('shift', 0), ('pos_out_ptr', P(1)), ('pos_out_dst', P(2))] + local
            + [('edge_index', P(6)), ('out_ptr', P(7)), ('out_dst', P(8)), ('in_ptr', P(9)), ('in_src', P(10)), ('ws', P(11)), ('ws_ints', n_ws)])
    own = [{'G': 0}, {'G': -1}, {'R': -1}, {'R': 101}, {'Epos': 0}, {'Epos': -1}, {'Epos': 1 << 31}, {'graph_ptr': None}, {'pos_in_src': None},
           {'pos_in_dst': None}]
    sizes = [{'N': 1}, {'N': 0}, {'N': 1 << 31}, {'E': -1, 'R': 0}, {'E': 1 << 28}, {'pos_out_ptr': None}]
    for over in own + sizes + [{'neg_src': None}, {'neg_dst': None}]:
        assert _call('mgv_neg_draw_local', draw, over) == EINVAL, over
    for over in own + sizes + [{'ws_ints': n_ws - 1}, {'ws_ints': 0}, {'ws': ctypes.c_void_p(64 * 11 + 4)}] + [
            {k: None} for k in ('edge_index', 'out_ptr', 'out_dst', 'in_ptr', 'in_src', 'ws')]:
        assert _call('mgv_neg_partition_local', part, over) == EINVAL, over
    for shift in (-1, 13):
        assert _call('mgv_neg_partition_local', part, {'shift': shift}) == EUNSUPPORTED
    assert _call('mgv_neg_partition_local', part, {'N': (2048 << 12) + 1, 'ws_ints': 1 << 30, 'shift': 12}) == EUNSUPPORTED
    # its own checks come first: a bad G is MGV_EINVAL where the shift alone would be MGV_EUNSUPPORTED
    assert _call('mgv_neg_partition_local', part, {'G': 0, 'shift': 13}) == EINVAL
    # R = 0 needs no in-lists, and an empty draw nothing to write to: MGV_OK before any launch
    assert _call('mgv_neg_draw_local', draw, {'E': 0, 'R': 0, 'Epos': 0, 'pos_in_src': None, 'pos_in_dst': None, 'neg_src': None, 'neg_dst': None}) == OK
