"""CPU checks behind tests/test_hip_dense_reference.py: the float64 restatements of tests/dense_ref.py are pinned to independent
formulations (torch.nn.functional.linear under autograd, the per-slot index_add form of tests/test_rounds.py, ops.split_bf16 /
ops.frag_order, torch.index_add), the case builders are shown to sit where the device tests need them (each side of every grid cap,
two and three tiles per workgroup, every regime of k_slab_sum, the list lengths around the loads in flight, both class-count paths,
a positive scale wherever a comparison divides by one), and every defect of the kinds the device tests are there to catch is shown
to land at least 10x outside the bound the device test uses for that output when planted in the restatement."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as DR  # noqa: E402

F64, F32 = torch.float64, torch.float32
v = lambda o: None if o is None else o.v       # noqa: E731


# ------------------------------------------------------------------------------------------------ pinning
@pytest.mark.parametrize('K1,bias,res,strided', [(None, True, False, False), (16, True, True, True), (4, False, True, False), (60, True, False, True)])
def test_linear_is_torch_linear_under_autograd(K1, bias, res, strided):
    M, K, N = 32, 64, 129
    c = DR.linear_case(M, K, N, K1=K1, strided=strided, bias=bias, res=res)
    r = DR.linear_ref(c)
    d = lambda t: None if t is None else t.to(F64)       # noqa: E731
    X = torch.cat([d(c['X1'].v)] + ([d(c['X2'].v)] if c['X2'] is not None else []), 1).requires_grad_(True)
    W = d(c['W']).requires_grad_(True)
    b = d(c['b']).requires_grad_(True) if bias else None
    Y = torch.nn.functional.linear(X, W, b)
    (Y * d(c['dY'].v)).sum().backward()
    want = {'Y': Y.detach() + (d(c['R'].v) if res else 0), 'dX': X.grad, 'dW': W.grad}
    if bias:
        want['db'] = b.grad
    else:
        assert float((r['db'] - d(c['dY'].v).sum(0)).abs().max()) == 0
    for k, w in want.items():
        q = DR.ratio(r[k], w, r['S'][k])
        assert q <= 1e-13, (k, q)
    assert all(bool((S > 0).all()) for S in r['S'].values())
    if strided:
        assert all(bool(torch.isnan(c[k].parent[:, :4]).all()) and bool(torch.isnan(c[k].parent[:, -4:]).all()) and c[k].ld == c[k].w + 8
                   for k in ('X1', 'dY') + (('X2',) if c['X2'] is not None else ()) + (('R',) if res else ()))


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('ghs', [False, True])
@pytest.mark.parametrize('bias', [False, True])
def test_pair_is_two_torch_linears_under_autograd(bias, ghs, strided):
    """dense_ref.pair in float64: hs = linear([s | t]), st = linear(hs), the loss <st, dST> + <hs, gHS>; also 'ST_given' and the
    backward's weight gradient of an HS handed in (the pair's backward takes hs as an input of its own)."""
    c = DR.pair_case(129, strided=strided, bias=bias, ghs=ghs)
    r = DR.pair_ref(c)
    d = lambda t: None if t is None else t.to(F64).requires_grad_(True)       # noqa: E731
    S, T, Wl, bl, Wd, bd = (d(t) for t in (c['S'].v, c['T'].v, c['Wl'], c['bl'], c['Wd'], c['bd']))
    hs = torch.nn.functional.linear(torch.cat([S, T], 1), Wl, bl)
    hs.retain_grad()
    st = torch.nn.functional.linear(hs, Wd, bd)
    loss = (st * c['dST'].v.to(F64)).sum()
    if ghs:
        loss = loss + (hs * c['gHS'].v.to(F64)).sum()
    loss.backward()
    want = {'HS': hs.detach(), 'ST': st.detach(), 'dhs': hs.grad, 'dS': S.grad, 'dT': T.grad, 'dWl': Wl.grad, 'dWd': Wd.grad}
    if bias:
        want.update(dbl=bl.grad, dbd=bd.grad)
    else:
        assert float((r['dbl'] - hs.grad.sum(0)).abs().max()) <= 1e-13 * float(r['S']['dbl'].max())
        assert float((r['dbd'] - c['dST'].v.to(F64).sum(0)).abs().max()) == 0
    for k, w in want.items():
        q = DR.ratio(r[k], w, r['S'][k])
        assert q <= 1e-13, (k, q)
    assert set(r['S']) == set(want) | {'dbl', 'dbd'} and all(bool((s > 0).all()) for s in r['S'].values())
    # an HS handed in: a perturbed copy, so that it is told apart from the run's own
    given = (hs.detach() * 1.25).to(F32).to(F64)
    rg = DR.pair_ref(c, given)
    assert DR.ratio(rg['ST_given'], torch.nn.functional.linear(given, Wd.detach(), None if bd is None else bd.detach()), rg['S']['ST_given']) <= 1e-13
    assert DR.ratio(rg['dWd'], c['dST'].v.to(F64).t() @ given, rg['S']['dWd']) <= 1e-13
    assert all(torch.equal(rg[k], r[k]) for k in ('HS', 'ST', 'dhs', 'dS', 'dT', 'dWl', 'dbl', 'dbd'))
    if strided:
        ops_ = ('S', 'T', 'dST') + (('gHS',) if ghs else ())
        assert all(bool(torch.isnan(c[k].parent[:, :4]).all()) and bool(torch.isnan(c[k].parent[:, -4:]).all()) and c[k].ld == c[k].w + 8 for k in ops_)


def test_pair_case_is_built_as_designed():
    c = DR.pair_case(129)
    for k, w in (('S', 64), ('T', 64), ('dST', 128), ('gHS', 64)):
        m = c[k].v.abs().amax(1)
        assert c[k].v.shape == (129, w) and float(m.max() / m.min()) > 1e4 and float(m[-1]) > 1e3      # a power of ten per row, the last row on top
    assert c['Wl'].shape == (64, 128) and c['Wd'].shape == (128, 64) and c['bl'].shape == (64,) and c['bd'].shape == (128,)
    q = DR.pair_case(129, coherent=True)
    assert all(float(q[k].v.min()) >= 0 for k in ('S', 'T', 'dST', 'gHS'))
    for W in (q['Wl'], q['Wd']):
        hi = W.to(torch.bfloat16).to(F32)
        assert bool((torch.log2(hi) % 1 == 0).all()) and torch.equal((W - hi), hi * 2.0 ** -9)


@pytest.mark.parametrize('M,K', DR.GROUPED_FWD)
@pytest.mark.parametrize('subset', [False, True])
def test_grouped_is_the_per_slot_index_add_form(M, K, subset):
    """tests/test_rounds.py's formulation: a slot per node (255: no tile names it), ref.index_add over the nodes of each slot, autograd
    for the gradients; the weight gradient of the restatement takes ONE slot's tile list, as the entry does."""
    c = DR.grouped_case(M, K, subset=subset, res=True)
    tb = c['tables']
    r = DR.grouped_ref(c)
    order, ts, tc, tslot = (tb[k].long() for k in ('order', 'tile_start', 'tile_count', 'tile_slot'))
    listed = tb['tile_list'].long().tolist() if subset else list(range(ts.numel()))
    slot = torch.full((c['Nn'],), 255)
    for t in listed:
        slot[order[ts[t]:ts[t] + tc[t]]] = tslot[t]
    X, W, b = (t.to(F64).requires_grad_(True) for t in (c['X'].v, c['W'], c['b']))
    ref = torch.zeros(c['Nn'], M, dtype=F64)
    for s in range(c['T']):
        idx = torch.nonzero(slot == s).reshape(-1)
        ref = ref.index_add(0, idx, X[idx] @ W[s].t() + b[s] + c['R'].v.to(F64)[idx])
    (ref * c['dY'].v.to(F64)).sum().backward()
    assert torch.equal(r['named'], slot != 255) and 0 < int(r['named'].sum()) < c['Nn']
    assert DR.ratio(r['Y'], ref.detach(), r['S']['Y'].clamp(min=1e-300)) <= 1e-13
    assert float(r['Y'][~r['named']].abs().max()) == 0 and bool((r['S']['Y'][r['named']] > 0).all())
    for s in range(c['T']):
        one = dict(tb, tile_list=torch.tensor([t for t in listed if int(tslot[t]) == s], dtype=torch.int32))
        g = DR.grouped(c['X'].v, None, None, None, one, c['dY'].v)
        assert DR.ratio(g['dW'], W.grad[s], g['S']['dW']) <= 1e-13 and DR.ratio(g['db'], b.grad[s], g['S']['db']) <= 1e-13


def test_grouped_tables_are_designed():
    """Tile counts {0, 1, 63, 64}; tile_start is not the running sum of the counts; order is a non-monotone permutation that leaves
    nodes out; slots out of order; per-slot biases 10 apart (the forward's bound is ~1e-4 of scale); the subset is strict, shuffled and
    keeps a zero-count tile."""
    c = DR.grouped_case(192, 64, subset=True)
    tb = {k: (None if t is None else t.long()) for k, t in c['tables'].items()}
    assert {0, 1, 63, 64} <= set(tb['tile_count'].tolist())
    assert tb['tile_start'].tolist() != (torch.cumsum(tb['tile_count'], 0) - tb['tile_count']).tolist()
    nodes, slots = DR.tile_nodes(dict(c['tables'], tile_list=None))
    assert nodes.unique().numel() == nodes.numel() < c['Nn'] and bool((nodes[1:] < nodes[:-1]).any()) and bool((nodes[1:] > nodes[:-1]).any())
    s = tb['tile_slot'].tolist()
    assert s != sorted(s) and set(s) == set(range(c['T']))
    assert float((c['b'][1] - c['b'][0]).abs().min()) > 5 and float((c['W'][2].abs().mean() / c['W'][0].abs().mean())) > 2
    tl = tb['tile_list'].tolist()
    assert 0 < len(tl) < tb['tile_count'].numel() and tl != sorted(tl) and len(set(tl)) == len(tl) and any(tb['tile_count'][t] == 0 for t in tl)


@pytest.mark.parametrize('transpose', [0, 1])
def test_wpack_is_split_bf16_in_frag_order(transpose):
    from deepgate import ops
    torch.manual_seed(transpose)
    W = torch.randn(192, 64) * 10.0 ** torch.empty(192, 1).uniform_(-3, 3)
    A = W.t().contiguous() if transpose else W
    hi, lo = ops.split_bf16(A)
    mine = DR.wpack(W, transpose)
    assert torch.equal(mine[0], ops.frag_order(hi).contiguous().view(torch.int16)) and torch.equal(mine[1], ops.frag_order(lo).contiguous().view(torch.int16))
    # fragment order, stated once more from the kernel's index arithmetic (linear_x3.hip k_wpack_bf16x3)
    R, K = A.shape
    o = torch.arange(R * K)
    blk, lane, e = o >> 9, (o & 511) >> 3, o & 7
    row, k = (blk // (K // 32)) * 16 + (lane & 15), (blk % (K // 32)) * 32 + (lane >> 4) * 8 + e
    assert torch.equal(mine[0], hi[row, k].view(torch.int16))
    back = mine[0].view(torch.bfloat16).to(F64) + mine[1].view(torch.bfloat16).to(F64)
    assert float(((back - A[row, k].to(F64)).abs() / A[row, k].abs().to(F64)).max()) <= 2.0 ** -16


def test_row_sums_are_index_add():
    c = DR.list_case(32, 129)
    r = DR.gather_sum(c['h'], c['ptr'], c['idx'])
    ptr = c['ptr'].long()
    deg = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(c['N']), deg)
    want = torch.zeros(c['N'], 32, dtype=F64).index_add_(0, rows, c['h'].to(F64)[c['idx'].long()[:int(ptr[-1])]])
    assert DR.ratio(r['agg'], want, r['S']['agg'].clamp(min=1e-300)) <= 1e-13 and torch.equal(r['deg'], deg.to(F64))
    for items, agg, out_row in ((True, True, True), (False, True, False), (True, False, False), (False, False, True)):
        s = DR.seg_case(32, 70, items, agg, out_row)
        r = DR.seg_ref(s)
        total = int(s['seg_ptr'][-1])
        member = s['items'].long()[:total] if items else torch.arange(total)
        val = s['direct'].to(F64)
        if agg:
            np_ = s['nbr_ptr'].long()
            nrow = torch.repeat_interleave(torch.arange(np_.numel() - 1), np_[1:] - np_[:-1])
            val = val.clone().index_add_(0, nrow, s['agg'].to(F64)[s['nbr_idx'].long()[:int(np_[-1])]])
        sp = s['seg_ptr'].long()
        seg = torch.repeat_interleave(torch.arange(70), sp[1:] - sp[:-1])
        want = torch.zeros(70, 32, dtype=F64).index_add_(0, seg, val[member])
        assert DR.ratio(r['out'], want, r['S']['out'].clamp(min=1e-300)) <= 1e-13
        assert r['rows'].unique().numel() == 70 and int(r['rows'].max()) < s['n_out'] and (out_row or torch.equal(r['rows'], torch.arange(70)))
    for C in (1, 8, 9, 40):
        q = DR.class_case(16, 300, C)
        r = DR.class_ref(q)
        np_ = q['ptr'].long()
        nrow = torch.repeat_interleave(torch.arange(300), np_[1:] - np_[:-1])
        val = q['gy_direct'].to(F64).clone().index_add_(0, nrow, q['gy_agg'].to(F64)[q['idx'].long()[:int(np_[-1])]])
        want = torch.zeros(C, 16, dtype=F64).index_add_(0, q['class_id'].long(), val)
        assert DR.ratio(r['out'], want, r['S']['out'].clamp(min=1e-300)) <= 1e-13
        present = torch.bincount(q['class_id'].long(), minlength=C) > 0
        assert bool((r['S']['out'][present] > 0).all()) and bool((r['S']['out'][~present] == 0).all()) and (C <= 2 or not present[q['absent']])
        assert torch.equal(DR.class_expand(q['table'], q['class_id']), torch.stack([q['table'][int(k)] for k in q['class_id']]))


def test_float32_list_order_is_the_order_of_a_plain_loop():
    """The float32 restatements of gather_sum and seg_sum, which the device must match bit for bit, against scalar loops written
    straight from the kernel comments (list order; own row, then neighbours, then into the segment's sum)."""
    c = DR.list_case(16, 65)
    r = DR.gather_sum(c['h'], c['ptr'], c['idx'], F32)['agg'].to(F32)
    for n in range(65):
        acc = torch.zeros(16)
        for e in range(int(c['ptr'][n]), int(c['ptr'][n + 1])):
            acc = acc + c['h'][int(c['idx'][e])]
        assert torch.equal(acc, r[n]), n
    s = DR.seg_case(16, 9)
    r = DR.seg_ref(s, F32)['out'].to(F32)
    for k in range(9):
        acc = torch.zeros(16)
        for m in range(int(s['seg_ptr'][k]), int(s['seg_ptr'][k + 1])):
            row = int(s['items'][m])
            val = s['direct'][row].clone()
            for e in range(int(s['nbr_ptr'][row]), int(s['nbr_ptr'][row + 1])):
                val = val + s['agg'][int(s['nbr_idx'][e])]
            acc = acc + val
        assert torch.equal(acc, r[k]), k


# ------------------------------------------------------------------------------------------------ designed sizes
LARGE = [('linear_fwd', (64, 64)), ('linear_wgrad', (64, 64)), ('linear_fwd_x3', (64, 128)), ('linear_wgrad_x3', (64, 128)), ('linear_wgrad_x3', (32, 32)),
         ('linear_pair_fwd_x3', DR.PAIR), ('linear_pair_bwd_x3', DR.PAIR)]


def test_workgroups_per_cu_as_the_launchers_compute_them():
    for k in ('linear_pair_fwd_x3', 'linear_pair_bwd_x3'):
        assert DR.per_cu(k, DR.PAIR) == 2 and DR.unit_rows(k, DR.PAIR) == 64 and DR.cap_rows(k, DR.PAIR) == 32768 and DR.large_rows(k, DR.PAIR) == 65875
    assert DR.per_cu('linear_pair_bwd_x3', DR.PAIR) == DR.per_cu('linear_wgrad_x3', (64, 128))      # "the grid of hs_linear's backward"
    assert [DR.per_cu('linear_fwd_x3', s) for s in DR.X3_SHAPES] == [3, 3, 4, 4, 4, 4]
    assert [DR.per_cu('linear_wgrad_x3', s) for s in DR.X3_SHAPES] == [2, 2, 2, 2, 2, 4]
    assert DR.per_cu('linear_fwd', (64, 64)) == 8 and DR.per_cu('linear_wgrad', (64, 64)) == 2
    assert [DR.unit_rows('gather_sum', H) for H in DR.WIDTHS] == [64, 32, 16, 8]
    # the workspace query sizes for 4 workgroups per CU, the launch never takes more
    assert all(DR.per_cu('linear_wgrad_x3', s) <= 4 for s in DR.X3_WGRAD_WAVES)


@pytest.mark.parametrize('kernel,shape', LARGE)
def test_designed_rows_sit_where_they_claim(kernel, shape):
    cap = DR.cap_rows(kernel, shape)
    assert max(DR.visits(kernel, shape, cap)) == 1 and len(DR.visits(kernel, shape, cap)) == DR.GRID_CAP * DR.per_cu(kernel, shape)
    two = DR.visits(kernel, shape, cap + 1)
    assert two[0] == 2 and set(two[1:]) == {1}
    big = DR.large_rows(kernel, shape)
    vis = DR.visits(kernel, shape, big)
    assert vis[:6] == [3] * 6 and set(vis[6:]) == {2} and big % DR.TILE == 19
    assert all(max(DR.visits(kernel, shape, n)) == 1 for n in DR.SMALL_ROWS)
    assert big <= 300000 and big * max(shape) * 4 <= 160e6


def test_slab_regimes_are_all_hit():
    reg = {t: DR.slab_regime(t) for t in DR.SLAB_TILES}
    assert [reg[t] for t in DR.SLAB_TILES] == ['short', 'short', 'short', 'phases', 'phases', 'mixed', 'unrolled', 'unrolled+tail', 'unrolled+tail']
    assert DR.slab_passes(127)[15] == (0, 7) and DR.slab_passes(127)[14] == (1, 0) and DR.slab_passes(128) == [(1, 0)] * 16
    assert DR.slab_passes(147)[:3] == [(1, 2), (1, 2), (1, 2)] and DR.slab_passes(147)[3] == (1, 1) and DR.slab_passes(17)[0] == (0, 2)
    for shape in ((64, 128), (32, 32)):
        for t in DR.SLAB_TILES:       # below the cap the grid, and with it the slab, has one row per tile
            assert DR.grid('linear_wgrad_x3', shape, DR.slab_rows(t)) == t and DR.slab_rows(t) % DR.TILE == 5
    # mgv_class_pull_sum's slab: one row per workgroup; past the cap 2048 rows, sixteen unrolled passes per phase and no tail
    assert DR.slab_passes(DR.grid('class_pull_sum', 128, DR.pull_sizes(128)[3]))[0] == (16, 0)


@pytest.mark.parametrize('H', DR.WIDTHS)
def test_lists_hold_the_designed_lengths(H):
    c = DR.list_case(H, 129)
    deg = (c['ptr'][1:] - c['ptr'][:-1]).tolist()
    assert set(DR.DEGREES) | {DR.HUB} <= set(deg) and int(c['idx'].max()) >= 129
    s = DR.seg_case(H, 129)
    assert set(DR.SEG_LENS) | {DR.HUB} <= set((s['seg_ptr'][1:] - s['seg_ptr'][:-1]).tolist())
    assert set(DR.DEGREES) | {DR.HUB} <= set((s['nbr_ptr'][1:] - s['nbr_ptr'][:-1]).tolist())
    untouched = set(range(s['n_out'])) - set(s['out_row'].tolist())
    assert len(untouched) == 7
    for kernel in ('gather_sum', 'seg_sum', 'class_expand'):
        past = DR.cap_rows(kernel, H) + 77
        assert max(DR.visits(kernel, H, past)) == 2 and max(DR.visits(kernel, H, DR.cap_rows(kernel, H))) == 1
    stride = DR.cap_rows('class_pull_sum', H)
    for u, n in zip((1, 2, 3, 4), DR.pull_sizes(H)):
        assert DR.grid('class_pull_sum', H, n) * DR.unit_rows('class_pull_sum', H) == stride
        assert u * stride < n < u * stride + stride // 2          # some lane groups have a u-th row, most have not
    big = DR.list_case(H, DR.FEW + 100)
    assert int(big['ptr'][-1]) < 25 * DR.FEW


def test_both_class_count_paths():
    """dense.hip mgv_class_pull_sum (launch_class_pull_sum<H, 8> / <H, 0>): register sums up to 8 classes, LDS atomics above; the cases hold every class but the absent one."""
    for C in (8, 9, 40):
        q = DR.class_case(64, 1000, C)
        assert set(q['class_id'].tolist()) == set(range(C)) - {q['absent']} and 40 * 128 * 20 <= 160 * 1024


# ------------------------------------------------------------------------------------------------ planted defects
@functools.lru_cache(maxsize=None)
def _lin(mm, M, K, N, K1=None, res=False, coherent=False):
    c = DR.linear_case(M, K, N, K1=K1, res=res, coherent=coherent)
    r64 = DR.linear_ref(c)
    tau = DR.taus(r64, DR.linear_ref(c, F32, 'x3' if mm == 'x3' else 'exact'), mm)
    if mm == 'f32':             # the fp32 weight gradient's dW: the derived bound of the device test (dense_ref.chain_length)
        tau['dW'] = DR.device_bound('linear_wgrad', 'dW', (M, K), N, tau['dW'])
    return c, r64, tau


def _worst(got, r64, tau, only=None):
    ex = {k: q / tau[k] for k, q in DR.ratios(got, r64).items() if only is None or k in only}
    k = max(ex, key=ex.get)
    return k, ex[k]


def _lin_defect(mm, mutate, only, **kw):
    c, r64, tau = _lin(mm, **kw)
    return _worst(DR.linear_ref(c, F32, 'x3' if mm == 'x3' else 'exact', mutate), r64, tau, only)


X3_CAP = DR.cap_rows('linear_fwd_x3', (64, 128))


def _defects():
    both = ('f32', 'x3')
    out = []
    for mm in both:
        out += [('a partial tile\'s last row dropped (forward) [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('drop_last_row',), ('Y',), M=64, K=64, N=65)),
                ('a partial tile\'s last row dropped (gradients) [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('drop_last_row',), ('dW', 'db'), M=64, K=64, N=65)),
                ('a partial tile\'s last row dropped (dW alone) [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('drop_last_row',), ('dW',), M=64, K=64, N=65)),
                ('the X1 | X2 seam off by four columns [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('seam',), ('Y',), M=64, K=64, N=129, K1=32)),
                ('the X1 | X2 seam off by four columns (weight gradient) [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('seam',), ('dW',), M=64, K=64, N=129, K1=60)),
                ('the residual not added [%s]' % mm, lambda mm=mm: _lin_defect(mm, ('no_residual',), ('Y',), M=64, K=64, N=65, res=True))]
    # with random signs the hi.lo products largely cancel and the defect sits near the bound itself (dense_ref.linear_case): the
    # coherent case, which the device test runs as well, makes them add up
    out += [('the hi.lo term dropped (forward, coherent inputs) [x3]', lambda: _lin_defect('x3', ('drop_hilo',), ('Y', 'dX'), M=64, K=128, N=65, coherent=True)),
            ('the hi.lo term dropped (weight gradient, coherent inputs) [x3]', lambda: _lin_defect('x3', ('drop_hilo',), ('dW',), M=64, K=128, N=65, coherent=True)),
            ('slab rows from 128 on not added [x3]', lambda: _lin_defect('x3', ('slab_from_128',), ('dW',), M=32, K=32, N=DR.slab_rows(147))),
            ('db missing the second load phase [x3]', lambda: _lin_defect('x3', ('db_second_phase', 32), ('db',), M=64, K=128, N=129)),
            ('the second tile of a workgroup computed from the first tile\'s prefetch [x3]',
             lambda: _lin_defect('x3', ('stale_prefetch', X3_CAP // DR.TILE), ('Y',), M=64, K=128, N=X3_CAP + 1))]

    def grp(mutate, only, subset=True):
        c = DR.grouped_case(192, 64, subset=subset, res=True)
        r64 = DR.grouped_ref(c, wgrad=True)
        tau = DR.taus(r64, DR.grouped_ref(c, F32, 'x3', wgrad=True), 'x3')
        return _worst(DR.grouped_ref(c, F32, 'x3', mutate, wgrad=True), r64, tau, only)
    out += [('the bias of slot 0 used for every tile [x3]', lambda: grp(('bias_slot0',), ('Y',))),
            ('a node outside tile_list written [x3]', lambda: grp(('write_outside_list',), ('Y',)))]      # (S = 0 there: any value but the reference's 0 is infinitely far)

    def rows(build, ref, mutate):
        c = build()
        r64 = ref(c, F64, None)
        tau = DR.taus(r64, ref(c, F32, None), 'f32')
        return _worst(ref(c, F32, mutate), r64, tau)
    g_ref = lambda c, dt, mu: DR.gather_sum(c['h'], c['ptr'], c['idx'], dt, mu)       # noqa: E731
    s128 = DR.cap_rows('class_pull_sum', 128)
    out += [('the third neighbour lost (gather)', lambda: rows(lambda: DR.list_case(64, 129), g_ref, ('drop_pos', 2))),
            ('the third neighbour lost (segment members)', lambda: rows(lambda: DR.seg_case(64, 129), DR.seg_ref, ('drop_pos', 2))),
            ('the third neighbour lost (class sums)', lambda: rows(lambda: DR.class_case(64, 129, 8), DR.class_ref, ('drop_pos', 2))),
            ('the second in-flight segment member lost', lambda: rows(lambda: DR.seg_case(64, 129), DR.seg_ref, ('drop_member', 1))),
            ('class 8 folded into class 0', lambda: rows(lambda: DR.class_case(64, 1000, 9), DR.class_ref, ('fold_class', 8, 0))),
            ('the row u = 3 past the stride lost', lambda: rows(lambda: DR.class_case(128, DR.pull_sizes(128)[2], 40), DR.class_ref, ('lost_u', 3, s128)))]
    out += _pair_defects()
    return out


PAIR_CAP = DR.cap_rows('linear_pair_bwd_x3', DR.PAIR)
PAIR_BIG = DR.large_rows('linear_pair_bwd_x3', DR.PAIR)


@functools.lru_cache(maxsize=None)
def _pair(N, coherent=False):
    c = DR.pair_case(N, coherent=coherent)
    r64, rx3, tau = DR.pair_runs(c)
    return c, r64, rx3, tau


def _pair_defect(mutate, only, N, coherent=False):
    """The defect in the bf16x3 run, with the given HS of the bound's own runs: the worst of the outputs `only` over its bound."""
    c, r64, rx3, tau = _pair(N, coherent)
    return _worst(DR.pair_ref(c, rx3['HS'], F32, 'x3', mutate), r64, tau, only)


def _pair_defects():
    out = []
    for N in (PAIR_CAP + 1, PAIR_BIG):
        g = DR.grid('linear_pair_bwd_x3', DR.PAIR, N)
        assert g == DR.grid('linear_pair_fwd_x3', DR.PAIR, N) == 512
        at = ' [pair, N=%d]' % N
        out += [('the second tile of a workgroup from its first tile\'s S | T (forward)' + at, lambda N=N, g=g: _pair_defect(('stale_fwd', g), ('HS', 'ST'), N)),
                ('the second tile of a workgroup from its first tile\'s dST / HS (backward)' + at, lambda N=N, g=g: _pair_defect(('stale_bwd_gh', g), ('dS', 'dT', 'dWd', 'dbd'), N)),
                ('the second tile of a workgroup from its first tile\'s S | T (backward)' + at, lambda N=N, g=g: _pair_defect(('stale_bwd_x', g), ('dWl',), N)),
                ('the second tile of a workgroup from its first tile\'s gHS alone (backward)' + at, lambda N=N, g=g: _pair_defect(('stale_bwd_ghs', g), ('dS', 'dT', 'dWl', 'dbl'), N))]
        out += [('a workgroup\'s %s kept from its last visited tile only' % k + at, lambda N=N, g=g, k=k: _pair_defect(('last_visit', k, g), (k,), N))
                for k in ('dWd', 'dWl', 'dbl', 'dbd')]
    out += [('gHS not added to dhs [pair]', lambda: _pair_defect(('no_ghs',), ('dS', 'dT', 'dWl', 'dbl'), 129)),
            ('dbl summed without gHS [pair]', lambda: _pair_defect(('dbl_no_ghs',), ('dbl',), 129)),
            ('ST formed from the unbiased hs [pair]', lambda: _pair_defect(('st_unbiased',), ('ST', 'ST_given'), 129)),
            ('a partial tile\'s last row dropped (forward) [pair]', lambda: _pair_defect(('drop_last_row',), ('HS', 'ST', 'ST_given'), 65)),
            ('a partial tile\'s last row dropped (gradients) [pair]', lambda: _pair_defect(('drop_last_row',), ('dWl', 'dbl', 'dWd', 'dbd'), 65)),
            ('the hi.lo term dropped from dST Wd (coherent inputs) [pair]', lambda: _pair_defect(('drop_hilo_dhs',), ('dS', 'dT', 'dWl', 'dbl'), 65, True)),
            ('rows 32 to 63 of each tile missing from dbd [pair]', lambda: _pair_defect(('dbd_half',), ('dbd',), 129))]
    return out


DEFECTS = _defects()


@pytest.mark.parametrize('what,run', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_far_outside_the_device_bound(what, run):
    """Each defect, planted in the float32 / bf16x3 restatement, exceeds the bound the device test uses for that output on the same case
    (tau S, tau = 8 max(r, floor) per output; max(tau, L 2^-24) S for dW of the fp32 weight gradient) by at least 10x on an output the
    defect belongs to."""
    k, ex = run()
    print('%s: %.3g x the bound on %s' % (what, ex, k))
    assert ex >= 10


# ------------------------------------------------------------------------------------------------ host size query
def test_workspace_query_knows_the_supported_widths():
    """mgv_class_pull_sum_ws_floats through the built library (a pure host computation, no device and no pointers): 0 for every width
    the row-sum kernels do not take (H < 4 used to divide by zero there: kThreads / (H / 4) before H was looked at), one row of C H
    floats per workgroup otherwise.  The refusals of the launch entries are asserted on the device, with device buffers large enough
    for the call: tests/test_hip_dense_reference.py test_refusals_are_return_codes."""
    from deepgate import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load()
    for H in (0, 2, 8, 48, 256, -16, 3):
        assert lib.mgv_class_pull_sum_ws_floats(H, 5, 4) == 0
    for H in DR.WIDTHS:
        assert lib.mgv_class_pull_sum_ws_floats(H, 5, 4) == 4 * H and lib.mgv_class_pull_sum_ws_floats(H, 0, 4) == 0
        assert lib.mgv_class_pull_sum_ws_floats(H, DR.pull_sizes(H)[3], 4) == DR.GRID_CAP * 8 * 4 * H


def _lib():
    from deepgate import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


def test_pair_workspace_query_is_one_slab_row_pair_per_workgroup():
    """mgv_linear_pair_bwd_x3_ws_floats: per workgroup one row of (dWl, dbl) and one of (dWd, dbd) partials; never negative."""
    lib = _lib()
    assert DR.PAIR_SLAB == 64 * 128 + 64 + 128 * 64 + 128
    for N in DR.SMALL_ROWS + (PAIR_CAP, PAIR_CAP + 1, PAIR_BIG, 1 << 22):
        assert lib.mgv_linear_pair_bwd_x3_ws_floats(N) == DR.grid('linear_pair_bwd_x3', DR.PAIR, N) * DR.PAIR_SLAB, N
    assert lib.mgv_linear_pair_bwd_x3_ws_floats(PAIR_CAP + 1) == 512 * DR.PAIR_SLAB
    for N in (0, -1, -(1 << 40)):
        assert lib.mgv_linear_pair_bwd_x3_ws_floats(N) >= 0, N


def _pair_call(lib, name, N=65, **over):
    """The entry with arguments that pass every check (dummy non-NULL pointers, never dereferenced on the host: a refused call
    returns before anything is launched; an accepted one is made with N = 0 only, which returns before the launch too)."""
    import ctypes
    import re
    from deepgate import _hip
    with open(_hip.HEADER_PATH) as f:
        text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S))
    decl = re.search(r'\bint\s+%s\s*\(([^;{]*?)\)\s*;' % name, text, flags=re.S).group(1)
    names = [re.findall(r'\w+', a)[-1] for a in decl.split(',')]
    wide = {'lddst': 136, 'ldst': 136}
    args = []
    for k, (n, t) in enumerate(zip(names, _hip.parse_header()[name])):
        if n in over:
            v = over[n]
            args.append(v if t is not ctypes.c_void_p or v is None else ctypes.c_void_p(v))
        elif n == 'stream':
            args.append(None)
        elif t is ctypes.c_void_p:
            args.append(ctypes.c_void_p(64 * (k + 1)))
        else:
            args.append(N if n == 'N' else 1 << 30 if n == 'workspace_floats' else wide.get(n, 72))
    assert set(over) <= set(names), (name, over)
    return getattr(lib, name)(*args)


@pytest.mark.parametrize('name,arg,value', DR.PAIR_REFUSALS, ids=['%s-%s-%s' % r for r in DR.PAIR_REFUSALS])
def test_pair_entries_refuse_every_clause_of_their_argument_checks(name, arg, value):
    """MGV_EINVAL for a NULL required pointer, a row stride narrower than its matrix or no multiple of 4 (float4 rows), N < 0: every
    clause of the MGV_CHECK_ARG lines of mgv_linear_pair_fwd_x3 / _bwd_x3, before N = 0 is looked at and before any launch (so
    nothing is written; the device test repeats the table over real buffers and looks)."""
    lib = _lib()
    assert _pair_call(lib, name, 0) == 0                      # the base call is valid: N = 0 is MGV_OK
    assert _pair_call(lib, name, **{arg: value}) == -1
    if arg != 'N':
        assert _pair_call(lib, name, 0, **{arg: value}) == -1


def test_pair_backward_looks_at_ldghs_only_where_ghs_is_given():
    lib = _lib()
    for ld in DR.PAIR_GHS_NULL_ACCEPTS:
        assert _pair_call(lib, 'mgv_linear_pair_bwd_x3', 0, gHS=None, ldghs=ld) == 0
    for k in ('bl', 'bd'):
        assert _pair_call(lib, 'mgv_linear_pair_fwd_x3', 0, **{k: None}) == 0
    for k in ('dbl', 'dbd'):
        assert _pair_call(lib, 'mgv_linear_pair_bwd_x3', 0, **{k: None}) == 0
