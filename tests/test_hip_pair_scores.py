"""The all-pairs decoder entries of csrc/pair_scores.hip — mgv_pair_scores_fwd, mgv_pair_scores_bwd, mgv_pair_scores_at, mgv_pair_topk —
through the C ABI and then through the surface (ops.pair_scores / pair_scores_at / pair_topk / reconstruction_counts,
DirectedInnerProductDecoder.forward_all / topk, DirectedGAE.forward, Model.predict_links / reconstruction_counts), against the float64
restatements of tests/pair_scores_ref.py (pinned on the CPU by tests/test_pair_scores_spec.py, which also asserts the properties of the
case builders used here and shows that the defects these tests are there to catch are far outside their bounds).

Bounds, entry by entry, derived (pair_scores_ref's docstring; nothing is taken from what the device returns):
  raw   H 2^-24 S                       p   dq = 4 2^-24 + p (1 - p) H 2^-24 S
  ds    max(H, L) 2^-24 sum_j |g| p (1 - p) |t| + sum_j |g| dq |t|,   L = pair_scores_ref.chain_length(N)        (dt alike, L from M)
Exact, bit for bit: pair_scores_at against the dense entry, the scores of pair_topk against the dense entries its indices name, n_above
against the dense rows, repeated backward runs, guard rows and foreign columns (NaN before the call).  Counts against float64 lie
between the float64 counts at threshold -/+ bound.

Operands are column slices of wider matrices whose foreign columns hold NaN; every output has 64 NaN guard rows behind it.
Every check prints one line `PS <entry> <case> | worst error / bound`."""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()
SIZES = (1, 15, 16, 17, 30, 63, 64, 65, 129, 257)
HS = (16, 32, 64, 128)
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _hip():
    from deepgate import _hip
    return _hip


def _rc(name, *args):
    """The launcher's return code itself (the refusals are return codes)."""
    h = _hip()
    return int(getattr(h.load(), name)(*args, h.stream()))


def _call(name, *args):
    rc = _rc(name, *args)
    assert rc == 0, '%s returned %d' % (name, rc)


def _ptr(t):
    return _hip().ptr(t)


def _slice(x, dev):
    """x [n, H] as columns 4 .. 4 + H of a matrix 8 wider whose other columns hold NaN -> (view, row stride)."""
    n, H = x.shape
    parent = torch.full((max(n, 1), H + 8), NAN, dtype=F32, device=dev)
    v = parent[:n, 4:4 + H]
    v.copy_(x)
    return v, H + 8


class Out:
    """An [n][w] float output with GUARD rows behind it; strided: columns 3 .. 3 + w of a matrix 5 wider.  NaN everywhere before the call."""

    def __init__(self, n, w, dev, strided=False, dtype=F32):
        self.n, self.w, self.off = n, w, 3 if strided else 0
        fill = NAN if dtype == F32 else -77
        self.fill = fill
        self.parent = torch.full((n + GUARD, max(w + (5 if strided else 0), 1)), fill, dtype=dtype, device=dev)
        self.v = self.parent[:n, self.off:self.off + w]
        self.ld = self.parent.shape[1]

    def intact(self, rows_written=None):
        """Guard rows and foreign columns bit-identical to their fill."""
        p = self.parent
        bits = p.view(I32) if p.dtype == F32 else p
        want = NANBITS if p.dtype == F32 else self.fill
        mine = torch.zeros(p.shape, dtype=torch.bool, device=p.device)
        mine[:self.n, self.off:self.off + self.w] = True
        return bool((bits[~mine] == want).all())

    def untouched(self):
        p = self.parent
        bits = p.view(I32) if p.dtype == F32 else p
        return bool((bits == (NANBITS if p.dtype == F32 else self.fill)).all())


def _bits(t):
    return t.detach().contiguous().view(I32).cpu()


def _worst(val, ref, bound):
    """max |val - ref| / bound (inf for a NaN or where a zero bound is missed)."""
    val = val.detach().cpu().to(F64)
    if val.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(val).all()):
        return float('inf')
    e = (val - ref).abs()
    r = torch.where(bound > 0, e / bound.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, float('inf')), torch.zeros_like(e)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ shared float64 references
@functools.lru_cache(maxsize=None)
def _dense(H, sigmoid):
    """One 257 x 257 case per (H, sigmoid); every (M, N) of SIZES is its leading block."""
    c = PR.dense_case(257, 257, H, 11, sigmoid)
    return c, PR.scores_ref(c['s'], c['t'])


@functools.lru_cache(maxsize=None)
def _topk(H):
    c = PR.topk_case(H, 1)
    return c, PR.scores_ref(c['s'], c['t'])


def _fwd(dev, s, t, sigmoid, strided_out=False):
    """mgv_pair_scores_fwd on strided operands -> (Out, operand views)."""
    M, N, H = s.shape[0], t.shape[0], s.shape[1]
    sv, lds = _slice(s, dev)
    tv, ldt = _slice(t, dev)
    o = Out(M, N, dev, strided=strided_out)
    _call('mgv_pair_scores_fwd', H, M, N, _ptr(sv), lds, _ptr(tv), ldt, int(sigmoid), _ptr(o.v), o.ld)
    return o, (sv, lds, tv, ldt)


# ------------------------------------------------------------------------------------------------ the reference's fixture
def test_forward_all_reproduces_the_recorded_dec_all():
    """forward_all(dec_s, dec_t) of g3_ops: 30 x 30, a size the Linear-borrowing route refused with NotImplementedError.  Within dq of
    float64, and within 2 dq of the reference's own float32 output (which is under the same bound)."""
    dev = _dev()
    import deepgate
    z = load_golden('g3_ops')
    s, t, ref = (torch.from_numpy(z[k]) for k in ('dec_s', 'dec_t', 'dec_all'))
    dec = deepgate.digae_layer.DirectedInnerProductDecoder()
    got = dec.forward_all(s.to(dev), t.to(dev))
    r = PR.scores_ref(s, t)
    w64, wfx = _worst(got, r['p'], r['dq']), _worst(got, ref.to(F64), 2 * r['dq'])
    print('PS forward_all dec_all 30x30 | float64 %.2g/1 | fixture %.2g/1' % (w64, wfx))
    assert got.shape == (30, 30) and w64 <= 1 and wfx <= 1
    raw = dec.forward_all(s.to(dev), t.to(dev), sigmoid=False)
    assert _worst(raw, r['raw'], r['raw_bound']) <= 1


def test_directed_gae_forward_on_a_100_node_graph():
    """DirectedGAE(enc)(data) at a size that is none of 16 / 32 / 64 / 128, against float64 of the encoder's own outputs."""
    dev = _dev()
    import deepgate
    from test_digae_spec import build
    enc = build('a1b0').to(dev)
    model = deepgate.digae_model.DirectedGAE(enc)
    g = torch.Generator().manual_seed(5)
    N = 100
    x = torch.nn.functional.one_hot(torch.randint(0, 6, (N,), generator=g), 6).long().to(dev)
    ei = torch.stack([torch.randint(0, N, (300,), generator=g), torch.randint(0, N, (300,), generator=g)]).to(dev)
    with torch.no_grad():
        adj = model(types.SimpleNamespace(x=x, edge_index=ei))
        s, t = model.encode(x, x, ei)
    r = PR.scores_ref(s.cpu(), t.cpu())
    w = _worst(adj, r['p'], r['dq'])
    print('PS DirectedGAE.forward N=100 | %.2g/1' % w)
    assert adj.shape == (N, N) and w <= 1


# ------------------------------------------------------------------------------------------------ dense forward
@pytest.mark.parametrize('H', HS)
def test_dense_forward_every_shape(H):
    """M, N over SIZES independently, with and without the sigmoid, strided operands, alternating contiguous / strided outputs."""
    dev = _dev()
    bad, worst = [], {True: 0.0, False: 0.0}
    for sigmoid in (True, False):
        c, r = _dense(H, sigmoid)
        ref, bound = (r['p'], r['dq']) if sigmoid else (r['raw'], r['raw_bound'])
        for i, M in enumerate(SIZES):
            for j, N in enumerate(SIZES):
                o, _ = _fwd(dev, c['s'][:M], c['t'][:N], sigmoid, strided_out=(i + j) % 2 == 1)
                w = _worst(o.v, ref[:M, :N], bound[:M, :N])
                worst[sigmoid] = max(worst[sigmoid], w)
                if not w <= 1:
                    bad.append('M=%d N=%d sigmoid=%s: %.3g of the bound' % (M, N, sigmoid, w))
                if not o.intact():
                    bad.append('M=%d N=%d sigmoid=%s: guard rows or foreign columns changed' % (M, N, sigmoid))
    print('PS pair_scores_fwd H=%d 10x10 shapes | p %.2g/1 | raw %.2g/1' % (H, worst[True], worst[False]))
    assert not bad, bad


def test_dense_forward_empty_sides_launch_nothing():
    dev = _dev()
    for M, N in ((0, 17), (17, 0), (0, 0)):
        o = Out(max(M, 1), max(N, 1), dev)
        s, t = torch.full((max(M, 1), 16), NAN, device=dev), torch.full((max(N, 1), 16), NAN, device=dev)
        _call('mgv_pair_scores_fwd', 16, M, N, _ptr(s), 16, _ptr(t), 16, 1, _ptr(o.v), o.ld)
        assert o.untouched(), (M, N)
    from deepgate import ops
    assert ops.pair_scores(torch.zeros(0, 16, device=dev), torch.zeros(5, 16, device=dev)).shape == (0, 5)
    assert ops.pair_scores(torch.zeros(5, 16, device=dev), torch.zeros(0, 16, device=dev)).shape == (5, 0)


def test_dense_forward_65_by_65_tiles():
    """H = 16, M = N = 4,097: 65 row tiles by 65 column tiles, the last of each with one row / column; the fifth chunk of column tiles
    of every row tile holds that one tile (the kernel has no grid cap: every tile has its own place in the grid)."""
    dev = _dev()
    n = 4097
    c = PR.dense_case(n, n, 16, 3, True)
    r = PR.scores_ref(c['s'], c['t'])
    o, _ = _fwd(dev, c['s'], c['t'], True)
    w = _worst(o.v, r['p'], r['dq'])
    print('PS pair_scores_fwd H=16 4097x4097 | %.2g/1' % w)
    assert w <= 1 and o.intact()


def test_surface_forward_matches_the_abi_bit_for_bit_and_takes_column_halves():
    dev = _dev()
    from deepgate import ops
    c, r = _dense(64, True)
    st = torch.cat([c['s'], c['t']], 1).to(dev)            # the two halves of one [N, 2H] matrix, as on the models
    got = ops.pair_scores(st[:, :64], st[:, 64:])
    o, _ = _fwd(dev, c['s'], c['t'], True)
    assert torch.equal(_bits(got), _bits(o.v))
    assert torch.equal(_bits(ops.dense_scores(st[:, :64], st[:, 64:])), _bits(_fwd(dev, c['s'], c['t'], False)[0].v))


def test_old_and_new_route_agree_at_64_nodes():
    """The four sizes forward_all accepted before came from the Linear kernel with t as the weight (exact fp32, another k order):
    both are within H 2^-24 S of float64, hence within twice that of each other."""
    dev = _dev()
    c, r = _dense(64, False)
    s, t = c['s'][:64].to(dev).contiguous(), c['t'][:64].to(dev).contiguous()
    old = torch.empty(64, 64, device=dev)
    _call('mgv_linear_fwd', 64, _ptr(s), 64, 64, None, 0, 0, _ptr(t), None, 64, _ptr(old), 64)
    import deepgate
    new = deepgate.digae_layer.DirectedInnerProductDecoder().forward_all(s, t, sigmoid=False)
    w = _worst(new, old.cpu().to(F64), 2 * r['raw_bound'][:64, :64])
    print('PS forward_all against the Linear route N=64 | %.2g/1' % w)
    assert w <= 1 and _worst(new, r['raw'][:64, :64], r['raw_bound'][:64, :64]) <= 1


def test_a_dense_request_beyond_the_device_names_topk():
    dev = _dev()
    from deepgate import _hip, ops
    free, _ = torch.cuda.mem_get_info(dev)
    n = int((2 * free / 4) ** 0.5) + 4096
    s = torch.zeros(n, 16, device=dev)
    with pytest.raises(_hip.HipLibraryError, match='topk'):
        ops.pair_scores(s, s)


# ------------------------------------------------------------------------------------------------ backward
BWD_SHAPES = ((1, 1), (17, 65), (65, 17), (64, 64), (129, 257), (257, 30))


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('H', HS)
def test_dense_backward(H, sigmoid):
    """ds only, dt only and both; accumulators start as NaN (they are written, not added to); two runs give the same bits."""
    dev = _dev()
    c, _ = _dense(H, sigmoid)
    bad, worst = [], {'ds': 0.0, 'dt': 0.0}
    for M, N in BWD_SHAPES:
        s, t, g = c['s'][:M], c['t'][:N], c['g'][:M, :N].contiguous()
        r = PR.grads_ref(s, t, g, sigmoid)
        o, (sv, lds, tv, ldt) = _fwd(dev, s, t, sigmoid, strided_out=True)
        gv = Out(M, N, dev, strided=True)
        gv.v.copy_(g)
        first = {}
        for mode in ('both', 'ds', 'dt', 'both'):
            ds, dt = Out(M, H, dev, strided=True), Out(N, H, dev, strided=True)
            _call('mgv_pair_scores_bwd', H, M, N, _ptr(sv), lds, _ptr(tv), ldt, int(sigmoid), _ptr(o.v), o.ld, _ptr(gv.v), gv.ld,
                  _ptr(ds.v) if mode != 'dt' else None, ds.ld, _ptr(dt.v) if mode != 'ds' else None, dt.ld)
            for k, buf in (('ds', ds), ('dt', dt)):
                if mode not in ('both', k):
                    if not buf.untouched():
                        bad.append('%dx%d %s: %s was not asked for and changed' % (M, N, mode, k))
                    continue
                w = _worst(buf.v, r[k], r[k + '_bound'])
                worst[k] = max(worst[k], w)
                if not w <= 1:
                    bad.append('%dx%d %s: %s %.3g of its bound' % (M, N, mode, k, w))
                if not buf.intact():
                    bad.append('%dx%d %s: guard rows or foreign columns of %s changed' % (M, N, mode, k))
                if k in first and not torch.equal(first[k], _bits(buf.v)):
                    bad.append('%dx%d %s: %s differs in bits from the first run' % (M, N, mode, k))
                first.setdefault(k, _bits(buf.v))
    print('PS pair_scores_bwd H=%d sigmoid=%s | ds %.2g/1 | dt %.2g/1' % (H, sigmoid, worst['ds'], worst['dt']))
    assert not bad, bad


@pytest.mark.parametrize('sigmoid', [True, False])
def test_backward_through_autograd_on_forward_all(sigmoid):
    dev = _dev()
    import deepgate
    c, _ = _dense(32, sigmoid)
    M, N = 65, 129
    s, t, g = c['s'][:M], c['t'][:N], c['g'][:M, :N].contiguous()
    r = PR.grads_ref(s, t, g, sigmoid)
    sd, td = s.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    out = deepgate.digae_layer.DirectedInnerProductDecoder().forward_all(sd, td, sigmoid=sigmoid)
    out.backward(g.to(dev))
    ws, wt = _worst(sd.grad, r['ds'], r['ds_bound']), _worst(td.grad, r['dt'], r['dt_bound'])
    print('PS autograd forward_all 65x129 sigmoid=%s | ds %.2g/1 | dt %.2g/1' % (sigmoid, ws, wt))
    assert ws <= 1 and wt <= 1
    # one side only
    sd2 = s.to(dev).requires_grad_(True)
    deepgate.digae_layer.DirectedInnerProductDecoder().forward_all(sd2, t.to(dev), sigmoid=sigmoid).backward(g.to(dev))
    assert torch.equal(_bits(sd2.grad), _bits(sd.grad))


# ------------------------------------------------------------------------------------------------ consistency on the device
@pytest.mark.parametrize('H', HS)
def test_listed_pairs_equal_the_dense_entries_bit_for_bit(H):
    """All 257 x 257 pairs, with and without the sigmoid, through the ABI on strided operands and through ops.pair_scores_at."""
    dev = _dev()
    from deepgate import ops
    n = 257
    src = torch.arange(n, device=dev).repeat_interleave(n)
    dst = torch.arange(n, device=dev).repeat(n)
    for sigmoid in (True, False):
        c, r = _dense(H, sigmoid)
        o, (sv, lds, tv, ldt) = _fwd(dev, c['s'], c['t'], sigmoid)
        at = Out(n * n, 1, dev)
        _call('mgv_pair_scores_at', H, n * n, _ptr(sv), lds, _ptr(tv), ldt, _ptr(src), _ptr(dst), int(sigmoid), _ptr(at.v))
        diff = int((_bits(at.v).view(n, n) != _bits(o.v)).sum())
        print('PS pair_scores_at H=%d sigmoid=%s | %d of %d entries differ in bits from the dense entry' % (H, sigmoid, diff, n * n))
        assert diff == 0 and at.intact()
        got = ops.pair_scores_at(sv, tv, torch.stack([src, dst]), sigmoid=sigmoid)
        assert torch.equal(_bits(got).view(n, n), _bits(o.v))


def _run_topk(dev, c, k, gp, sigmoid, threshold, skip_self):
    H, N = c['H'], c['N']
    sv, lds = _slice(c['s'], dev)
    tv, ldt = _slice(c['t'], dev)
    idx, score, na = Out(N, k, dev, dtype=I32), Out(N, k, dev), Out(N, 1, dev, dtype=I32)
    gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
    _call('mgv_pair_topk', H, N, _ptr(sv), lds, _ptr(tv), ldt, _ptr(gpd), 0 if gp is None else len(gp) - 1, k, int(sigmoid),
          float(threshold), int(skip_self), _ptr(idx.v), _ptr(score.v), _ptr(na.v))
    assert idx.intact() and score.intact() and na.intact()
    return idx.v.cpu(), score.v.cpu(), na.v.cpu().flatten()


@pytest.mark.parametrize('k', [1, 4, 8, 32])
@pytest.mark.parametrize('H', HS)
def test_topk(H, k):
    """Graphs of (1, 2, 63, 64, 65, 130, 5, 200) nodes in one batch and the same nodes as one graph (graph_ptr NULL); with and without
    skip_self; against float64 with no exclusions (pair_scores_ref.check_topk), against the dense entry bit for bit, and the planted
    rows: exact ties across a column-tile boundary in ascending id order, a graph's first and last node found and the next graph's
    first node never, self skipped where it is the row's maximum."""
    dev = _dev()
    c, r = _topk(H)
    N, gp, info = c['N'], c['graph_ptr'], c['info']
    bad = []
    for sigmoid, thr in ((True, 0.5), (False, 0.0)):
        dense = _fwd(dev, c['s'], c['t'], sigmoid)[0].v.cpu()
        ref, bound = (r['p'], r['dq']) if sigmoid else (r['raw'], r['raw_bound'])
        for g in (gp, None):
            for skip in (False, True):
                if not sigmoid and (g is None) != skip:
                    continue                                # (the raw-score runs: one with and one without the table)
                tag = 'H=%d k=%d sigmoid=%s graphs=%s skip_self=%s' % (H, k, sigmoid, g is not None, skip)
                idx, score, na = _run_topk(dev, c, k, g, sigmoid, thr, skip)
                bad += ['%s: %s' % (tag, b) for b in PR.check_topk(idx, score, r, g, k, skip, sigmoid)[:5]]
                # bit for bit against the dense entry
                ok = idx >= 0
                pick = dense.gather(1, idx.clamp(min=0).long())
                if not torch.equal(_bits(score)[ok], _bits(pick)[ok]):
                    bad.append('%s: a score differs in bits from the dense entry its index names' % tag)
                mask = PR.candidate_mask(N, g, skip)
                cnt = ((dense > thr) & mask).sum(1)
                if not torch.equal(na.long(), cnt):
                    bad.append('%s: n_above differs from the dense row\'s count in %d rows' % (tag, int((na.long() != cnt).sum())))
                lo, hi = ((ref - bound > thr) & mask).sum(1), ((ref + bound > thr) & mask).sum(1)
                if not bool(((na >= lo) & (na <= hi)).all()):
                    bad.append('%s: n_above outside the float64 counts at threshold -/+ bound' % tag)
                # padding where k exceeds the candidates
                ncand = mask.sum(1)
                if not torch.equal((idx >= 0).sum(1), ncand.clamp(max=k)):
                    bad.append('%s: the number of returned links is not min(k, candidates)' % tag)
                # planted rows (float64 says which rows the tie heads; the tied scores are equal bits on the device)
                a, b, d = info['ties']
                want, _ = PR.topk_ref(r['raw'], g, min(k, 3), skip, sigmoid)
                rows = [u for u in range(N) if want[u].tolist() == [a, b, d][:min(k, 3)]]
                if not rows or not torch.equal(idx[rows][:, :min(k, 3)], want[rows]):
                    bad.append('%s: tied columns not in ascending id order' % tag)
                u, v0, v1, vx = info['edge_row']
                if g is not None:
                    if vx in idx[u].tolist() or idx[u, 0] != v1 or (k > 1 and idx[u, 1] != v0):
                        bad.append('%s: row %d should start %d, %d and never hold %d: %s' % (tag, u, v1, v0, vx, idx[u].tolist()))
                elif idx[u, 0] != vx:
                    bad.append('%s: one graph: row %d should start with %d' % (tag, u, vx))
                us = info['self_row']
                if (us in idx[us].tolist()) == skip or (not skip and idx[us, 0] != us):
                    bad.append('%s: self row %d: %s' % (tag, us, idx[us].tolist()))
    print('PS pair_topk H=%d k=%d | %d findings' % (H, k, len(bad)))
    assert not bad, bad


def test_topk_surface_and_nan_scores():
    """ops.pair_topk / decoder.topk equal the ABI's answer; a NaN score is never selected or counted."""
    dev = _dev()
    import deepgate
    c, r = _topk(32)
    gp = c['graph_ptr']
    idx, score, na = _run_topk(dev, c, 8, gp, True, 0.5, True)
    dec = deepgate.digae_layer.DirectedInnerProductDecoder()
    i2, s2, n2 = dec.topk(c['s'].to(dev), c['t'].to(dev), 8, graph_ptr=gp, skip_self=True)
    assert i2.dtype == I32 and n2.dtype == I32 and i2.is_cuda
    assert torch.equal(i2.cpu(), idx) and torch.equal(_bits(s2), _bits(score)) and torch.equal(n2.cpu(), na)
    t = c['t'].clone()
    poisoned = [gp[5] + 3, gp[5] + 70, gp[7] + 1]
    t[poisoned] = NAN
    i3, s3, n3 = dec.topk(c['s'].to(dev), t.to(dev), 32, graph_ptr=gp)
    assert not bool(torch.isin(i3.cpu().long(), torch.tensor(poisoned)).any()) and not bool(torch.isnan(s3).any())
    raw = r['raw'].clone()
    raw[:, poisoned] = NAN
    want = PR.row_counts(torch.sigmoid(raw), gp, 0.5)
    lo = PR.row_counts(torch.sigmoid(raw) - r['dq'], gp, 0.5)
    hi = PR.row_counts(torch.sigmoid(raw) + r['dq'], gp, 0.5)
    assert bool(((n3.cpu() >= lo) & (n3.cpu() <= hi)).all()), int((n3.cpu() != want).sum())
    sizes = torch.tensor(gp[1:]) - torch.tensor(gp[:-1])
    cand = torch.repeat_interleave(sizes, sizes)
    for g_, p_ in ((5, 2), (7, 1)):
        cand[gp[g_]:gp[g_ + 1]] -= p_
    assert torch.equal((i3.cpu() >= 0).sum(1), cand.clamp(max=32))


# ------------------------------------------------------------------------------------------------ counts
def test_reconstruction_counts_and_predict_links_on_the_models():
    dev = _dev()
    import deepgate
    from deepgate import ops
    H = 64
    c, _ = _topk(H)
    gp, N = c['graph_ptr'], c['N']
    ei = PR.edges_case(c, 3, 1).to(dev)
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev)
    hs = c['s'].to(dev)
    with torch.no_grad():
        st = ops.linear(hs, model.hs_decompose.weight, model.hs_decompose.bias)
    s, t = st[:, :H].cpu(), st[:, H:].cpu()
    r = PR.scores_ref(s, t)
    mask = PR.candidate_mask(N, gp, False)
    assert PR.band_fraction(r['p'], r['dq'], 0.5, mask) <= 1e-3
    counts = model.reconstruction_counts(hs, ei, gp)
    assert counts.dtype == I64 and counts.is_cuda and counts.shape == (len(gp) - 1, 4)
    counts = counts.cpu()
    lo, hi = PR.graph_counts(r['p'] - r['dq'], ei.cpu(), gp, 0.5), PR.graph_counts(r['p'] + r['dq'], ei.cpu(), gp, 0.5)
    print('PS reconstruction_counts | device %s | float64 low %s high %s' % (counts.sum(0).tolist(), lo.sum(0).tolist(), hi.sum(0).tolist()))
    assert bool(((counts >= lo) & (counts <= hi)).all())
    assert torch.equal(counts[:, 2:], lo[:, 2:])
    # the integers sum over the graphs to the whole-batch counts exactly, and agree with the dense matrix to the bit
    dense = ops.pair_scores(st[:, :H], st[:, H:]).cpu()
    tot = counts.sum(0).tolist()
    assert tot[0] == int((ops.pair_scores_at(st[:, :H], st[:, H:], ei) > 0.5).sum()) == int((dense[ei[0].cpu(), ei[1].cpu()] > 0.5).sum())
    assert tot[1] == int(((dense > 0.5) & mask).sum()) and tot[2] == ei.shape[1] and tot[3] == sum((b - a) ** 2 for a, b in zip(gp, gp[1:]))
    assert torch.equal(counts, PR.graph_counts(dense, ei.cpu(), gp, 0.5))
    # predict_links: skip_self by default, ids batch-wide, consistent with the dense matrix
    idx, score, na = model.predict_links(hs, 4, graph_ptr=gp)
    assert PR.check_topk(idx.cpu(), score.cpu(), r, gp, 4, True, True) == []
    ok = idx.cpu() >= 0
    assert torch.equal(_bits(score)[ok], _bits(dense.gather(1, idx.cpu().clamp(min=0).long()))[ok])
    # DirectedGAE carries the same two methods
    gae = deepgate.digae_model.DirectedGAE(enc)
    i2, s2, n2 = gae.predict_links(st[:, :H], st[:, H:], 4, graph_ptr=gp)
    assert torch.equal(i2, idx) and torch.equal(_bits(s2), _bits(score)) and torch.equal(n2, na)
    assert torch.equal(gae.reconstruction_counts(st[:, :H], st[:, H:], ei, gp).cpu(), counts)


def test_feature_extract_predict_links(tmp_path, capsys):
    """examples/feature_extract.py --predict_links K: name/pred_dst with ids local to the graph, name/pred_score, and the printed mean
    full-adjacency precision and recall."""
    _dev()
    import importlib

    import numpy as np
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '3', '--rounds', '1', '--batch_size', '2', '--predict_links', '4', '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(3) for k in ('hs', 'hf', 'pred_dst', 'pred_score'))
    for i in range(3):
        dst, sc = emb['graph%d/pred_dst' % i], emb['graph%d/pred_score' % i]
        n = emb['graph%d/hs' % i].shape[0]
        assert dst.shape == (n, 4) and sc.shape == (n, 4) and dst.dtype == np.int32
        assert dst.min() >= 0 and dst.max() < n                              # 1,024 nodes: four candidates everywhere, ids local
        assert not (dst == np.arange(n)[:, None]).any()                      # self skipped
        assert (np.diff(sc, axis=1) <= 0).all() and sc.min() >= 0 and sc.max() <= 1
    text = capsys.readouterr().out
    assert 'full-adjacency reconstruction over 3 graphs' in text and 'precision' in text and 'recall' in text


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_before_anything_is_launched():
    dev = _dev()
    n = 40
    s = torch.randn(n, 48, device=dev)
    o = Out(n, n, dev)
    assert _rc('mgv_pair_scores_fwd', 48, n, n, _ptr(s), 48, _ptr(s), 48, 1, _ptr(o.v), o.ld) == MGV_EUNSUPPORTED and o.untouched()
    d = Out(n, 48, dev)
    assert _rc('mgv_pair_scores_bwd', 48, n, n, _ptr(s), 48, _ptr(s), 48, 1, _ptr(o.v), o.ld, _ptr(o.v), o.ld, _ptr(d.v), d.ld, None, 48) \
        == MGV_EUNSUPPORTED and d.untouched()
    e = torch.zeros(4, dtype=I64, device=dev)
    a = Out(4, 1, dev)
    assert _rc('mgv_pair_scores_at', 48, 4, _ptr(s), 48, _ptr(s), 48, _ptr(e), _ptr(e), 1, _ptr(a.v)) == MGV_EUNSUPPORTED and a.untouched()
    s = torch.randn(n, 16, device=dev)

    def topk(H, k, gp):
        idx, score, na = Out(n, max(k, 1), dev, dtype=I32), Out(n, max(k, 1), dev), Out(n, 1, dev, dtype=I32)
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        rc = _rc('mgv_pair_topk', H, n, _ptr(s), 16, _ptr(s), 16, _ptr(gpd), 0 if gp is None else len(gp) - 1, k, 1, 0.5, 0,
                 _ptr(idx.v), _ptr(score.v), _ptr(na.v))
        return rc, idx.untouched() and score.untouched() and na.untouched()
    assert topk(48, 4, None) == (MGV_EUNSUPPORTED, True)
    assert topk(16, 0, None) == (MGV_EINVAL, True)
    assert topk(16, 33, None) == (MGV_EINVAL, True)
    assert topk(16, 4, [0, 10, n - 1]) == (MGV_EINVAL, True)           # does not end at N
    assert topk(16, 4, [0, 10, n + 1]) == (MGV_EINVAL, True)
    assert topk(16, 4, [1, 10, n]) == (MGV_EINVAL, True)               # does not start at 0
    assert topk(16, 4, [0, 10, n]) == (0, False)
    assert topk(16, 32, None) == (0, False)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.pair_topk(s, s, 0)
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.pair_topk(s, s, 4, graph_ptr=[0, 10, n - 1])
