"""The Linear and row-sum entries of csrc/dense.hip and csrc/linear_x3.hip (with k_slab_sum of csrc/mgv_slab.h behind them), every
entry on its own through the C ABI against the float64 restatements of tests/dense_ref.py (pinned on the CPU by
tests/test_dense_spec.py, which also asserts the properties of the case builders used here and shows that the defects these tests
are there to catch are far outside their bounds):

  f32   mgv_linear_fwd, mgv_linear_wgrad            x3    mgv_linear_fwd_x3, mgv_linear_fwd_x3_res, mgv_linear_wgrad_x3, mgv_wpack_bf16x3
  grp   mgv_grouped_linear_fwd_x3 / _wgrad_x3       rows  mgv_gather_sum, mgv_seg_sum, mgv_class_expand, mgv_class_pull_sum

Every output has 64 guard rows behind it (NaN before the call, bit-identical after it); strided operands are column slices of wider
matrices whose other columns hold NaN, and a strided output's foreign columns must come back bit-identical; workspaces are NaN-filled
with a guard of their own; the accumulators (dW, db, the class sums) start from random a0 of their entry's own magnitude
(a0 = S u, u uniform in [-1, 1]; standard normal where nothing contributes, S = 0: such an entry must come back as a0 exactly).

Bounds: err <= tau S entry by entry, tau = 8 max(r, floor), r the worst ratio FOR THAT OUTPUT of the CPU restatement in the kernel's
arithmetic (float32, or the bf16x3 emulation struct_stage_ref.mm3) against float64 on the same inputs, floor = 2^-23 (fp32 kernels)
or 2^-17 (bf16x3); an accumulator entry additionally gets 2^-24 |a0|.  Nothing is taken from what the device returns.  DERIVED_L
names the outputs whose bound had to take the derived form max(tau, L 2^-24): dW of mgv_linear_wgrad, whose 4 waves x 512 workgroups
meet in float atomics (3.2e-6 of S on the device and 3.1e-6 in a float32 model of that design at 32,768 rows, beside tau = 9.5e-7;
L = dense_ref.chain_length = 16 per visited tile + 4 per workgroup; NOTEBOOK.md, 2026-10-18).  db of the same entry keeps tau: its worst
case on the device, 0.81 of tau at 65,875 rows, is the first candidate for the same form (L = 65 per visit + one per workgroup) should
it ever be measured outside.  Exact: the weight pack, mgv_class_expand, the degree output, and mgv_gather_sum / mgv_seg_sum against the
float32 list-order restatement, all bit for bit; rows no grouped tile names stay the sentinel; the fixed-order routes (bf16x3 weight
gradients, plain and grouped; class sums with C <= 8) give identical bits twice.

Every check prints one line `DN <entry> <shape> <case> | <output> ratio/tau | ...`; the table of the worst device ratio per entry and
output is in NOTEBOOK.md."""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_dev as DD  # noqa: E402
import dense_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, I32 = torch.float64, torch.float32, torch.int32
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()
# (entry, output) whose bound is max(tau, L 2^-24), L = dense_ref.chain_length of the case: the longest chain of sequential float32
# additions the kernel's design makes for one entry.  Only outputs a correct kernel was MEASURED to exceed tau on are listed (NOTEBOOK.md).
DERIVED_L = {('linear_wgrad', 'dW')}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _hip():
    from deepgate import _hip
    return _hip


# ------------------------------------------------------------------------------------------------ buffers
# (tests/dense_dev.py: shared with tests/test_hip_linear_pair_reference.py)
Out, _ws, _ws_intact, _a0, _bits = DD.Out, DD.ws, DD.ws_intact, DD.a0, DD.bits


def _compare(entry, tag, got, r64, tau, a0=None, chain=None):
    """Ratio err / S per output against its bound (module docstring); prints, then asserts.  chain: output -> L of this case."""
    return DD.compare('DN', DERIVED_L, entry, tag, got, r64, tau, a0, chain)


# ------------------------------------------------------------------------------------------------ Linear: cases and runners
def _cache_small(size_arg):
    """One float64 run per case, shared by every entry and test that uses the case; the cases of more than 4096 rows are used once
    and not kept."""
    def deco(fn):
        small = functools.lru_cache(maxsize=None)(fn)
        return lambda *key: small(*key) if key[size_arg] <= 4096 else fn(*key)
    return deco


@_cache_small(2)
def _lin(M, K, N, K1, strided, bias, res, coherent, grad):
    """(case, float64 run, {arithmetic: tau per output})"""
    c = DR.linear_case(M, K, N, K1=K1, strided=strided, bias=bias, res=res, coherent=coherent)
    return c, DR.linear_ref(c, want_grad=grad), {}


def _key(M, K, N, K1=None, strided=False, bias=True, res=False, coherent=False, grad=True):
    return (M, K, N, K1, strided, bias, res, coherent, grad)


def _pack(W, R, K, ldw, transpose, dev):
    """mgv_wpack_bf16x3 into a fresh [2][R K] bf16 pack with a guard behind it."""
    h = _hip()
    pack = torch.full((2 * R * K + GUARD,), NAN, dtype=torch.bfloat16, device=dev)
    h.call('mgv_wpack_bf16x3', h.ptr(W), R, K, ldw, int(transpose), h.ptr(pack[:R * K]), h.ptr(pack[R * K:]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(pack[2 * R * K:]).all()), 'the weight packer wrote behind its planes'
    return pack


def _forward(mm, dev, N, X1, X2, W, b, R, M, strided_out, transposed=False):
    """One forward call: Y [N][M] = [X1 | X2] A^T + b + R with A = W (M x K) or, transposed, the transposed view of W (K x M: the input
    gradient).  X1 / X2 / R are device views (or None); returns the Out."""
    h = _hip()
    p = h.ptr
    K1, K2 = X1.shape[1], 0 if X2 is None else X2.shape[1]
    Y = Out(N, M, dev, strided_out)
    xs = (p(X1), K1, X1.stride(0), p(X2), K2, 0 if X2 is None else X2.stride(0))
    if mm == 'x3':
        pack = _pack(W, M, K1 + K2, W.stride(0), transposed, dev)
        if R is not None:
            h.call('mgv_linear_fwd_x3_res', N, *xs, p(pack), p(b), M, p(R), R.stride(0), p(Y.v), Y.ld)
        else:
            h.call('mgv_linear_fwd_x3', N, *xs, p(pack), p(b), M, p(Y.v), Y.ld)
    else:
        assert R is None
        h.call('mgv_linear_fwd', N, *xs, p(W.t().contiguous() if transposed else W), p(b), M, p(Y.v), Y.ld)
    torch.cuda.synchronize()
    assert Y.intact(), 'a forward wrote outside its rows and columns'
    return Y


def _on(c, dev):
    f = lambda o: None if o is None else o.on(dev)       # noqa: E731
    d = {k: f(c[k]) for k in ('X1', 'X2', 'R', 'dY')}
    d['W'], d['b'] = c['W'].to(dev), None if c['b'] is None else c['b'].to(dev)
    return d


def _tau_of(mm, c, r64, taus, grad):
    if mm not in taus:
        taus[mm] = DR.taus(r64, DR.linear_ref(c, F32, 'x3' if mm == 'x3' else 'exact', want_grad=grad), mm)
    return taus[mm]


def _check_fwd(mm, key, dev, with_dx=False):
    c, r64, taus = _lin(*key)
    d = _on(c, dev)
    M, K, N = c['M'], c['K'], c['N']
    got = {'Y': _forward(mm, dev, N, d['X1'], d['X2'], d['W'], d['b'], d['R'], M, c['strided']).v}
    if with_dx:
        got['dX'] = _forward(mm, dev, N, d['dY'], None, d['W'], None, None, K, c['strided'], transposed=True).v
    tag = '(%d,%d) N=%d K1=%s%s%s%s%s' % (M, K, N, c['K1'], ' strided' if c['strided'] else '', '' if c['b'] is not None else ' nobias',
                                         ' res' if c['R'] is not None else '', ' coherent' if key[7] else '')
    return _compare('linear_fwd' + ('_x3' if mm == 'x3' else ''), tag, got, r64, _tau_of(mm, c, r64, taus, key[-1]))


def _wgrad(mm, c, r64, dev, seed=1, with_db=True):
    h = _hip()
    p = h.ptr
    d = _on(c, dev)
    M, K, N = c['M'], c['K'], c['N']
    a0 = {'dW': _a0(r64['S']['dW'], seed), 'db': _a0(r64['S']['db'], seed + 1)}
    dW, db = Out(M, K, dev, fill=a0['dW'].to(dev)), Out(1, M, dev, fill=a0['db'].to(dev)[None])
    xs = (p(d['X1']), c['K1'], d['X1'].stride(0), p(d['X2']), c['K2'], 0 if d['X2'] is None else d['X2'].stride(0))
    if mm == 'x3':
        nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
        assert nws >= DR.grid('linear_wgrad_x3', (M, K), N) * (M * K + M)
        ws = _ws(nws, dev)
        h.call('mgv_linear_wgrad_x3', N, *xs, p(d['dY']), d['dY'].stride(0), M, p(dW.v), p(db.v) if with_db else None, p(ws), nws)
        torch.cuda.synchronize()
        assert _ws_intact(ws, nws), 'the weight gradient wrote behind its workspace'
    else:
        h.call('mgv_linear_wgrad', N, *xs, p(d['dY']), d['dY'].stride(0), M, p(dW.v), p(db.v) if with_db else None)
        torch.cuda.synchronize()
    assert dW.intact() and db.intact(), 'a weight gradient wrote behind its accumulator'
    if not with_db:
        assert torch.equal(db.v[0].cpu(), a0['db']), 'db touched through a NULL pointer?'
        return {'dW': dW.v}, {'dW': a0['dW']}
    return {'dW': dW.v, 'db': db.v[0]}, a0


def _check_wgrad(mm, key, dev, with_db=True):
    c, r64, taus = _lin(*key)
    got, a0 = _wgrad(mm, c, r64, dev, with_db=with_db)
    tag = '(%d,%d) N=%d K1=%s%s%s' % (c['M'], c['K'], c['N'], c['K1'], ' strided' if c['strided'] else '', '' if with_db else ' nodb')
    return _compare('linear_wgrad' + ('_x3' if mm == 'x3' else ''), tag, got, r64, _tau_of(mm, c, r64, taus, key[-1]), a0,
                    None if mm == 'x3' else (lambda k: DR.chain_length('linear_wgrad', k, (c['M'], c['K']), c['N'])))


def _variants(K, res=False):
    """(K1, strided, bias, res) in turn over the sizes: one input / the two-input form with the seam at 4, K / 2 and K - 4; contiguous /
    column slices of NaN-holding matrices; bias NULL; the residual entry."""
    return [(None, False, True, False), (4, True, True, res), (K // 2, False, False, False), (K - 4, True, True, res), (None, True, True, res)]


def _small(M, K, res=False, grad=True):
    v = _variants(K, res)
    return [_key(M, K, N, *v[i % len(v)], grad=grad) for i, N in enumerate(DR.SMALL_ROWS)] + [_key(M, K, 129, K // 2, True, True, res, grad=grad)]


def _big(kernel, M, K, grad):
    cap = DR.cap_rows(kernel, (M, K))
    return [_key(M, K, cap, grad=grad), _key(M, K, cap + 1, grad=grad), _key(M, K, DR.large_rows(kernel, (M, K)), K // 2, grad=grad)]


@pytest.mark.parametrize('M', DR.F32_FWD_M)
def test_linear_fwd_f32(M):
    """mgv_linear_fwd: M x K in {16, 48, 128, 256} at 1 .. 129 rows with the stride, seam and bias forms in turn; (64, 64) also at the
    grid cap, one row past it and at the size where workgroups 0..5 visit three tiles, the others two and the last tile is partial."""
    dev, bad = _dev(), []
    for K in DR.F32_FWD_K + ((64,) if M == 64 else ()):
        for key in _small(M, K, grad=False) + (_big('linear_fwd', M, K, False) if (M, K) == (64, 64) else []):
            bad += _check_fwd('f32', key, dev)
    if M == 64:
        bad += _check_fwd('f32', _key(64, 64, 129, 32, True), dev, with_dx=True)
    assert not bad, bad


@pytest.mark.parametrize('M,K', DR.F32_WGRAD_SHAPES)
def test_linear_wgrad_f32(M, K):
    """mgv_linear_wgrad (float atomics between the workgroups: no bit-identity asserted), all ten shapes, db NULL once."""
    dev, bad = _dev(), []
    for key in _small(M, K) + (_big('linear_wgrad', M, K, True) if (M, K) == (64, 64) else []):
        bad += _check_wgrad('f32', key, dev)
    bad += _check_wgrad('f32', _key(M, K, 65, None, True), dev, with_db=False)
    assert not bad, bad


@pytest.mark.parametrize('M,K', DR.X3_SHAPES)
def test_linear_fwd_x3(M, K):
    """mgv_linear_fwd_x3 and mgv_linear_fwd_x3_res (the variants with a residual), and the input gradient as the forward over the
    transposed pack; the coherent case (dense_ref.linear_case) where a lost hi.lo term is 30x outside the bound."""
    dev, bad = _dev(), []
    for key in _small(M, K, res=True) + (_big('linear_fwd_x3', M, K, False) if (M, K) == (64, 128) else []):
        bad += _check_fwd('x3', key, dev, with_dx=key[-1])
    bad += _check_fwd('x3', _key(M, K, 65, coherent=True), dev, with_dx=True)
    assert not bad, bad


@pytest.mark.parametrize('M,K', DR.X3_SHAPES)
def test_linear_wgrad_x3(M, K):
    """mgv_linear_wgrad_x3; for the two thread counts, (64, 128) and (32, 32), also every regime of k_slab_sum (1 .. 147 tiles = slab
    rows), the grid cap, one row past it and the two-and-three-tiles size; and two identical calls give identical bits."""
    dev, bad = _dev(), []
    keys = _small(M, K)
    if (M, K) in ((64, 128), (32, 32)):
        keys += [_key(M, K, DR.slab_rows(t)) for t in DR.SLAB_TILES] + _big('linear_wgrad_x3', M, K, True)
    for key in keys:
        bad += _check_wgrad('x3', key, dev)
    bad += _check_wgrad('x3', _key(M, K, 65, None, True), dev, with_db=False)
    bad += _check_wgrad('x3', _key(M, K, 65, coherent=True), dev)
    c, r64, _ = _lin(*_key(M, K, DR.slab_rows(147)))
    a, _ = _wgrad('x3', c, r64, dev)
    b, _ = _wgrad('x3', c, r64, dev)
    assert all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a), 'the fixed-order weight gradient differs between two identical calls'
    assert not bad, bad


@pytest.mark.parametrize('R,K', [(64, 128), (128, 64), (32, 32), (192, 64), (64, 192)])
def test_wpack_bits(R, K):
    """mgv_wpack_bf16x3 bit for bit: both transpose settings, W contiguous and as a column slice (ldw > K) of a NaN-holding matrix."""
    dev = _dev()
    g = DR._gen(7, R, K)
    for transpose in (0, 1):
        shape = (K, R) if transpose else (R, K)                  # W itself: [R][K], or [K][R] behind the transposed view
        for strided in (False, True):
            W = DR.Operand(DR.scaled_rows(g, *shape), strided)
            want = DR.wpack(W.v, transpose)
            pack = _pack(W.on(dev), R, K, W.ld, transpose, dev)
            got = pack[:2 * R * K].view(torch.int16).cpu()
            assert torch.equal(got[:R * K], want[0]) and torch.equal(got[R * K:], want[1]), (R, K, transpose, strided)
    print('DN wpack (%d,%d) | hi and lo planes bit-identical in 4 forms' % (R, K))


# ------------------------------------------------------------------------------------------------ grouped Linear
@functools.lru_cache(maxsize=None)
def _grp(M, K, ntiles, subset, bias, res, strided, fwd, wgrad):
    c = DR.grouped_case(M, K, ntiles=ntiles, subset=subset, bias=bias, res=res, strided=strided)
    r64 = DR.grouped_ref(c, fwd=fwd, wgrad=wgrad)
    return c, r64, DR.taus(r64, DR.grouped_ref(c, F32, 'x3', fwd=fwd, wgrad=wgrad), 'x3')


def _tables_on(c, dev):
    return {k: (None if t is None else t.to(dev)) for k, t in c['tables'].items()}


def _grouped_fwd(c, dev):
    h = _hip()
    p = h.ptr
    M, K, T = c['M'], c['K'], c['T']
    tb = _tables_on(c, dev)
    W = c['W'].to(dev)
    pack = torch.cat([_pack(W[s], M, K, K, 0, dev)[:2 * M * K] for s in range(T)] + [torch.full((GUARD,), NAN, dtype=torch.bfloat16, device=dev)])
    X, R = c['X'].on(dev), None if c['R'] is None else c['R'].on(dev)
    b = None if c['b'] is None else c['b'].to(dev)
    Y = Out(c['Nn'], M, dev, c['strided'])
    n = tb['tile_count'].numel() if tb['tile_list'] is None else tb['tile_list'].numel()
    h.call('mgv_grouped_linear_fwd_x3', n, p(tb['tile_list']), p(tb['order']), p(tb['tile_start']), p(tb['tile_count']), p(tb['tile_slot']),
           p(X), K, X.stride(0), p(pack), p(b), M, p(R), 0 if R is None else R.stride(0), p(Y.v), Y.ld)
    torch.cuda.synchronize()
    return Y


def _grouped_wgrad(c, r64, dev, seed=3):
    h = _hip()
    p = h.ptr
    M, K = c['M'], c['K']
    tb = _tables_on(c, dev)
    X, dY = c['X'].on(dev), c['dY'].on(dev)
    a0 = {'dW': _a0(r64['S']['dW'], seed), 'db': _a0(r64['S']['db'], seed + 1)}
    dW, db = Out(M, K, dev, fill=a0['dW'].to(dev)), Out(1, M, dev, fill=a0['db'].to(dev)[None])
    n = tb['tile_count'].numel() if tb['tile_list'] is None else tb['tile_list'].numel()
    nws = h.call_value('mgv_grouped_linear_wgrad_x3_ws_floats', M, K, n)
    ws = _ws(nws, dev)
    h.call('mgv_grouped_linear_wgrad_x3', n, p(tb['tile_list']), p(tb['order']), p(tb['tile_start']), p(tb['tile_count']), p(X), K, X.stride(0),
           p(dY), dY.stride(0), M, p(dW.v), p(db.v), p(ws), nws)
    torch.cuda.synchronize()
    assert _ws_intact(ws, nws) and dW.intact() and db.intact(), 'the grouped weight gradient wrote outside its buffers'
    return {'dW': dW.v, 'db': db.v[0]}, a0


FORMS = [(False, True, False, False), (True, True, True, False), (True, False, True, True), (False, True, True, True), (True, True, False, True)]


@pytest.mark.parametrize('M,K', DR.GROUPED_FWD)
def test_grouped_linear_fwd(M, K):
    """mgv_grouped_linear_fwd_x3 over hand-built tables (dense_ref.grouped_case: tiles of 64, 1, 63 and 0 rows, a non-monotone order
    with nodes left out, slots out of order with biases 10 apart), tile_list NULL and a shuffled strict subset, b NULL, R present,
    strided; 12 tiles, 150, and 1100 (the grid is capped at 512 workgroups: up to three tiles each, the next tile's rows fetched ahead
    and its slot's weights reloaded).  The rows no listed tile names come back as the NaN sentinel."""
    dev, bad = _dev(), []
    assert DR.LDS_BYTES // DR.x3_fwd_smem(M, K) == 2
    for ntiles in (12, 150, 1100):
        for subset, bias, res, strided in (FORMS if ntiles < 1100 else FORMS[1:2]):
            c, r64, tau = _grp(M, K, ntiles, subset, bias, res, strided, True, False)
            Y = _grouped_fwd(c, dev)
            assert Y.intact(), 'the grouped forward wrote outside its rows and columns'
            named = r64['named'].to(dev)
            assert bool((Y.v[~named].view(I32) == NANBITS).all()), 'a row no listed tile names was written'
            got = torch.where(named[:, None], Y.v, torch.zeros_like(Y.v))
            tag = '(%d,%d) tiles=%d%s%s%s%s' % (M, K, ntiles, ' subset' if subset else '', '' if bias else ' nobias', ' res' if res else '', ' strided' if strided else '')
            bad += _compare('grouped_fwd_x3', tag, {'Y': got}, r64, tau)
    assert not bad, bad


def test_grouped_linear_wgrad():
    """mgv_grouped_linear_wgrad_x3 at (192, 64): 12 tiles, 150 (slab rows past 128) and 1100 (past the grid cap of 512), every tile and
    a subset; fixed order: twice the same bits."""
    dev, bad = _dev(), []
    for ntiles in (12, 150, 1100):
        for subset, strided in ((False, False), (True, True)):
            c, r64, tau = _grp(192, 64, ntiles, subset, True, False, strided, False, True)
            got, a0 = _grouped_wgrad(c, r64, dev)
            again, _ = _grouped_wgrad(c, r64, dev)
            assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), 'the grouped weight gradient differs between two identical calls'
            bad += _compare('grouped_wgrad_x3', '(192,64) tiles=%d%s%s' % (ntiles, ' subset' if subset else '', ' strided' if strided else ''), got, r64, tau, a0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ row sums
ROWS_N = (1, 2, 65, 129, 1000)


@_cache_small(1)
def _gather(H, N):
    c = DR.list_case(H, N)
    return c, DR.gather_sum(c['h'], c['ptr'], c['idx']), DR.gather_sum(c['h'], c['ptr'], c['idx'], F32)


@pytest.mark.parametrize('H', DR.WIDTHS)
def test_gather_sum(H):
    """mgv_gather_sum: list lengths 0, 1, 2, 3, 5, 64, 65 and 600; H = 128 and 64 also past the grid cap.  Against float64, and BIT
    FOR BIT against the float32 restatement that adds in list order (the order the kernel promises); the degree output bit for bit,
    and the same call with a NULL degree pointer."""
    dev, bad = _dev(), []
    h = _hip()
    p = h.ptr
    for N in ROWS_N + ((DR.cap_rows('gather_sum', H) + 77,) if H >= 64 else ()):
        c, r64, r32 = _gather(H, N)
        d = {k: c[k].to(dev) for k in ('h', 'ptr', 'idx')}
        for with_deg in (True, False):
            agg, deg = Out(N, H, dev), Out(N, 1, dev)
            h.call('mgv_gather_sum', H, N, p(d['h']), p(d['ptr']), p(d['idx']), p(agg.v), p(deg.v) if with_deg else None)
            torch.cuda.synchronize()
            assert agg.intact() and deg.intact(), 'gather_sum wrote behind row N'
            if with_deg:
                assert torch.equal(deg.v[:, 0].cpu().to(F64), r64['deg'])
            else:
                assert bool((deg.parent.view(I32) == NANBITS).all())
            assert torch.equal(_bits(agg.v), _bits(r32['agg'].to(F32))), 'gather_sum does not add in list order (H=%d N=%d)' % (H, N)
        bad += _compare('gather_sum', 'H=%d N=%d' % (H, N), {'agg': agg.v}, r64, DR.taus(r64, r32, 'f32'))
    assert not bad, bad


@_cache_small(1)
def _seg(H, n_seg, items, agg, out_row):
    c = DR.seg_case(H, n_seg, items, agg, out_row)
    return c, DR.seg_ref(c), DR.seg_ref(c, F32)


@pytest.mark.parametrize('H', DR.WIDTHS)
def test_seg_sum(H):
    """mgv_seg_sum: segment lengths 0, 1, 2, 3, 64, 65 and 600, items / agg / out_row each present and absent; bit for bit against the
    float32 restatement (own row, then neighbours in list order, then into the segment's sum) besides the float64 bound; the rows of
    `out` no segment writes stay the sentinel."""
    dev, bad = _dev(), []
    h = _hip()
    p = h.ptr
    forms = [(129, i, a, o) for i in (True, False) for a in (True, False) for o in (True, False)]
    forms += [(n, f, f, f) for n in (1, 2) for f in (True, False)]
    forms += [(1000, True, True, True)] + ([(DR.cap_rows('seg_sum', H) + 77, True, True, True)] if H >= 64 else [])
    for n_seg, items, agg, out_row in forms:
        c, r64, r32 = _seg(H, n_seg, items, agg, out_row)
        d = {k: (None if c[k] is None else c[k].to(dev)) for k in ('seg_ptr', 'items', 'direct', 'agg', 'nbr_ptr', 'nbr_idx', 'out_row')}
        out = Out(c['n_out'], H, dev)
        h.call('mgv_seg_sum', H, n_seg, p(d['seg_ptr']), p(d['items']), p(d['direct']), p(d['agg']), p(d['nbr_ptr']), p(d['nbr_idx']), p(d['out_row']), p(out.v))
        torch.cuda.synchronize()
        assert out.intact(), 'seg_sum wrote behind its output'
        rows = r64['rows'].to(dev)
        rest = torch.ones(c['n_out'], dtype=torch.bool, device=dev)
        rest[rows] = False
        assert int(rest.sum()) == 7 and bool((out.v[rest].view(I32) == NANBITS).all()), 'a row no segment names was written'
        got = out.v[rows]
        assert torch.equal(_bits(got), _bits(r32['out'].to(F32))), 'seg_sum does not add in list order (H=%d %s)' % (H, (n_seg, items, agg, out_row))
        tag = 'H=%d n_seg=%d%s%s%s' % (H, n_seg, ' items' if items else '', ' agg' if agg else '', ' out_row' if out_row else '')
        bad += _compare('seg_sum', tag, {'out': got}, r64, DR.taus(r64, r32, 'f32'))
    assert not bad, bad


@_cache_small(1)
def _cls(H, N, C, agg):
    c = DR.class_case(H, N, C, agg)
    r64 = DR.class_ref(c)
    return c, r64, DR.taus(r64, DR.class_ref(c, F32), 'f32')


def _pull(c, r64, dev, seed=5):
    h = _hip()
    p = h.ptr
    H, N, C = c['H'], c['N'], c['C']
    d = {k: (None if c[k] is None else c[k].to(dev)) for k in ('gy_direct', 'gy_agg', 'ptr', 'idx', 'class_id')}
    a0 = _a0(r64['S']['out'], seed)
    out = Out(C, H, dev, fill=a0.to(dev))
    nws = h.call_value('mgv_class_pull_sum_ws_floats', H, N, C)
    assert nws == DR.grid('class_pull_sum', H, N) * C * H
    ws = _ws(nws, dev)
    h.call('mgv_class_pull_sum', H, N, p(d['gy_direct']), p(d['gy_agg']), p(d['ptr']), p(d['idx']), p(d['class_id']), C, p(out.v), p(ws), nws)
    torch.cuda.synchronize()
    assert out.intact() and _ws_intact(ws, nws), 'class_pull_sum wrote outside its buffers'
    return {'out': out.v}, {'out': a0}


@pytest.mark.parametrize('H', DR.WIDTHS)
def test_class_expand_and_pull_sum(H):
    """mgv_class_expand bit for bit, and mgv_class_pull_sum with C = 1, 8 (register sums) and 9, 40 (LDS atomics), gy_agg present and
    NULL, into pre-filled sums (the absent class's row must stay a0); H = 128 at the four sizes where a lane group's rows u = 1, 2, 3
    cross N and where the outer loop runs twice, H = 64 at two of them; C <= 8 twice with identical bits."""
    dev, bad = _dev(), []
    h = _hip()
    p = h.ptr
    sizes = [(N, C, True) for N in (65, 129) for C in (1, 8, 9, 40)] + [(N, C, True) for N in (1, 2) for C in (1, 9)]
    sizes += [(1000, 8, True), (1000, 40, True), (129, 8, False), (129, 9, False)]
    if H == 128:
        sizes += [(n, 8, True) for n in DR.pull_sizes(H)] + [(DR.pull_sizes(H)[3], 40, True)]
    if H == 64:
        sizes += [(DR.pull_sizes(H)[1], 8, True), (DR.pull_sizes(H)[3], 8, True), (DR.pull_sizes(H)[3], 9, True)]
    for N, C, agg in sizes:
        c, r64, tau = _cls(H, N, C, agg)
        table, cid = c['table'].to(dev), c['class_id'].to(dev)
        ex = Out(N, H, dev)
        h.call('mgv_class_expand', H, N, p(table), p(cid), p(ex.v))
        torch.cuda.synchronize()
        assert ex.intact() and torch.equal(_bits(ex.v), _bits(DR.class_expand(c['table'], c['class_id']))), 'class_expand (H=%d N=%d C=%d)' % (H, N, C)
        got, a0 = _pull(c, r64, dev)
        if C <= 8:
            again, _ = _pull(c, r64, dev)
            assert torch.equal(_bits(got['out']), _bits(again['out'])), 'the fixed-order class sums differ between two identical calls'
        bad += _compare('class_pull_sum', 'H=%d N=%d C=%d%s' % (H, N, C, '' if agg else ' noagg'), got, r64, tau, a0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ through deepgate.ops
def test_through_ops():
    """ops.linear (bf16x3 and fp32 shapes, one and two inputs), ops.linear_passthrough with a second consumer (its gradient rides in as
    the residual of the input-gradient kernel), ops.RoundGhFn over the hand-built tables and ops.gather_sum: the same bounds."""
    dev, bad = _dev(), []
    from deepgate import ops
    for M, K, N, K1 in ((64, 128, 129, None), (64, 128, 1000, 64), (32, 16, 129, None), (16, 32, 65, 16)):
        x3 = ops._lin_x3(M, K)
        assert x3 == ((M, K) in DR.X3_SHAPES)
        key = _key(M, K, N, K1)
        c, r64, taus = _lin(*key)
        x1 = c['X1'].v.to(dev).requires_grad_(True)
        x2 = c['X2'].v.to(dev).requires_grad_(True) if K1 else None
        W, b = c['W'].to(dev).requires_grad_(True), c['b'].to(dev).requires_grad_(True)
        y = ops.linear(x1, W, b, x2=x2)
        (y * c['dY'].v.to(dev)).sum().backward()
        got = {'Y': y, 'dX': x1.grad if x2 is None else torch.cat([x1.grad, x2.grad], 1), 'dW': W.grad, 'db': b.grad}
        bad += _compare('ops.linear', '(%d,%d) N=%d K1=%s %s' % (M, K, N, K1, 'x3' if x3 else 'f32'), got, r64, _tau_of('x3' if x3 else 'f32', c, r64, taus, True))
    # pass-through: x has a second consumer whose gradient G2 arrives through the second output
    c, _, _ = _lin(*_key(128, 64, 129))
    G2 = DR.scaled_rows(DR._gen(11), 129, 64)
    want = DR.linear(c['dY'].v, None, c['W'].t(), None, G2)
    tau = DR.taus(want, DR.linear(c['dY'].v, None, c['W'].t(), None, G2, dtype=F32, mm='x3'), 'x3')
    x = c['X1'].v.to(dev).requires_grad_(True)
    y, xp = ops.linear_passthrough(x, c['W'].to(dev), c['b'].to(dev))
    ((y * c['dY'].v.to(dev)).sum() + (xp * G2.to(dev)).sum()).backward()
    bad += _compare('ops.linear_passthrough', '(128,64) N=129', {'Y': x.grad}, want, tau)
    # RoundGhFn over a stand-in plan holding the hand-built tables
    g, r64, tau = _grp(192, 64, 12, False, True, False, False, True, False)
    tb = _tables_on(g, dev)
    slot = g['tables']['tile_slot'].long()
    by_slot = [[t for t in range(slot.numel()) if int(slot[t]) == s] for s in range(g['T'])]
    stp = [0]
    for ts in by_slot:
        stp.append(stp[-1] + len(ts))
    plan = types.SimpleNamespace(has_levels=True, num_slots=g['T'], N=g['Nn'], num_tiles=slot.numel(), order=tb['order'], tile_start=tb['tile_start'],
                                 tile_count=tb['tile_count'], tile_slot=tb['tile_slot'], slot_tile_ptr=stp,
                                 slot_tiles=torch.tensor([t for ts in by_slot for t in ts], dtype=I32, device=dev))
    hx = g['X'].v.to(dev).requires_grad_(True)
    Wg, bg = g['W'].to(dev).requires_grad_(True), g['b'].to(dev).requires_grad_(True)
    gh = ops.RoundGhFn.apply(plan, hx, Wg, bg)
    (gh * g['dY'].v.to(dev)).sum().backward()
    assert float(gh.detach()[~r64['named'].to(dev)].abs().max()) == 0
    bad += _compare('ops.RoundGhFn', 'gh', {'Y': gh}, r64, tau)
    back = DR.grouped(g['dY'].v, g['W'].transpose(1, 2), None, None, g['tables'])
    tb_ = DR.taus(back, DR.grouped(g['dY'].v, g['W'].transpose(1, 2), None, None, g['tables'], dtype=F32, mm='x3'), 'x3')
    bad += _compare('ops.RoundGhFn', 'dh', {'Y': hx.grad}, back, tb_)
    for s in range(g['T']):
        one = dict(g['tables'], tile_list=torch.tensor(by_slot[s], dtype=I32))
        w64 = DR.grouped(g['X'].v, None, None, None, one, g['dY'].v)
        tw = DR.taus(w64, DR.grouped(g['X'].v, None, None, None, one, g['dY'].v, dtype=F32, mm='x3'), 'x3')
        bad += _compare('ops.RoundGhFn', 'slot %d' % s, {'dW': Wg.grad[s], 'db': bg.grad[s]}, w64, tw)
    # ops.gather_sum takes N from h's rows: the case's h has 11 rows more than it has lists, so those rows get empty lists
    c, r64, r32 = _gather(64, 1000)
    rows = c['h'].shape[0]
    ptr = torch.cat([c['ptr'], c['ptr'][-1:].repeat(rows - c['N'])])
    assert ptr.numel() == rows + 1
    agg, deg = ops.gather_sum(c['h'].to(dev), ptr.to(dev), c['idx'].to(dev))
    assert agg.shape == (rows, 64) and deg.shape == (rows,)
    assert torch.equal(deg[:c['N']].cpu().to(F64), r64['deg']) and float(deg[c['N']:].abs().max()) == 0 and float(agg[c['N']:].abs().max()) == 0
    assert torch.equal(_bits(agg[:c['N']]), _bits(r32['agg'].to(F32)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes():
    """Every refusal is MGV_EINVAL / MGV_EUNSUPPORTED from the argument check, before any launch and with every buffer untouched;
    N = 0 and zero tiles are accepted and touch nothing.  (H < 4 used to divide by zero on the host before it was looked at, and the
    weight-gradient entries took ld < K.)"""
    dev = _dev()
    h = _hip()
    p = h.ptr
    from deepgate._hip import HipLibraryError
    N = 65
    buf = {k: torch.full(s, 7.25, device=dev) for k, s in (('X', (N, 280)), ('X2', (N, 64)), ('W', (192, 272)), ('b', (192,)), ('Y', (N, 200)), ('R', (N, 200)),
                                                            ('dW', (192, 128)), ('db', (192,)), ('ws', (1 << 16,)), ('out', (N + 8, 128)))}
    pack = torch.zeros(2 * 192 * 272, dtype=torch.bfloat16, device=dev)
    i32 = {k: torch.zeros(N + 1, dtype=I32, device=dev) for k in ('ptr', 'idx', 'cls', 'order', 'ts', 'tc', 'slot', 'tl')}
    X, X2, W, b, Y, R, dW, db, ws, out = (buf[k] for k in ('X', 'X2', 'W', 'b', 'Y', 'R', 'dW', 'db', 'ws', 'out'))

    def fwd(entry='mgv_linear_fwd', N=N, K1=64, ld1=280, K2=0, ld2=0, M=64, ldy=200, R=R, ldr=200):
        x2 = (p(X2) if K2 else None, K2, ld2)
        if entry == 'mgv_linear_fwd':
            return h.call(entry, N, p(X), K1, ld1, *x2, p(W), p(b), M, p(Y), ldy)
        if entry == 'mgv_linear_fwd_x3':
            return h.call(entry, N, p(X), K1, ld1, *x2, p(pack), p(b), M, p(Y), ldy)
        return h.call(entry, N, p(X), K1, ld1, *x2, p(pack), p(b), M, p(R), ldr, p(Y), ldy)

    def wg(entry='mgv_linear_wgrad', N=N, K1=64, ld1=280, K2=0, ld2=0, M=64, lddy=200, nws=1 << 16):
        x2 = (p(X2) if K2 else None, K2, ld2)
        tail = (p(ws), nws) if entry.endswith('x3') else ()
        return h.call(entry, N, p(X), K1, ld1, *x2, p(Y), lddy, M, p(dW), p(db), *tail)

    def gfwd(ntiles=4, M=192, K=64, ldx=280, ldy=200, R=None, ldr=0):
        return h.call('mgv_grouped_linear_fwd_x3', ntiles, None, p(i32['order']), p(i32['ts']), p(i32['tc']), p(i32['slot']), p(X), K, ldx, p(pack), p(b), M,
                      p(R), ldr, p(Y), ldy)

    def gwg(ntiles=4, M=192, K=64, ldx=280, lddy=200, nws=1 << 16):
        return h.call('mgv_grouped_linear_wgrad_x3', ntiles, None, p(i32['order']), p(i32['ts']), p(i32['tc']), p(X), K, ldx, p(Y), lddy, M, p(dW), p(db), p(ws), nws)

    def rows(entry, H, N=N, C=4, nws=1 << 16):
        if entry == 'mgv_gather_sum':
            return h.call(entry, H, N, p(X), p(i32['ptr']), p(i32['idx']), p(out), None)
        if entry == 'mgv_seg_sum':
            return h.call(entry, H, N, p(i32['ptr']), None, p(X), None, None, None, None, p(out))
        if entry == 'mgv_class_expand':
            return h.call(entry, H, N, p(X), p(i32['cls']), p(out))
        return h.call('mgv_class_pull_sum', H, N, p(X), None, None, None, p(i32['cls']), C, p(out), p(ws), nws)

    X3, RES, WG3 = 'mgv_linear_fwd_x3', 'mgv_linear_fwd_x3_res', 'mgv_linear_wgrad_x3'
    U, E = 'MGV_EUNSUPPORTED', 'MGV_EINVAL'
    refused = [
        (U, lambda: fwd(M=48)), (U, lambda: fwd(X3, K1=16)), (U, lambda: fwd(RES, M=16)), (U, lambda: wg(M=128, K1=128)), (U, lambda: wg(WG3, K1=16)),
        (U, lambda: gfwd(M=64, K=64)), (U, lambda: gwg(M=64, K=192)),
        (E, lambda: fwd(K1=24)), (E, lambda: fwd(K1=40, K2=20, ld2=64)), (E, lambda: fwd(K1=272)), (E, lambda: fwd(K1=256, K2=16, ld2=64)),
        (E, lambda: fwd(ld1=66)), (E, lambda: fwd(X3, ld1=66)), (E, lambda: fwd(ldy=66)), (E, lambda: fwd(X3, ldy=198)), (E, lambda: wg(ld1=66)), (E, lambda: wg(WG3, lddy=66)),
        (E, lambda: fwd(K1=32, K2=32, ld2=30)), (E, lambda: fwd(X3, K1=32, K2=32, ld2=30)),
        (E, lambda: fwd(ld1=60)), (E, lambda: fwd(X3, ld1=60)), (E, lambda: fwd(K1=32, K2=32, ld2=28)),
        (E, lambda: fwd(ldy=60)), (E, lambda: fwd(X3, ldy=60)), (E, lambda: fwd(RES, ldy=60)), (E, lambda: fwd(RES, ldr=60)), (E, lambda: gfwd(ldy=188)), (E, lambda: gfwd(ldx=60)),
        (E, lambda: fwd(RES, R=None)),
        (E, lambda: wg(WG3, nws=h.call_value('mgv_linear_wgrad_x3_ws_floats', 64, 64, N) - 1)),
        (E, lambda: gwg(nws=h.call_value('mgv_grouped_linear_wgrad_x3_ws_floats', 192, 64, 4) - 1)),
        (E, lambda: rows('mgv_class_pull_sum', 64, nws=h.call_value('mgv_class_pull_sum_ws_floats', 64, N, 4) - 1)),
        (E, lambda: rows('mgv_class_pull_sum', 64, C=0)), (E, lambda: rows('mgv_class_pull_sum', 128, C=65)),
        # the two host fixes of this file's pull request
        (E, lambda: wg(ld1=60)), (E, lambda: wg(WG3, ld1=60)), (E, lambda: wg(K1=32, K2=32, ld2=28)), (E, lambda: wg(WG3, K1=32, K2=32, ld2=28)), (E, lambda: gwg(ldx=60)),
    ]
    for H in (0, 2, 8, 48, 256):
        refused += [('MGV_E', lambda H=H, e=e: rows(e, H)) for e in ('mgv_gather_sum', 'mgv_seg_sum', 'mgv_class_expand', 'mgv_class_pull_sum')]
        assert h.call_value('mgv_class_pull_sum_ws_floats', H, N, 4) == 0
    assert h.call_value('mgv_class_pull_sum_ws_floats', 64, N, 4) == DR.grid('class_pull_sum', 64, N) * 4 * 64
    assert h.call_value('mgv_linear_wgrad_x3_ws_floats', 64, 64, N) == 2 * (64 * 64 + 64)
    for code, fn in refused:
        with pytest.raises(HipLibraryError, match=code):
            fn()
    # empty calls: accepted, nothing enqueued
    fwd(N=0); fwd(X3, N=0); fwd(RES, N=0); wg(N=0); wg(WG3, N=0); gfwd(ntiles=0); gwg(ntiles=0)
    for e in ('mgv_gather_sum', 'mgv_seg_sum', 'mgv_class_expand', 'mgv_class_pull_sum'):
        rows(e, 64, N=0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.25).all()) for t in buf.values())
    print('DN refusals: %d calls refused by return code, 11 empty calls accepted, every buffer untouched' % len(refused))
