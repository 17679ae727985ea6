"""mgv_linear_bwd_x3 (csrc/linear_x3.hip): the whole backward of one Linear in one pass over dY, through the C ABI, against the separate
launches it replaces — mgv_linear_wgrad_x3 for dW / db and mgv_linear_fwd_x3(_res) on the transposed packs of W's column blocks for
dX1 / dX2.  Everything is compared BIT FOR BIT (the fused kernel keeps the weight-gradient kernel's grid, tile walk and slab rows,
and forms dX with the forward kernel's MFMA chain from the same bf16 planes): there is no tolerance anywhere in this file.

Sizes: 1, 63, 64, 65 rows (tile edge, ragged last tile), 4,099 (many tiles, ragged last one), 32,833 (514 tiles against the grid
cap of 512: some workgroups take a second tile, which exercises the register prefetch and the reuse of the staging area).  dX1 / dX2
have guard rows of NaN behind row N, which must come back untouched; every call is made twice and must give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()
SHAPES = [(64, 128), (128, 64), (64, 64)]            # (M, K) = (out features, in features)
SIZES = [1, 63, 64, 65, 4099, 32833]
MGV_OK, MGV_EINVAL, MGV_EUNSUPPORTED = 0, -1, -2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _hip():
    from deepgate import _hip
    return _hip


def _bits(t):
    return t.detach().contiguous().view(I32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _guarded(n, w, dev):
    """[n + GUARD][w] of NaN; the first n rows are the output."""
    return torch.full((n + GUARD, w), NAN, dtype=F32, device=dev)


def _guard_intact(t, n):
    return bool((t[n:].view(I32) == NANBITS).all())


def _rc(name, *args):
    """The entry's return code itself (deepgate._hip.call raises on anything but MGV_OK)."""
    h = _hip()
    return int(getattr(h.load(), name)(*args, h.stream()))


def _tpack(Wv, dev):
    """Transposed fragment-order pack of the [M x Kx] view Wv (rows M, leading dimension Wv.stride(0)): the [Kx x M] operand."""
    h = _hip()
    M, Kx = Wv.shape
    pack = torch.empty(2 * M * Kx, dtype=BF16, device=dev)
    base = pack.data_ptr()
    h.call('mgv_wpack_bf16x3', h.ptr(Wv), Kx, M, Wv.stride(0), 1, h.ctypes.c_void_p(base), h.ctypes.c_void_p(base + 2 * M * Kx))
    return pack


def _inputs(M, K, N, dev, seed):
    """randn rows; X1 | X2 are two 64-column tensors at K = 128, one tensor otherwise; dY also as columns 4 .. 4 + M of a wider matrix."""
    g = torch.Generator().manual_seed(seed)
    K1 = 64
    d = {'K1': K1, 'K2': K - K1}
    d['X1'] = torch.randn(N, K1, generator=g).to(dev)
    d['X2'] = torch.randn(N, K - K1, generator=g).to(dev) if K > K1 else None
    d['dY'] = torch.randn(N, M, generator=g).to(dev)
    wide = torch.full((N, M + 8), NAN, dtype=F32, device=dev)
    wide[:, 4:4 + M] = d['dY']
    d['dY_wide'] = wide[:, 4:4 + M]
    d['W'] = (torch.randn(M, K, generator=g) / K ** 0.5).to(dev)
    d['R'] = torch.randn(N, K1, generator=g).to(dev)
    d['dW0'] = torch.randn(M, K, generator=g).to(dev)         # dW and db accumulate: both routes start from the same contents
    d['db0'] = torch.randn(M, generator=g).to(dev)
    return d


def _xargs(d):
    h = _hip()
    X2 = d['X2']
    return (h.ptr(d['X1']), d['K1'], d['X1'].stride(0), h.ptr(X2), d['K2'], 0 if X2 is None else X2.stride(0))


def _separate(M, K, N, d, with_db, with_res, strided, dev):
    """The launches the fused entry replaces: one weight gradient, one input gradient per column block."""
    h = _hip()
    p = h.ptr
    dY = d['dY_wide'] if strided else d['dY']
    dW, db = d['dW0'].clone(), d['db0'].clone() if with_db else None
    nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
    ws = torch.empty(max(nws, 1), dtype=F32, device=dev)
    h.call('mgv_linear_wgrad_x3', N, *_xargs(d), p(dY), dY.stride(0), M, p(dW), p(db), p(ws), nws)
    K1, K2 = d['K1'], d['K2']
    dX1, dX2 = _guarded(N, K1, dev), _guarded(N, K2, dev) if K2 else None
    pack1 = _tpack(d['W'][:, :K1], dev)
    if with_res:
        h.call('mgv_linear_fwd_x3_res', N, p(dY), M, dY.stride(0), None, 0, 0, p(pack1), None, K1, p(d['R']), d['R'].stride(0), p(dX1), K1)
    else:
        h.call('mgv_linear_fwd_x3', N, p(dY), M, dY.stride(0), None, 0, 0, p(pack1), None, K1, p(dX1), K1)
    if K2:
        h.call('mgv_linear_fwd_x3', N, p(dY), M, dY.stride(0), None, 0, 0, p(_tpack(d['W'][:, K1:], dev)), None, K2, p(dX2), K2)
    return {'dW': dW, 'db': db, 'dX1': dX1, 'dX2': dX2}


def _fused_args(M, K, N, d, out, with_res, strided, ws, nws):
    p = _hip().ptr
    dY = d['dY_wide'] if strided else d['dY']
    R = d['R'] if with_res else None
    return (N, *_xargs(d), p(dY), dY.stride(0), M, p(d['wt']), p(out['dW']), p(out['db']), p(out['dX1']), d['K1'],
            p(out['dX2']), d['K2'], p(R), 0 if R is None else R.stride(0), p(ws), nws)


def _fused(M, K, N, d, with_db, with_res, strided, dev):
    h = _hip()
    out = {'dW': d['dW0'].clone(), 'db': d['db0'].clone() if with_db else None,
           'dX1': _guarded(N, d['K1'], dev), 'dX2': _guarded(N, d['K2'], dev) if d['K2'] else None}
    nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
    ws = torch.full((nws + GUARD,), NAN, dtype=F32, device=dev)
    h.call('mgv_linear_bwd_x3', *_fused_args(M, K, N, d, out, with_res, strided, ws, nws))
    assert bool((ws[nws:].view(I32) == NANBITS).all()), 'workspace overrun'
    return out


def _variants(M, K):
    """(db, residual, dY as a column slice)"""
    if (M, K) == (128, 64):
        return [(True, False, False), (False, True, False), (True, True, True), (False, False, True)]
    return [(True, False, False), (False, True, False)]


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('M,K', SHAPES)
def test_fused_backward_equals_separate_launches_bit_for_bit(M, K, N):
    dev = _dev()
    h = _hip()
    assert h.call_value('mgv_linear_bwd_x3_supported', M, K) == 1
    d = _inputs(M, K, N, dev, seed=1000 * M + K + N)
    d['wt'] = _tpack(d['W'], dev)
    for with_db, with_res, strided in _variants(M, K):
        tag = '(%d, %d) N=%d db=%s res=%s strided=%s' % (M, K, N, with_db, with_res, strided)
        ref = _separate(M, K, N, d, with_db, with_res, strided, dev)
        got = _fused(M, K, N, d, with_db, with_res, strided, dev)
        again = _fused(M, K, N, d, with_db, with_res, strided, dev)
        torch.cuda.synchronize()
        for k in ('dW', 'db', 'dX1', 'dX2'):
            if ref[k] is None:
                assert got[k] is None
                continue
            n = N if k.startswith('dX') else ref[k].shape[0]
            assert bool(torch.isfinite(got[k][:n]).all()), '%s: %s not finite' % (tag, k)
            assert _same(got[k][:n], ref[k][:n]), '%s: %s differs from the separate launches' % (tag, k)
            assert _same(got[k], again[k]), '%s: %s differs between two calls' % (tag, k)
            if k.startswith('dX'):
                assert _guard_intact(got[k], N), '%s: %s written behind row N' % (tag, k)


def test_refusals_launch_nothing():
    dev = _dev()
    h = _hip()
    M, K, N = 64, 64, 130
    d = _inputs(M, K, N, dev, seed=7)
    d['wt'] = _tpack(d['W'], dev)
    nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
    ws = torch.full((nws + GUARD,), NAN, dtype=F32, device=dev)

    def fresh():
        return {'dW': d['dW0'].clone(), 'db': d['db0'].clone(), 'dX1': _guarded(N, 64, dev), 'dX2': None}

    def untouched(out):
        torch.cuda.synchronize()
        return (_same(out['dW'], d['dW0']) and _same(out['db'], d['db0']) and _guard_intact(out['dX1'], 0)
                and bool((ws.view(I32) == NANBITS).all()))

    out = fresh()
    assert _rc('mgv_linear_bwd_x3', *_fused_args(M, K, N, d, out, False, False, ws, nws - 1)) == MGV_EINVAL
    assert untouched(out)
    assert _rc('mgv_linear_bwd_x3', *_fused_args(M, K, N, d, out, False, False, None, nws)) == MGV_EINVAL
    assert untouched(out)
    # shapes the fused entry does not serve (the separate kernels do serve (64, 32) and (32, 64))
    for Mu, K1u in ((32, 64), (64, 32), (32, 32), (16, 64)):
        assert h.call_value('mgv_linear_bwd_x3_supported', Mu, K1u) == 0
        du = dict(d, K1=K1u, K2=0)
        assert _rc('mgv_linear_bwd_x3', *_fused_args(Mu, K1u, N, du, out, False, False, ws, nws)) == MGV_EUNSUPPORTED
        assert untouched(out)
    # X2 and dX2 come together
    bad = dict(fresh(), dX2=_guarded(N, 64, dev))
    assert _rc('mgv_linear_bwd_x3', *_fused_args(M, K, N, d, bad, False, False, ws, nws)) == MGV_EINVAL
    assert _rc('mgv_linear_bwd_x3', *_fused_args(M, K, 0, d, out, False, False, ws, nws)) == MGV_OK
    assert untouched(out)


def _grads(fn, tensors, flag):
    """Gradients of every tensor in `tensors` through fn with ops.FUSED_LINEAR_BWD = flag, and the launcher names that ran."""
    from deepgate import ops
    h = _hip()
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    old_flag, ops.FUSED_LINEAR_BWD = ops.FUSED_LINEAR_BWD, flag
    old = h.profile(True)
    try:
        fn(*leaves).backward()
        names = set(h.profile_summary(h._profile))
    finally:
        h._profile = old
        ops.FUSED_LINEAR_BWD = old_flag
    return [t.grad for t in leaves], names


def test_autograd_path_flag_on_equals_flag_off():
    """ops.linear / ops.linear_passthrough at N = 4,099: every gradient bit-equal with the fused backward on and off, the fused entry
    running exactly when it should (both gradients wanted); a backward that wants one of the two keeps the separate launches."""
    dev = _dev()
    from deepgate import ops
    if ops.PRECISION != 'x3':
        pytest.skip('the fused backward serves the bf16x3 mode')
    N = 4099
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    s, t, hs = rn(N, 64), rn(N, 64), rn(N, 64)
    W_l, b_l, W_d, b_d, W_q = rn(64, 128) / 11, rn(64), rn(128, 64) / 8, rn(128), rn(64, 64) / 8
    c64, c128 = rn(N, 64), rn(N, 128)
    FUSED = 'mgv_linear_bwd_x3'
    cases = {
        # hs_linear: cat fused, two input gradients
        'cat': (lambda a, b, W, bias: (ops.linear(a, W, bias, x2=b) * c64).sum(), [s, t, W_l, b_l], True),
        # hs_decompose: the second consumer's gradient rides in as the residual
        'passthrough': (lambda x, W, bias: (lambda y, xp: (y * c128).sum() + (xp * xp * c64).sum())(*ops.linear_passthrough(x, W, bias)),
                        [hs, W_d, b_d], True),
        'passthrough, only y used': (lambda x, W, bias: (ops.linear_passthrough(x, W, bias)[0] * c128).sum(), [hs, W_d, b_d], True),
        'passthrough, only x used': (lambda x, W, bias: (ops.linear_passthrough(x, W, bias)[1] * c64).sum(), [hs, W_d, b_d], False),
        'square, no bias': (lambda x, W: (ops.linear(x, W) * c64).sum(), [hs, W_q], True),
        # only the weight gradient wanted: the input is no leaf of the graph
        'weights only': (lambda W, bias: (ops.linear(hs, W, bias) * c128).sum(), [W_d, b_d], False),
    }
    for tag, (fn, tensors, fused) in cases.items():
        on, names_on = _grads(fn, tensors, True)
        off, names_off = _grads(fn, tensors, False)
        assert (FUSED in names_on) == fused and FUSED not in names_off, (tag, names_on, names_off)
        for i, (a, b) in enumerate(zip(on, off)):
            if tag == 'passthrough, only x used' and i > 0:
                assert a is None and b is None
                continue
            assert a is not None and b is not None and _same(a, b), '%s: gradient %d differs with the flag' % (tag, i)
