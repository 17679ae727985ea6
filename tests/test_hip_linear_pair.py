"""mgv_linear_pair_fwd_x3 / mgv_linear_pair_bwd_x3 (csrc/linear_x3.hip): hs = hs_linear([s|t]) and st = hs_decompose(hs) in one
pass each way, through the C ABI, against the two launches each replaces — mgv_linear_fwd_x3 twice, and mgv_linear_bwd_x3 on
(128, 64) with ghs as its residual followed by mgv_linear_bwd_x3 on (64, 128).  hs, st, ds, dt, dWl and dbl are compared BIT FOR BIT.
dWd and dbd are summed over the pair kernel's own partition of the tiles: each entry is held to a float64 restatement within 1e-4 of
the restatement's largest entry, the bound tests/test_hip_linear_x3.py holds the weight and bias gradients of these kernels to.

Sizes: 1, 63, 64, 65, 129 rows (tile edge, ragged last tile, three tiles) and 4,097 (65 tiles): up to there every workgroup takes ONE
tile (the grid is min(tiles, 512)), so the loop-carried prefetch, the barrier before a workgroup's next tile and the sums carried
from tile to tile are not executed.  32,769 rows (513 tiles: workgroup 0 takes two) and 65,875 (1,030 tiles, the last of 19 rows:
workgroups 0..5 take three, the others two) execute them; the product's batches (from 131,072 rows: four tiles and more per
workgroup) run the same loop.  Against float64 entry by entry: tests/test_hip_linear_pair_reference.py.  s and t are column slices of one
wider matrix; outputs have guard rows of NaN behind row N and the workspace is NaN-filled with a NaN guard behind it; every call is
made twice and must give the same bytes.  Model level: one Trainer.train_step on a small batch with ops.LINEAR_PAIR on and off."""
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, I32, BF16 = torch.float32, torch.float64, torch.int32, torch.bfloat16
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()
SIZES = [1, 63, 64, 65, 129, 4097, 32769, 65875]
WGRAD_TOL = 1e-4            # of the largest entry: tests/test_hip_linear_x3.py
MGV_OK, MGV_EINVAL = 0, -1


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
    return torch.full((n + GUARD, w), NAN, dtype=F32, device=dev)


def _guard_intact(t, n):
    return bool((t[n:].view(I32) == NANBITS).all())


def _rc(name, *args):
    h = _hip()
    return int(getattr(h.load(), name)(*args, h.stream()))


def _pack(W, transpose, dev):
    h = _hip()
    R, K = (W.shape[1], W.shape[0]) if transpose else W.shape
    pack = torch.empty(2 * W.numel(), dtype=BF16, device=dev)
    base = pack.data_ptr()
    h.call('mgv_wpack_bf16x3', h.ptr(W), R, K, W.stride(0), int(transpose), h.ctypes.c_void_p(base), h.ctypes.c_void_p(base + 2 * W.numel()))
    return pack


_INPUTS = {}


def _inputs(N, dev):
    """randn rows; s and t are columns 4 .. 68 and 72 .. 136 of one [N, 144] matrix whose other columns are NaN."""
    if N in _INPUTS:
        return _INPUTS[N]
    g = torch.Generator().manual_seed(4200 + N)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
    wide = torch.full((N, 144), NAN, dtype=F32, device=dev)
    wide[:, 4:68], wide[:, 72:136] = rn(N, 64), rn(N, 64)
    d = {'S': wide[:, 4:68], 'T': wide[:, 72:136], 'Wl': rn(64, 128) / 128 ** 0.5, 'bl': rn(64), 'Wd': rn(128, 64) / 8, 'bd': rn(128),
         'dST': rn(N, 128), 'gHS': rn(N, 64),
         'dWl0': rn(64, 128), 'dbl0': rn(64), 'dWd0': rn(128, 64), 'dbd0': rn(128)}      # the weight gradients accumulate
    d['wl'], d['wd'] = _pack(d['Wl'], False, dev), _pack(d['Wd'], False, dev)
    d['wlt'], d['wdt'] = _pack(d['Wl'], True, dev), _pack(d['Wd'], True, dev)
    _INPUTS[N] = d
    return d


def _two_fwd(N, d, dev):
    h = _hip()
    p = h.ptr
    hs, st = _guarded(N, 64, dev), _guarded(N, 128, dev)
    h.call('mgv_linear_fwd_x3', N, p(d['S']), 64, d['S'].stride(0), p(d['T']), 64, d['T'].stride(0), p(d['wl']), p(d['bl']), 64, p(hs), 64)
    h.call('mgv_linear_fwd_x3', N, p(hs), 64, 64, None, 0, 0, p(d['wd']), p(d['bd']), 128, p(st), 128)
    return hs, st


def _pair_fwd(N, d, dev):
    h = _hip()
    p = h.ptr
    hs, st = _guarded(N, 64, dev), _guarded(N, 128, dev)
    h.call('mgv_linear_pair_fwd_x3', N, p(d['S']), d['S'].stride(0), p(d['T']), d['T'].stride(0), p(d['wl']), p(d['bl']), p(d['wd']), p(d['bd']),
           p(hs), 64, p(st), 128)
    return hs, st


def _fresh(N, d, dev):
    return {'dS': _guarded(N, 64, dev), 'dT': _guarded(N, 64, dev), 'dWl': d['dWl0'].clone(), 'dbl': d['dbl0'].clone(),
            'dWd': d['dWd0'].clone(), 'dbd': d['dbd0'].clone()}


def _two_bwd(N, d, hs, with_ghs, dev):
    h = _hip()
    p = h.ptr
    o = _fresh(N, d, dev)
    dhs = _guarded(N, 64, dev)
    R = d['gHS'] if with_ghs else None
    for M, K in ((128, 64), (64, 128)):
        nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
        ws = torch.full((max(nws, 1),), NAN, dtype=F32, device=dev)
        if M == 128:
            h.call('mgv_linear_bwd_x3', N, p(hs), 64, 64, None, 0, 0, p(d['dST']), 128, 128, p(d['wdt']), p(o['dWd']), p(o['dbd']),
                   p(dhs), 64, None, 0, p(R), 64 if with_ghs else 0, p(ws), nws)
        else:
            h.call('mgv_linear_bwd_x3', N, p(d['S']), 64, d['S'].stride(0), p(d['T']), 64, d['T'].stride(0), p(dhs), 64, 64, p(d['wlt']),
                   p(o['dWl']), p(o['dbl']), p(o['dS']), 64, p(o['dT']), 64, None, 0, p(ws), nws)
    o['dhs'] = dhs
    return o


def _pair_bwd_args(N, d, hs, o, with_ghs, ws, nws):
    p = _hip().ptr
    R = d['gHS'] if with_ghs else None
    return (N, p(d['dST']), 128, p(R), 64 if with_ghs else 0, p(hs), 64, p(d['S']), d['S'].stride(0), p(d['T']), d['T'].stride(0),
            p(d['wlt']), p(d['wdt']), p(o['dS']), 64, p(o['dT']), 64, p(o['dWl']), p(o['dbl']), p(o['dWd']), p(o['dbd']), p(ws), nws)


def _pair_bwd(N, d, hs, with_ghs, dev):
    h = _hip()
    o = _fresh(N, d, dev)
    nws = h.call_value('mgv_linear_pair_bwd_x3_ws_floats', N)
    ws = torch.full((nws + GUARD,), NAN, dtype=F32, device=dev)
    h.call('mgv_linear_pair_bwd_x3', *_pair_bwd_args(N, d, hs, o, with_ghs, ws, nws))
    assert bool((ws[nws:].view(I32) == NANBITS).all()), 'workspace overrun'
    return o


@pytest.mark.parametrize('N', SIZES)
def test_pair_forward_equals_the_two_launches_bit_for_bit(N):
    dev = _dev()
    d = _inputs(N, dev)
    ref, got, again = _two_fwd(N, d, dev), _pair_fwd(N, d, dev), _pair_fwd(N, d, dev)
    torch.cuda.synchronize()
    for k, r, g, a in zip(('hs', 'st'), ref, got, again):
        assert bool(torch.isfinite(g[:N]).all()), '%s not finite at N=%d' % (k, N)
        assert _same(g[:N], r[:N]), '%s differs from the two launches at N=%d' % (k, N)
        assert _same(g, a), '%s differs between two calls at N=%d' % (k, N)
        assert _guard_intact(g, N), '%s written behind row N=%d' % (k, N)


@pytest.mark.parametrize('with_ghs', [False, True])
@pytest.mark.parametrize('N', SIZES)
def test_pair_backward_equals_the_two_launches(N, with_ghs):
    dev = _dev()
    d = _inputs(N, dev)
    hs = _two_fwd(N, d, dev)[0][:N].contiguous()
    ref, got, again = _two_bwd(N, d, hs, with_ghs, dev), _pair_bwd(N, d, hs, with_ghs, dev), _pair_bwd(N, d, hs, with_ghs, dev)
    torch.cuda.synchronize()
    tag = 'N=%d ghs=%s' % (N, with_ghs)
    for k in ('dS', 'dT', 'dWl', 'dbl', 'dWd', 'dbd'):
        n = N if k in ('dS', 'dT') else got[k].shape[0]
        assert bool(torch.isfinite(got[k][:n]).all()), '%s: %s not finite' % (tag, k)
        assert _same(got[k], again[k]), '%s: %s differs between two calls' % (tag, k)
        if k in ('dS', 'dT'):
            assert _guard_intact(got[k], N), '%s: %s written behind row N' % (tag, k)
        if k not in ('dWd', 'dbd'):
            assert _same(got[k][:n], ref[k][:n]), '%s: %s differs from the two launches' % (tag, k)
    # dWd, dbd: each entry against float64, as an increment of the starting contents
    dst64, hs64 = d['dST'].double(), hs.double()
    for k, start, inc in (('dWd', d['dWd0'], dst64.t() @ hs64), ('dbd', d['dbd0'], dst64.sum(0))):
        bound = WGRAD_TOL * float(inc.abs().max())
        err = float((got[k].double() - (start.double() + inc)).abs().max())
        err_two = float((ref[k].double() - (start.double() + inc)).abs().max())
        print('%s %s: worst entry off float64 by %.3e (two launches %.3e), bound %.3e, same bits as the two launches: %s'
              % (tag, k, err, err_two, bound, _same(got[k], ref[k])))
        assert err <= bound, '%s: %s off float64 by %.3e > %.3e' % (tag, k, err, bound)


def test_no_rows_and_short_workspaces_launch_nothing():
    dev = _dev()
    h = _hip()
    N = 130
    d = _inputs(129, dev)
    d = dict(d, dST=torch.randn(N, 128, device=dev), gHS=torch.randn(N, 64, device=dev))
    wide = torch.randn(N, 144, device=dev)
    d['S'], d['T'] = wide[:, 4:68], wide[:, 72:136]
    hs = torch.randn(N, 64, device=dev)
    nws = h.call_value('mgv_linear_pair_bwd_x3_ws_floats', N)
    assert nws == 3 * (64 * 128 + 64 + 128 * 64 + 128) and h.call_value('mgv_linear_pair_bwd_x3_ws_floats', 0) >= 0
    ws = torch.full((nws + GUARD,), NAN, dtype=F32, device=dev)
    o = _fresh(N, d, dev)

    def untouched():
        torch.cuda.synchronize()
        return (all(_same(o[k], d[k + '0']) for k in ('dWl', 'dbl', 'dWd', 'dbd')) and _guard_intact(o['dS'], 0) and _guard_intact(o['dT'], 0)
                and bool((ws.view(I32) == NANBITS).all()))

    assert _rc('mgv_linear_pair_bwd_x3', *_pair_bwd_args(N, d, hs, o, True, ws, nws - 1)) == MGV_EINVAL
    assert untouched()
    assert _rc('mgv_linear_pair_bwd_x3', *_pair_bwd_args(N, d, hs, o, True, None, nws)) == MGV_EINVAL
    assert untouched()
    assert _rc('mgv_linear_pair_bwd_x3', *_pair_bwd_args(0, d, hs, o, True, ws, nws)) == MGV_OK
    assert untouched()
    p = h.ptr
    out_hs, out_st = _guarded(N, 64, dev), _guarded(N, 128, dev)
    assert _rc('mgv_linear_pair_fwd_x3', 0, p(d['S']), 144, p(d['T']), 144, p(d['wl']), p(d['bl']), p(d['wd']), p(d['bd']), p(out_hs), 64, p(out_st), 128) == MGV_OK
    assert _rc('mgv_linear_pair_fwd_x3', N, p(d['S']), 144, p(d['T']), 144, p(d['wl']), p(d['bl']), p(d['wd']), p(d['bd']), p(out_hs), 64, p(out_st), 126) == MGV_EINVAL
    torch.cuda.synchronize()
    assert _guard_intact(out_hs, 0) and _guard_intact(out_st, 0)


def _train_step(pair, dev, monkeypatch):
    """One Trainer.train_step of a fresh H = 64 model on two synthetic AIGs of 304 nodes, ops.LINEAR_PAIR = pair (from the first row
    on); the losses, every parameter gradient, the launcher names, and hs and the gradient that reached st where the pair ran."""
    import deepgate
    from deepgate import _hip, ops, sampling, synthetic as syn
    monkeypatch.setattr(ops, 'LINEAR_PAIR', pair)
    monkeypatch.setattr(ops, 'LINEAR_PAIR_MIN_ROWS', 0)
    monkeypatch.setattr(sampling, '_CALLS', itertools.count())      # the sampled negatives repeat
    torch.manual_seed(31)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=64, s_rounds=2, t_rounds=2, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.to(dev).train()
    graphs = [syn.make_graph('aig', 304, 8, 7300 + i, n_inputs=16) for i in range(2)]
    for g in graphs:
        del g['neg_edge_index']
    batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)
    tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='pair', save_dir='/tmp/mgv_test_exp', lr=1e-4,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=2, distributed=False)
    seam = {}
    real_pair = ops.linear_pair

    def pair_capture(*a):
        hs, st = real_pair(*a)
        seam['hs'] = hs.detach().clone()
        st.register_hook(lambda g: seam.__setitem__('g_st', g.detach().clone()))
        return hs, st
    monkeypatch.setattr(ops, 'linear_pair', pair_capture)
    names = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    ls = tr.train_step(batch)
    torch.cuda.synchronize()
    monkeypatch.setattr(_hip, 'call', real)
    return {'losses': {k: ls[k].detach().clone() for k in ('recon_loss', 'prob_loss', 'func_loss')}, 'names': names, 'seam': seam,
            'grads': {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}}


def test_train_step_with_the_pair_on_and_off(monkeypatch):
    dev = _dev()
    from deepgate import ops
    if ops.PRECISION != 'x3':
        pytest.skip('the pair serves the bf16x3 mode')
    on, off = _train_step(True, dev, monkeypatch), _train_step(False, dev, monkeypatch)
    PAIR = {'mgv_linear_pair_fwd_x3', 'mgv_linear_pair_bwd_x3'}
    assert PAIR <= set(on['names']) and not PAIR & set(off['names'])
    assert on['names'].count('mgv_linear_pair_fwd_x3') == 1 and on['names'].count('mgv_linear_pair_bwd_x3') == 1
    # the four launches of the seam are gone: what is left of these launchers with the pair on serves other layers
    assert off['names'].count('mgv_linear_fwd_x3') - on['names'].count('mgv_linear_fwd_x3') == 2
    assert off['names'].count('mgv_linear_bwd_x3') - on['names'].count('mgv_linear_bwd_x3') == 2
    for k in on['losses']:
        assert _same(on['losses'][k], off['losses'][k]), k
    loose = {'hs_decompose.weight', 'hs_decompose.bias'}
    assert on['grads'].keys() == off['grads'].keys() and loose <= set(on['grads'])
    diff = [k for k in on['grads'] if k not in loose and not _same(on['grads'][k], off['grads'][k])]
    assert not diff, diff
    hs64, g64 = on['seam']['hs'].double(), on['seam']['g_st'].double()
    for k, ref in (('hs_decompose.weight', g64.t() @ hs64), ('hs_decompose.bias', g64.sum(0))):
        bound = WGRAD_TOL * float(ref.abs().max())
        for tag, run in (('pair', on), ('two launches', off)):
            err = float((run['grads'][k].double() - ref).abs().max())
            print('%s, %s: worst entry off float64 by %.3e, bound %.3e' % (k, tag, err, bound))
            assert err <= bound, (k, tag, err, bound)
