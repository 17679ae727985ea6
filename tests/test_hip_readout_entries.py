"""The readout entries of csrc/readout.hip and csrc/readout_fused_x3.hip (with k_slab_sum of csrc/mgv_slab.h behind them), every entry on
its own through the C ABI against the float64 restatements of tests/readout_ref.py (pinned on the CPU by tests/test_readout_spec.py,
which also asserts the properties of the case builders used here and shows that the defects these tests are there to catch are far
outside their bounds):

  per layer  mgv_colstats, mgv_bn_act_fwd, mgv_bn_act_bwd, mgv_bn_bwd_apply, mgv_readout_head_fwd, mgv_readout_head_bwd   C in {4 .. 64}
  loss       mgv_l1_loss_fwd, mgv_l1_loss_bwd
  fused      mgv_readout_fused_fwd, mgv_readout_fused_bwd (with mgv_wpack_bf16x3 and the size functions mgv_readout_fused_pack_elems,
             mgv_readout_fused_grad_floats, mgv_readout_fused_ws_doubles, mgv_sum_workspace_doubles)

Every output has 64 guard rows behind it (NaN before the call, bit-identical after it); outputs, workspaces, stats and sums are NaN
before the call (grads and dhf too: the header says overwritten); the accumulating outputs (sums of mgv_colstats / mgv_bn_act_bwd, dw /
db of the head, sum of mgv_l1_loss_fwd) start from a0 of their entry's own magnitude and are judged against S + |a0|; mgv_colstats with
ld > C reads a matrix whose foreign columns hold NaN.  Workspaces are sized exactly by the header's size functions.

Bound: err <= tau S entry by entry, tau = 8 max(r, floor), r the worst ratio FOR THAT OUTPUT of the float32 / bf16x3 restatement against
float64 on the same case, computed here; floor 2^-23 (float32 work), 2^-17 (a bf16x3 product behind the entry), 2^-53 x the longest chain
of additions for mgv_colstats' double sums (readout_ref.FLOOR, chain_len).  Nothing is taken from what the device returns.

The fused forward is CHAINED: y1 is held to the reference from hf; stats1 / rm1 / rv1 to the reference from the device's own y1; y2 to
the reference from the device's y1 and stats1, and so on, so a defect is pinned to its pass.  The fused backward runs from the forward's
own y1 / y2 / stats and from designed ones no forward produced.  Decisions (ReLU, clamp) are the float64 run's own everywhere outside
readout_ref.BAND, asserted exactly; inside the band the device's branch is taken: the ReLU branch from mgv_bn_act_fwd on the same y and
stats (the fused kernels form bn as k_bn_act_fwd does), the clamp branch from prob.  Every call is repeated with other workspace garbage
(1e30 for NaN) and must return identical bits.

Every check prints one line `RO <entry> <case> | <output> ratio/tau | ...`; the worst per entry is in NOTEBOOK.md."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readout_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
GUARD = 64
NAN = float('nan')
EINVAL = -1
C, D = RR.CF, RR.D
LAYER_FLOOR = {'sums': 'f32', 'dZ': 'f32', 'A': 'f32', 'dY': 'f32', 'prob': 'f32', 'dA': 'f32', 'dw': 'f32', 'db': 'f32', 'dx': 'f32', 'sum': 'f32'}


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


def _p(t):
    return _hip().ptr(t.v if isinstance(t, Buf) else t)


# ------------------------------------------------------------------------------------------------ buffers
class Buf:
    """A contiguous output of `shape` with GUARD rows behind it: NaN everywhere before the call, or `fill` in its own part."""

    def __init__(self, shape, dev, dtype=F32, fill=None):
        shape = tuple(shape)
        n, w = shape[0], 1
        for s in shape[1:]:
            w *= s
        self.parent = torch.full((n + GUARD, w), NAN, dtype=dtype, device=dev)
        self.v = self.parent[:n].view(shape)
        self.n = n
        if fill is not None:
            if torch.is_tensor(fill):
                self.v.copy_(fill.to(dtype))
            else:
                self.v.fill_(fill)
        self.before = self._bits(self.parent).clone()

    @staticmethod
    def _bits(t):
        return t.view(I32 if t.dtype == F32 else I64)

    def intact(self):
        """The guard rows bit-identical to what they held."""
        return bool((self._bits(self.parent)[self.n:] == self.before[self.n:]).all())

    def untouched(self):
        return bool((self._bits(self.parent) == self.before).all())

    def cpu(self):
        return self.v.detach().cpu()

    def bits(self):
        return self._bits(self.v.contiguous()).cpu()


def _a0(S, seed, dtype):
    """Accumulator contents of each entry's own magnitude (standard normal where nothing contributes)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(S.shape, generator=g, dtype=F64) * 2 - 1
    return torch.where(S > 0, S * u, torch.randn(S.shape, generator=g, dtype=F64)).to(dtype)


def _compare(entry, tag, got, r64, tau, a0=None):
    """Ratio err / S per output against tau; an accumulator is judged against S + |a0|.  Prints, then returns the failures."""
    a0 = a0 or {}
    line, bad = [], []
    for k, val in got.items():
        val = val.detach().cpu().to(F64).reshape(r64[k].shape)
        S = r64['S'][k] + (a0[k].to(F64).abs().reshape(r64['S'][k].shape) if k in a0 else 0)
        r = RR.ratio(val, r64[k], S)
        line.append('%s %.2g/%.2g' % (k, r, tau[k]))
        if not r <= tau[k]:
            bad.append('%s %s %s: %.3g of its scale, bound %.3g' % (entry, tag, k, r, tau[k]))
    print('RO %s %s | %s' % (entry, tag, ' | '.join(line)))
    return bad


def _sum_ws(dev, garbage=NAN):
    n = _hip().call_value('mgv_sum_workspace_doubles')
    return Buf((n,), dev, F64, fill=garbage), n


# ------------------------------------------------------------------------------------------------ the per-layer entries
LAYER_CASES = [(Cw, N) for Cw in RR.WIDTHS for N in RR.layer_sizes(Cw)]


@functools.lru_cache(maxsize=1)
def _layer(Cw, N):
    return RR.layer_case(Cw, N), RR.head_case(Cw, N)


def _twice(run):
    """run(workspace garbage) -> {name: Buf}; the second call, with other garbage in the workspace, must give identical bits."""
    a, b = run(NAN), run(1e30)
    for k in a:
        assert torch.equal(a[k].bits(), b[k].bits()), 'repeat call: %s differs' % k
    return a


@pytest.mark.parametrize('Cw,N', LAYER_CASES)
def test_colstats(Cw, N):
    dev, bad = _dev(), []
    c, _ = _layer(Cw, N)
    rows = RR.rows_per_wg(Cw)
    lds = [Cw] + ([Cw + 4, 2 * Cw, 72] if N in (rows + 1, 4099) else [])
    for ld in lds:
        Y = torch.full((N, ld), NAN)
        Y[:, :Cw] = c['Y']
        r64 = RR.colstats(Y, ld, Cw)
        a0 = _a0(r64['S']['sums'], 3, F64)
        r64 = RR.colstats(Y, ld, Cw, a0)
        rk = RR.colstats(Y, ld, Cw, a0, dtype=F32)
        Yd = Y.to(dev)

        def run(garbage):
            sums = Buf((2 * Cw,), dev, F64, fill=a0)
            ws, nws = _sum_ws(dev, garbage)
            _call('mgv_colstats', N, Cw, _p(Yd), ld, _p(sums), _p(ws), nws)
            torch.cuda.synchronize()
            assert sums.intact() and ws.intact()
            return {'sums': sums}
        got = _twice(run)
        bad += _compare('colstats', 'C=%d N=%d ld=%d' % (Cw, N, ld), {'sums': got['sums'].v}, r64, RR.taus(r64, rk, {'sums': 2.0 ** -53 * RR.chain_len('colstats', N, Cw)}), {'sums': a0})
    assert not bad, bad


@pytest.mark.parametrize('Cw,N', LAYER_CASES)
def test_bn_act_fwd_bwd_and_apply(Cw, N):
    dev, bad = _dev(), []
    c, _ = _layer(Cw, N)
    d = {k: c[k].to(dev) for k in ('Y', 'mean', 'invstd', 'gamma', 'beta', 'dA', 'dZ', 'sums')}
    tag = 'C=%d N=%d' % (Cw, N)
    variants = [(c['p'], c['seed'])] + ([(0.0, 2 ** 62 + 11), (0.5, 2 ** 63 + 5)] if N == 4099 else [])
    for p, seed in variants:
        a = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['beta'], p, seed)
        ad = (N, Cw, _p(d['Y']), _p(d['mean']), _p(d['invstd']), _p(d['gamma']), _p(d['beta']), p, seed)
        r64 = RR.bn_act_fwd(*a)
        dec = {'relu': r64['relu']}                                          # the builders leave nothing inside the band
        kept = RR._factors(seed, N, Cw, p, F64) != 0
        A = Buf((N, Cw), dev)
        _call('mgv_bn_act_fwd', *ad, _p(A))
        torch.cuda.synchronize()
        assert A.intact()
        bad += _compare('bn_act_fwd', '%s p=%g' % (tag, p), {'A': A.v}, r64, RR.taus(r64, RR.bn_act_fwd(*a, dtype=F32, dec=dec), LAYER_FLOOR))
        assert torch.equal(A.cpu() != 0, r64['relu'] & kept), 'bn_act_fwd: the zeros are not the mask and the closed gates'
        assert p > 0 or bool(kept.all())

        r64 = RR.bn_act_bwd(*a, c['dA'])
        a0 = _a0(r64['S']['sums'], 5, F64)
        r64 = RR.bn_act_bwd(*a, c['dA'], a0)
        rk = RR.bn_act_bwd(*a, c['dA'], a0, dtype=F32, dec=dec)

        def run(garbage):
            dZ, sums = Buf((N, Cw), dev), Buf((2 * Cw,), dev, F64, fill=a0)
            ws, nws = _sum_ws(dev, garbage)
            _call('mgv_bn_act_bwd', *ad, _p(d['dA']), _p(dZ), _p(sums), _p(ws), nws)
            torch.cuda.synchronize()
            assert dZ.intact() and sums.intact() and ws.intact()
            return {'dZ': dZ, 'sums': sums}
        got = _twice(run)
        bad += _compare('bn_act_bwd', '%s p=%g' % (tag, p), {k: v.v for k, v in got.items()}, r64, RR.taus(r64, rk, LAYER_FLOOR), {'sums': a0})
        assert torch.equal(got['dZ'].cpu() != 0, r64['relu'] & kept & (c['dA'] != 0)), 'bn_act_bwd: the zeros of dZ are not the closed gates'
        dead = [RR.DEAD_COL, Cw + RR.DEAD_COL]
        assert torch.equal(got['sums'].cpu()[dead], a0[dead]), 'the dead column added something to its sums'
    for bs in (0, 1):
        ap = (c['Y'], c['mean'], c['invstd'], c['gamma'], c['dZ'], c['sums'], bs)
        r64, rk = RR.bn_bwd_apply(*ap), RR.bn_bwd_apply(*ap, dtype=F32)
        dY = Buf((N, Cw), dev)
        _call('mgv_bn_bwd_apply', N, Cw, _p(d['Y']), _p(d['mean']), _p(d['invstd']), _p(d['gamma']), _p(d['dZ']), _p(d['sums']), bs, _p(dY))
        torch.cuda.synchronize()
        assert dY.intact()
        bad += _compare('bn_bwd_apply', '%s batch_stats=%d' % (tag, bs), {'dY': dY.v}, r64, RR.taus(r64, rk, LAYER_FLOOR))
        assert bool((dY.cpu()[:, RR.ZERO_GAMMA_COL] == 0).all())
    assert not bad, bad


@pytest.mark.parametrize('Cw,N', LAYER_CASES)
def test_head_fwd_and_bwd(Cw, N):
    dev, bad = _dev(), []
    _, h = _layer(Cw, N)
    d = {k: h[k].to(dev) for k in ('A', 'w', 'b', 'dprob')}
    for clamp01 in (0, 1):
        tag = 'C=%d N=%d clamp01=%d' % (Cw, N, clamp01)
        a = (h['A'], h['w'], h['b'], clamp01)
        r64 = RR.head_fwd(*a)
        dec = {'inside': r64['inside']}
        prob = Buf((N,), dev)
        _call('mgv_readout_head_fwd', N, Cw, _p(d['A']), _p(d['w']), _p(d['b']), clamp01, _p(prob))
        torch.cuda.synchronize()
        assert prob.intact()
        bad += _compare('head_fwd', tag, {'prob': prob.v}, r64, RR.taus(r64, RR.head_fwd(*a, dtype=F32, dec=dec), LAYER_FLOOR))
        if clamp01:
            pc = prob.cpu()
            assert bool((pc[r64['h'] < 0] == 0).all()) and bool((pc[r64['h'] > 1] == 1).all()), 'head_fwd: a row outside [0, 1] is not clamped'
        r64 = RR.head_bwd(*a, h['dprob'])
        a0 = {'dw': _a0(r64['S']['dw'], 7, F32), 'db': _a0(r64['S']['db'], 8, F32)}
        r64 = RR.head_bwd(*a, h['dprob'], a0['dw'], a0['db'])
        rk = RR.head_bwd(*a, h['dprob'], a0['dw'], a0['db'], dtype=F32, dec=dec)

        def run(garbage):
            dA, dw, db = Buf((N, Cw), dev), Buf((Cw,), dev, fill=a0['dw']), Buf((1,), dev, fill=a0['db'])
            ws, nws = _sum_ws(dev, garbage)
            _call('mgv_readout_head_bwd', N, Cw, _p(d['A']), _p(d['w']), _p(d['b']), clamp01, _p(d['dprob']), _p(dA), _p(dw), _p(db), _p(ws), nws)
            torch.cuda.synchronize()
            assert dA.intact() and dw.intact() and db.intact() and ws.intact()
            return {'dA': dA, 'dw': dw, 'db': db}
        got = _twice(run)
        bad += _compare('head_bwd', tag, {k: v.v for k, v in got.items()}, r64, RR.taus(r64, rk, LAYER_FLOOR), a0)
        open_rows = (r64['inside'] if clamp01 else torch.ones(N, dtype=torch.bool)) & (h['dprob'] != 0)
        assert torch.equal((got['dA'].cpu() != 0).any(1), open_rows & bool((h['w'] != 0).any())), 'head_bwd: the zero rows of dA are not the clamped rows'
    assert not bad, bad


@pytest.mark.parametrize('gscale', [1.0, -0.37])
@pytest.mark.parametrize('n', RR.L1_SIZES)
def test_l1_loss(n, gscale):
    dev, bad = _dev(), []
    c = RR.l1_case(n)
    x, t, g = c['x'].to(dev), c['t'].to(dev), torch.tensor([gscale], dtype=F32, device=dev)
    r64 = RR.l1_fwd(c['x'], c['t'])
    a0 = _a0(r64['S']['sum'], 9, F64)
    r64, rk = RR.l1_fwd(c['x'], c['t'], a0), RR.l1_fwd(c['x'], c['t'], a0, dtype=F32)

    def run(garbage):
        s = Buf((1,), dev, F64, fill=a0)
        ws, nws = _sum_ws(dev, garbage)
        _call('mgv_l1_loss_fwd', n, _p(x), _p(t), _p(s), _p(ws), nws)
        torch.cuda.synchronize()
        assert s.intact() and ws.intact()
        return {'sum': s}
    got = _twice(run)
    bad += _compare('l1_loss_fwd', 'n=%d' % n, {'sum': got['sum'].v}, r64, RR.taus(r64, rk, LAYER_FLOOR), {'sum': a0})
    r64, rk = RR.l1_bwd(c['x'], c['t'], gscale), RR.l1_bwd(c['x'], c['t'], gscale, dtype=F32)
    dx = Buf((n,), dev)
    _call('mgv_l1_loss_bwd', n, _p(x), _p(t), _p(g), _p(dx))
    torch.cuda.synchronize()
    assert dx.intact()
    bad += _compare('l1_loss_bwd', 'n=%d gscale=%g' % (n, gscale), {'dx': dx.v}, r64, RR.taus(r64, rk, LAYER_FLOOR))
    dc = dx.cpu()
    assert bool((dc[c['tie']] == 0).all()) and torch.equal(torch.sign(dc).to(F64), torch.sign(r64['dx'])), 'l1_loss_bwd: a sign or a tie is wrong'
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the fused entries
OPTS = {'A': {}, 'B': dict(clamp01=0, p=(0.0, 0.0), seeds=(77, 78)), 'S': dict(p=(0.5, 0.2), seeds=(2 ** 62 + 5, 2 ** 63 + 7)),
        'D': dict(momentum=0.3, keep=0.6, eps=1e-3)}
# every N once as the product runs it; every option on either side of the cap of the row kernels and of the forward tiles
FUSED_CASES = [(N, 'A') for N in RR.FUSED_SIZES] + [(N, o) for o in ('B', 'S', 'D') for N in (1024 * RR.TILE, 1024 * RR.TILE + 1)] + [(1, 'D'), (129, 'B')]
TENSORS = ('hf', 'W1', 'b1', 'g1', 'be1', 'W2', 'b2', 'g2', 'be2', 'w3', 'b3', 'dprob')


def _pack(c, dev):
    """[W1][W2][W2^T][W1^T], each hi / lo in fragment order, through mgv_wpack_bf16x3 (held to dense_ref.wpack bit for bit)."""
    h = _hip()
    n = h.call_value('mgv_readout_fused_pack_elems')
    pack = torch.full((n + GUARD,), NAN, dtype=torch.bfloat16, device=dev)
    off = 0
    for W, tr in ((c['W1'], 0), (c['W2'], 0), (c['W2'], 1), (c['W1'], 1)):
        Wd = W.to(dev).contiguous()
        R, K = (W.shape[1], W.shape[0]) if tr else W.shape
        m = W.numel()
        _call('mgv_wpack_bf16x3', h.ptr(Wd), R, K, Wd.stride(0), tr, h.ptr(pack[off:off + m]), h.ptr(pack[off + m:off + 2 * m]))
        torch.cuda.synchronize()
        hi, lo = RR.wpack(W, bool(tr))
        assert torch.equal(pack[off:off + m].view(torch.int16).cpu(), hi) and torch.equal(pack[off + m:off + 2 * m].view(torch.int16).cpu(), lo)
        off += 2 * m
    assert off == n and bool(torch.isnan(pack[n:]).all())
    return pack


def _dev_gates(N, y, stats, gamma, beta, dev):
    """bn > 0 as the device decides it: mgv_bn_act_fwd without dropout on the same y and statistics."""
    A = Buf((N, C), dev)
    _call('mgv_bn_act_fwd', N, C, _p(y), _p(stats[:C]), _p(stats[C:]), _p(gamma), _p(beta), 0.0, 0, _p(A))
    torch.cuda.synchronize()
    return A.cpu() > 0


def _fused_fwd(c, d, pack, N, nws, dev, garbage):
    o = {'y1': Buf((N, C), dev), 'y2': Buf((N, C), dev), 'stats': Buf((4 * C,), dev), 'sums': Buf((4 * C,), dev, F64), 'prob': Buf((N,), dev),
         'ws': Buf((nws,), dev, F64, fill=garbage)}
    for k in ('rm1', 'rv1', 'rm2', 'rv2'):
        o[k] = Buf((C,), dev, fill=c[k])
    _call('mgv_readout_fused_fwd', N, _p(d['hf']), _hip().ptr(pack), _p(d['b1']), _p(d['g1']), _p(d['be1']), _p(o['rm1']), _p(o['rv1']), _p(d['b2']),
          _p(d['g2']), _p(d['be2']), _p(o['rm2']), _p(o['rv2']), _p(d['w3']), _p(d['b3']), c['p1'], c['p2'], c['seed1'], c['seed2'], c['momentum'],
          c['keep'], c['eps'], c['clamp01'], _p(o['y1']), _p(o['y2']), _p(o['stats']), _p(o['sums']), _p(o['prob']), _p(o['ws']), nws)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), 'the fused forward wrote behind %s' % k
    return o


def _fused_bwd(c, d, pack, N, nws, dev, y1, y2, stats, garbage):
    ng = _hip().call_value('mgv_readout_fused_grad_floats')
    assert ng == sum(n for _, n in RR.GRAD_BLOCKS)
    o = {'dhf': Buf((N, D), dev), 'grads': Buf((ng,), dev), 'sums': Buf((4 * C,), dev, F64), 'ws': Buf((nws,), dev, F64, fill=garbage)}
    _call('mgv_readout_fused_bwd', N, _p(d['hf']), _p(y1), _p(y2), _p(stats), _p(d['dprob']), _hip().ptr(pack), _p(d['g1']), _p(d['be1']), _p(d['g2']),
          _p(d['be2']), _p(d['w3']), _p(d['b3']), c['p1'], c['p2'], c['seed1'], c['seed2'], c['clamp01'], _p(o['dhf']), _p(o['grads']), _p(o['sums']),
          _p(o['ws']), nws)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), 'the fused backward wrote behind %s' % k
    return o


def _split_grads(g):
    out, off = {}, 0
    for k, n in RR.GRAD_BLOCKS:
        out[k] = g[off:off + n]
        off += n
    return out


def _check_bwd(entry, tag, c, o, y1, y2, stats, dec):
    b = RR.fused_bwd(c, y1, y2, stats, c['dprob'], dec=dec)
    kb = RR.fused_bwd(c, y1, y2, stats, c['dprob'], dtype=F32, mm='x3', dec=dec or {q: b[q] for q in ('relu1', 'relu2', 'inside')})
    got = dict(_split_grads(o['grads'].cpu()), dhf=o['dhf'].v)
    bad = _compare(entry, tag, got, b, RR.taus(b, kb, RR.BWD_FLOOR))
    for k in (1, 2):          # the designed zeros, exactly
        for name in ('dgamma%d' % k, 'dbeta%d' % k):
            assert float(got[name][RR.DEAD_COL]) == 0, '%s of the dead column' % name
        assert float(got['dW%d' % k].view(C, -1)[RR.ZERO_GAMMA_COL].abs().max()) == 0, 'dW%d row of the zero-gamma column' % k
    assert float(got['dW2'].view(C, C)[:, RR.DEAD_COL].abs().max()) == 0, 'dW2 column of the dead unit'
    return bad


@pytest.mark.parametrize('N,opt', FUSED_CASES)
def test_fused_readout_stage_by_stage(N, opt):
    dev, bad = _dev(), []
    h = _hip()
    c = RR.fused_case(N, **OPTS[opt])
    d = {k: c[k].to(dev) for k in TENSORS}
    pack = _pack(c, dev)
    nws = h.call_value('mgv_readout_fused_ws_doubles', N)
    assert nws == RR.ws_doubles(N)
    tag = 'N=%d %s' % (N, opt)

    o = _fused_fwd(c, d, pack, N, nws, dev, NAN)
    given = {'y1': o['y1'].cpu(), 'stats1': o['stats'].cpu()[:2 * C], 'y2': o['y2'].cpu(), 'stats2': o['stats'].cpu()[2 * C:]}
    assert all(bool(torch.isfinite(v).all()) for v in given.values()), 'the forward left NaN in y1, y2 or stats'
    r = RR.fused_fwd_stages(c, given=given)
    # decisions: the float64 run's own outside the band (asserted), the device's inside it
    gates = {1: _dev_gates(N, o['y1'].v, o['stats'].v[:2 * C], d['g1'], d['be1'], dev), 2: _dev_gates(N, o['y2'].v, o['stats'].v[2 * C:], d['g2'], d['be2'], dev)}
    dec, nband = {}, {}
    for k in (1, 2):
        band = RR.banded(r['bn%d' % k]) & (c['g%d' % k] != 0)[None, :]
        nband['relu%d' % k] = int(band.sum())
        assert torch.equal(gates[k][~band], r['relu%d' % k][~band]), 'layer %d: a ReLU decision outside the band differs' % k
        dec['relu%d' % k] = torch.where(band, gates[k], r['relu%d' % k])
    pc = o['prob'].cpu()
    if c['clamp01']:
        band = RR.banded(r['h'], (0.0, 1.0))
        nband['clamp'] = int(band.sum())
        out_lo, out_hi = (r['h'] < 0) & ~band, (r['h'] > 1) & ~band
        assert bool((pc[out_lo] == 0).all()) and bool((pc[out_hi] == 1).all()), 'a row outside [0, 1] is not clamped'
        dec['inside'] = torch.where(band, (pc > 0) & (pc < 1), r['inside'])
    if any(not torch.equal(dec[k], r[k]) for k in dec):
        r = RR.fused_fwd_stages(c, given=given, dec=dec)
    rk = RR.fused_fwd_stages(c, given=given, dtype=F32, mm='x3', dec=dec)
    got = {'y1': o['y1'].v, 'stats1': given['stats1'], 'rm1': o['rm1'].v, 'rv1': o['rv1'].v, 'y2': o['y2'].v, 'stats2': given['stats2'], 'rm2': o['rm2'].v,
           'rv2': o['rv2'].v, 'prob': o['prob'].v}
    print('RO fused %s banded %s' % (tag, nband))
    bad += _compare('fused_fwd', tag, got, r, RR.taus(r, rk, RR.FWD_FLOOR))
    for k in (1, 2):
        assert bool((given['y%d' % k][:, RR.CONST_COL] == given['y%d' % k][0, RR.CONST_COL]).all()), 'the constant column of y%d is not constant' % k

    # backward from the forward's own y1 / y2 / stats
    ob = _fused_bwd(c, d, pack, N, nws, dev, o['y1'].v, o['y2'].v, o['stats'].v, NAN)
    bad += _check_bwd('fused_bwd', tag, c, ob, given['y1'], given['y2'], o['stats'].cpu(), dec)

    # the same two calls again with other garbage in the workspace: identical bits
    o2 = _fused_fwd(c, d, pack, N, nws, dev, 1e30)
    for k in ('y1', 'y2', 'stats', 'prob', 'rm1', 'rv1', 'rm2', 'rv2'):
        assert torch.equal(o[k].bits(), o2[k].bits()), 'repeat forward: %s differs' % k
    ob2 = _fused_bwd(c, d, pack, N, nws, dev, o2['y1'].v, o2['y2'].v, o2['stats'].v, 1e30)
    for k in ('dhf', 'grads'):
        assert torch.equal(ob[k].bits(), ob2[k].bits()), 'repeat backward: %s differs' % k

    # backward from designed y1 / y2 / stats no forward produced (nothing inside the band: tests/test_readout_spec.py)
    y1, y2, st = RR.designed_bwd_inputs(c)
    od = _fused_bwd(c, d, pack, N, nws, dev, y1.to(dev), y2.to(dev), st.to(dev), NAN)
    bad += _check_bwd('fused_bwd designed', tag, c, od, y1, y2, st, None)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_output_untouched():
    """Every refusal is MGV_EINVAL from the argument check, before any launch and with every output still holding its pre-fill; N = 0 is
    success with nothing written for the per-layer entries and a refusal for the fused ones."""
    dev = _dev()
    h = _hip()
    N, Cw = 40, 32
    c, hd = RR.layer_case(Cw, N), RR.head_case(Cw, N)
    d = {k: c[k].to(dev) for k in ('Y', 'mean', 'invstd', 'gamma', 'beta', 'dA', 'dZ', 'sums')}
    d.update({k: hd[k].to(dev) for k in ('A', 'w', 'b', 'dprob')})
    wide = torch.zeros(N, 128, device=dev)
    bufs = {}

    def fresh():
        bufs.clear()
        bufs.update(o=Buf((N, 128), dev), sums=Buf((256,), dev, F64, fill=1.5), dw=Buf((128,), dev, fill=2.5), db=Buf((1,), dev, fill=3.5),
                    prob=Buf((N,), dev), ws=Buf((h.call_value('mgv_sum_workspace_doubles'),), dev, F64))
        return bufs

    def entries(N=N, Cw=Cw, ld=Cw, p=0.2, nws=None, null=None):
        b = fresh()
        nws = h.call_value('mgv_sum_workspace_doubles') if nws is None else nws
        q = lambda name, t: None if null == name else _p(t)       # noqa: E731
        bn = (_p(wide), _p(d['mean']), _p(d['invstd']), _p(d['gamma']), q('beta', d['beta']))
        return {
            'mgv_colstats': (N, Cw, q('Y', wide), ld, q('sums', b['sums']), _p(b['ws']), nws),
            'mgv_bn_act_fwd': (N, Cw) + bn + (p, 7, q('out', b['o'])),
            'mgv_bn_act_bwd': (N, Cw) + bn + (p, 7, _p(wide), q('out', b['o']), q('sums', b['sums']), _p(b['ws']), nws),
            'mgv_bn_bwd_apply': (N, Cw, _p(wide), _p(d['mean']), _p(d['invstd']), _p(d['gamma']), _p(wide), q('sums', d['sums']), 1, q('out', b['o'])),
            'mgv_readout_head_fwd': (N, Cw, q('Y', wide), _p(d['w']), _p(d['b']), 1, q('out', b['prob'])),
            'mgv_readout_head_bwd': (N, Cw, _p(wide), _p(d['w']), _p(d['b']), 1, _p(d['dprob']), q('out', b['o']), q('sums', b['dw']), _p(b['db']), _p(b['ws']), nws),
        }

    def refused(name, args, want=EINVAL):
        rc = _rc(name, *args)
        torch.cuda.synchronize()
        assert rc == want, (name, rc)
        assert all(b.untouched() for b in bufs.values()), '%s wrote something although it returned %d' % (name, rc)

    rows = RR.rows_per_wg(Cw)
    short = {'mgv_colstats': 2 * (2 * Cw) - 1, 'mgv_bn_act_bwd': 2 * (2 * Cw) - 1, 'mgv_readout_head_bwd': 2 * (Cw + 1) - 1}      # N = 40: two workgroups
    assert -(-N // rows) == 2
    for name in entries():
        for bad_c in (12, 128):
            refused(name, entries(Cw=bad_c, ld=max(bad_c, 4))[name])
        refused(name, entries(N=-1)[name])
        refused(name, entries(N=0)[name], 0)                                  # success, nothing written
        refused(name, entries(null='out' if name != 'mgv_colstats' else 'Y')[name])
        if name in short:
            refused(name, entries(nws=short[name])[name])
            refused(name, entries(null='sums')[name])
    for ld in (Cw - 4, Cw + 2, Cw + 1):
        refused('mgv_colstats', entries(ld=ld)['mgv_colstats'])
    for p in (1.0, -0.1):
        for name in ('mgv_bn_act_fwd', 'mgv_bn_act_bwd'):
            refused(name, entries(p=p)[name])
    refused('mgv_bn_act_fwd', entries(null='beta')['mgv_bn_act_fwd'])

    # the L1 loss
    x = torch.rand(N, device=dev)
    g = torch.ones(1, device=dev)
    b = fresh()
    refused('mgv_l1_loss_fwd', (-1, _p(x), _p(x), _p(b['sums']), _p(b['ws']), 8))
    refused('mgv_l1_loss_fwd', (0, _p(x), _p(x), _p(b['sums']), _p(b['ws']), 8), 0)
    refused('mgv_l1_loss_fwd', (N, _p(x), _p(x), _p(b['sums']), _p(b['ws']), 0))            # one workgroup needs one double
    refused('mgv_l1_loss_fwd', (N, None, _p(x), _p(b['sums']), _p(b['ws']), 8))
    refused('mgv_l1_loss_fwd', (N, _p(x), _p(x), None, _p(b['ws']), 8))
    refused('mgv_l1_loss_bwd', (-1, _p(x), _p(x), _p(g), _p(b['prob'])))
    refused('mgv_l1_loss_bwd', (0, _p(x), _p(x), _p(g), _p(b['prob'])), 0)
    refused('mgv_l1_loss_bwd', (N, _p(x), _p(x), None, _p(b['prob'])))
    refused('mgv_l1_loss_bwd', (N, _p(x), _p(x), _p(g), None))

    # the fused entries
    c = RR.fused_case(N)
    f = {k: c[k].to(dev) for k in TENSORS}
    pack = _pack(c, dev)
    nws = h.call_value('mgv_readout_fused_ws_doubles', N)
    y1, y2, st = (t.to(dev) for t in RR.designed_bwd_inputs(c))

    def fused(N=N, p1=0.2, p2=0.5, nws=nws, null=None):
        bufs.clear()
        bufs.update({k: Buf((N if N > 0 else 1, C), dev) for k in ('y1', 'y2')})
        bufs.update(stats=Buf((4 * C,), dev), sums=Buf((4 * C,), dev, F64), prob=Buf((max(N, 1),), dev), ws=Buf((max(nws, 1),), dev, F64), dhf=Buf((max(N, 1), D), dev),
                    grads=Buf((3297,), dev, fill=4.5))
        bufs.update({k: Buf((C,), dev, fill=c[k]) for k in ('rm1', 'rv1', 'rm2', 'rv2')})
        b = bufs
        q = lambda name, t: None if null == name else (h.ptr(t) if not isinstance(t, Buf) else _p(t))       # noqa: E731
        fw = (N, q('hf', f['hf']), q('pack', pack), _p(f['b1']), _p(f['g1']), _p(f['be1']), q('rm1', b['rm1']), _p(b['rv1']), _p(f['b2']), _p(f['g2']), _p(f['be2']),
              _p(b['rm2']), _p(b['rv2']), _p(f['w3']), q('b3', f['b3']), p1, p2, 1, 2, 0.1, 0.9, 1e-5, 1, q('y1', b['y1']), _p(b['y2']), q('stats', b['stats']),
              q('sums', b['sums']), q('prob', b['prob']), q('ws', b['ws']), nws)
        bw = (N, q('hf', f['hf']), q('y1', y1), _p(y2), q('stats', st), _p(f['dprob']), q('pack', pack), _p(f['g1']), _p(f['be1']), _p(f['g2']), _p(f['be2']),
              _p(f['w3']), q('b3', f['b3']), p1, p2, 1, 2, 1, q('dhf', b['dhf']), q('grads', b['grads']), q('sums', b['sums']), q('ws', b['ws']), nws)
        return {'mgv_readout_fused_fwd': fw, 'mgv_readout_fused_bwd': bw}

    for name in ('mgv_readout_fused_fwd', 'mgv_readout_fused_bwd'):
        for kw in (dict(N=0), dict(N=-1), dict(p1=1.0), dict(p1=-0.1), dict(p2=1.0), dict(p2=-0.1), dict(nws=nws - 1), dict(null='hf'), dict(null='pack'),
                   dict(null='b3'), dict(null='y1'), dict(null='stats'), dict(null='sums'), dict(null='ws')):
            refused(name, fused(**kw)[name])
    refused('mgv_readout_fused_fwd', fused(null='rm1')['mgv_readout_fused_fwd'])
    refused('mgv_readout_fused_fwd', fused(null='prob')['mgv_readout_fused_fwd'])
    refused('mgv_readout_fused_bwd', fused(null='dhf')['mgv_readout_fused_bwd'])
    refused('mgv_readout_fused_bwd', fused(null='grads')['mgv_readout_fused_bwd'])
