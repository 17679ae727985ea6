"""mgv_var_head_fwd_x3 / mgv_var_head_bwd_x3 (csrc/var_head_x3.hip) through the C ABI against the float64 restatement
tests/var_head_ref.py (pinned on the CPU by tests/test_var_head_spec.py, which also shows the planted defects far outside the bounds
used here).

Every output has 64 NaN guard rows behind it; with `wide` the operands are column slices of wider matrices whose other columns hold
NaN (ldst, ldz, ldg, ldeps wider than 2H) and the foreign columns of an output must come back bit-identical; workspaces are NaN-filled
with a guard of their own; the accumulators dWp, dbp start from random a0 of their entry's own magnitude.

Bounds: err <= tau S entry by entry and row by row, tau = 8 max(r, 2^-17), r the worst ratio for that output of the float32 stand-in
in the kernel's arithmetic against float64 on the same inputs — never a device figure; an accumulator entry additionally gets
2^-24 |a0|.  Generated noise is checked on its own, through Z at mu = 0, ls = 0 (zero packs and biases), to losses_ref.GAUSS_FLOOR;
the other comparisons of such a case then use the device's own noise as the given eps of the restatement.
Every check prints one line `VH <entry> <case> | <output> ratio/tau | ...`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as DR  # noqa: E402
import losses_ref as LR  # noqa: E402
import var_head_ref as VR  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, I32 = torch.float64, torch.float32, torch.int32
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()
ACC = ('dWp_s', 'dWp_t', 'dbp_s', 'dbp_t')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _hip():
    from deepgate import _hip
    return _hip


class Out:
    """[n][w] output inside a NaN-filled [n + GUARD][ld] matrix."""

    def __init__(self, n, w, ld, dev):
        self.n, self.w, self.ld = n, w, ld
        self.parent = torch.full((n + GUARD, ld), NAN, dtype=F32, device=dev)
        self.v = self.parent[:n, :w]

    def intact(self):
        bits = self.parent.view(I32)
        mine = torch.zeros_like(bits, dtype=torch.bool)
        mine[:self.n, :self.w] = True
        return bool((bits[~mine] == NANBITS).all())

    def untouched(self):
        return bool((self.parent.view(I32) == NANBITS).all())


def _vec(n, dev, fill=None, dtype=F32):
    t = torch.full((n + GUARD,), NAN, dtype=dtype, device=dev)
    if fill is not None:
        t[:n] = fill.reshape(-1).to(dtype)
    return t


def _guard_ok(t, n):
    return bool(torch.isnan(t[n:]).all())


def _packs(Wp, dev, zero=False):
    """(forward packs, transposed packs) of the two halves through mgv_wpack_bf16x3."""
    h = _hip()
    fw, tr = [], []
    for W in Wp:
        M, K = W.shape
        Wd = (torch.zeros_like(W) if zero else W).to(dev).contiguous()
        for transpose, dst in ((0, fw), (1, tr)):
            p = torch.zeros(2 * M * K, dtype=torch.bfloat16, device=dev)
            R, KK = (K, M) if transpose else (M, K)
            h.call('mgv_wpack_bf16x3', h.ptr(Wd), R, KK, K, transpose, h.ptr(p[:M * K]), h.ptr(p[M * K:]))
            dst.append(p)
    return fw, tr


def _a0(S, seed):
    g = torch.Generator().manual_seed(seed)
    return (S * (torch.rand(S.shape, generator=g, dtype=F64) * 2 - 1)).to(F32)


def run_fwd(c, dev, eps='given', sample=1, ML=True, zero_heads=False, raw=None):
    """-> ({'Z', 'ML', 'kl'} on the device, [what was not left intact]).  raw: a dict of argument overrides for a refused call; the
    return code is then the third result and nothing is compared by the caller but the buffers."""
    h = _hip()
    H, N = c['H'], c['N']
    fw, _ = _packs(c['Wp'], dev, zero=zero_heads)
    bp = [(torch.zeros_like(b) if zero_heads else b).to(dev) for b in c['bp']]
    ST, E = c['ST'].to(dev), c['eps'].to(dev)
    Z, MLo = Out(N, 2 * H, c['ldz'], dev), Out(N, 4 * H, 4 * H + (4 if c['wide'] else 0), dev)
    kl = torch.full((2 + GUARD,), NAN, dtype=F64, device=dev)
    nws = VR.ws_floats(H, N, False)
    ws = _vec(nws, dev)
    a = dict(H=H, N=N, ST=h.ptr(ST), ldst=ST.stride(0), ws_=h.ptr(fw[0]), wt_=h.ptr(fw[1]), bs=h.ptr(bp[0]), bt=h.ptr(bp[1]),
             eps=h.ptr(E) if eps == 'given' else None, ldeps=E.stride(0) if eps == 'given' else 0, seed=c['seed'], sample=sample,
             Z=h.ptr(Z.parent), ldz=Z.ld, ML=h.ptr(MLo.parent) if ML else None, ldml=MLo.ld if ML else 0, kl=h.ptr(kl), ws=h.ptr(ws), nws=nws)
    if raw is not None:
        a.update(raw)
        rc = getattr(h.load(), 'mgv_var_head_fwd_x3')(*a.values(), h.stream())
        torch.cuda.synchronize()
        clean = Z.untouched() and MLo.untouched() and bool(torch.isnan(kl).all()) and bool(torch.isnan(ws).all())
        return rc, clean
    h.call('mgv_var_head_fwd_x3', *a.values())
    torch.cuda.synchronize()
    bad = [n for n, ok in (('Z', Z.intact()), ('ML', MLo.intact() if ML else MLo.untouched()), ('kl', _guard_ok(kl, 2)), ('ws', _guard_ok(ws, nws))) if not ok]
    out = {'Z': Z.v.clone(), 'kl': kl[:2].clone()}
    if ML:
        out['ML'] = MLo.v.clone()
    return out, bad


def run_bwd(c, dev, r64, eps='given', sample=1, gZ=True, gkl=True, raw=None):
    h = _hip()
    H, N = c['H'], c['N']
    fw, tr = _packs(c['Wp'], dev)
    bp = [b.to(dev) for b in c['bp']]
    ST, E, G = c['ST'].to(dev), c['eps'].to(dev), c['gZ'].to(dev)
    gk = torch.tensor(c['gkl'], dtype=F32, device=dev)
    dST = Out(N, 2 * H, 2 * H + (8 if c['wide'] else 0), dev)
    a0 = {k: _a0(r64['S'][k], 5 + i) for i, k in enumerate(ACC)} if r64 is not None else {k: torch.zeros(2 * H * H if 'W' in k else 2 * H) for k in ACC}
    acc = {k: _vec(a0[k].numel(), dev, fill=a0[k]) for k in ACC}
    nws = VR.ws_floats(H, N, True)
    ws = _vec(nws, dev)
    a = dict(H=H, N=N, ST=h.ptr(ST), ldst=ST.stride(0), ws_=h.ptr(fw[0]), wt_=h.ptr(fw[1]), ts_=h.ptr(tr[0]), tt_=h.ptr(tr[1]), bs=h.ptr(bp[0]),
             bt=h.ptr(bp[1]), eps=h.ptr(E) if eps == 'given' else None, ldeps=E.stride(0) if eps == 'given' else 0, seed=c['seed'], sample=sample,
             gZ=h.ptr(G) if gZ else None, ldg=G.stride(0) if gZ else 0, gkl=h.ptr(gk) if gkl else None, dST=h.ptr(dST.parent), lddst=dST.ld,
             dWs=h.ptr(acc['dWp_s']), dWt=h.ptr(acc['dWp_t']), dbs=h.ptr(acc['dbp_s']), dbt=h.ptr(acc['dbp_t']), ws=h.ptr(ws), nws=nws)
    if raw is not None:
        a.update(raw)
        rc = getattr(h.load(), 'mgv_var_head_bwd_x3')(*a.values(), h.stream())
        torch.cuda.synchronize()
        clean = dST.untouched() and bool(torch.isnan(ws).all()) and all(torch.equal(acc[k][:a0[k].numel()].cpu(), a0[k].reshape(-1)) for k in ACC)
        return rc, clean
    h.call('mgv_var_head_bwd_x3', *a.values())
    torch.cuda.synchronize()
    bad = [n for n, ok in [('dST', dST.intact()), ('ws', _guard_ok(ws, nws))] + [(k, _guard_ok(acc[k], a0[k].numel())) for k in ACC] if not ok]
    out = {'dST': dST.v.clone()}
    out.update({k: acc[k][:a0[k].numel()].reshape(a0[k].shape).clone() for k in ACC})
    return out, bad, a0


def _compare(entry, tag, got, r64, tau, a0=None, extra=0.0):
    """Ratio err / S per output (row by row for the row outputs: the worst row is reported) against tau (+ extra)."""
    a0 = a0 or {}
    line, bad = [], []
    for k, val in got.items():
        val = val.detach().cpu().to(F64)
        ref, S = r64[k], r64['S'][k]
        if k in a0:
            b = a0[k].to(F64)
            err = (((val - b) - ref).abs() - DR.U24 * b.abs()).clamp(min=0)
            r = float((err / S.clamp(min=1e-300)).max()) if bool(torch.isfinite(val).all()) else float('inf')
        else:
            r = DR.ratio(val, ref, S)
        line.append('%s %.2g/%.2g' % (k, r, tau[k] + extra))
        if not r <= tau[k] + extra:
            bad.append('%s: %.3g of its scale, bound %.3g' % (k, r, tau[k] + extra))
    print('VH %s %s | %s' % (entry, tag, ' | '.join(line)))
    return ['%s %s: %s' % (entry, tag, b) for b in bad]


def _device_noise(c, dev):
    """The generated noise of a case, read through Z at mu = 0, ls = 0 (exp(0) = 1: Z = eps exactly), checked to GAUSS_FLOOR."""
    out, bad = run_fwd(c, dev, eps='gen', sample=1, ML=False, zero_heads=True)
    assert not bad, bad
    e = out['Z'].cpu()
    want = VR.noise(c['H'], c['N'], c['seed'])
    worst = float((e.to(F64) - want).abs().max())
    print('VH noise H=%d N=%d | worst %.3g / %.3g' % (c['H'], c['N'], worst, LR.GAUSS_FLOOR))
    assert worst <= LR.GAUSS_FLOOR, worst
    assert out['kl'].tolist() == [0.0, 0.0]          # 1 + 0 - 0 - 1 per element
    return e


# (wide, eps, sample, gZ, gkl, ML)
COMBOS = {'A': (False, 'given', 1, True, True, True), 'B': (True, 'gen', 1, True, True, False), 'C': (True, 'given', 0, True, False, True),
          'D': (False, 'gen', 1, False, True, False), 'E': (False, 'gen', 0, True, True, False)}
SMALL = (1, 63, 64, 65, 70, 129)


def _sizes(H):
    caps = sorted({VR.cap_rows(k, H) for k in VR.GEOMETRY})
    return [(n, cb) for n in SMALL for cb in 'ABCDE'] + [(n + d, cb) for n in caps for d, cb in ((0, 'A'), (1, 'B'))] + \
           [(VR.large_rows(k, H), cb) for k, cb in (('var_head_fwd', 'B'), ('var_head_bwd', 'A'))]


CASES = [(H, N, cb) for H in VR.WIDTHS for N, cb in _sizes(H)]


@pytest.mark.parametrize('H,N,combo', CASES)
def test_both_entries_against_float64(H, N, combo):
    dev = _dev()
    wide, eps, sample, gZ, gkl, ML = COMBOS[combo]
    c = VR.case(H, N, seed=len(combo) + N % 7, wide=wide)
    if eps == 'gen' and sample:
        c = dict(c, eps_dev=_device_noise(c, dev))
    ref_c = dict(c, eps=c['eps_dev']) if 'eps_dev' in c else c          # the restatement on the device's own noise
    kw = dict(eps='given', sample=sample, gZ=gZ, gkl=gkl)
    r64, rk = VR.exact(ref_c, **kw), VR.stand_in(ref_c, **kw)
    tau = VR.taus(r64, rk)
    tag = 'H=%d N=%d %s' % (H, N, combo)
    f1, bad1 = run_fwd(c, dev, eps=eps, sample=sample, ML=ML)
    b1, bad2, a0 = run_bwd(c, dev, r64, eps=eps, sample=sample, gZ=gZ, gkl=gkl)
    bad = ['not intact: %s' % b for b in bad1 + bad2]
    bad += _compare('fwd', tag, f1, r64, tau)
    bad += _compare('bwd', tag, b1, r64, tau, a0=a0)
    # twice bit-identical, the KL sums included
    f2, _ = run_fwd(c, dev, eps=eps, sample=sample, ML=ML)
    b2, _, _ = run_bwd(c, dev, r64, eps=eps, sample=sample, gZ=gZ, gkl=gkl)
    for k in f1:
        if not torch.equal(f1[k].view(torch.int64 if f1[k].dtype == F64 else I32), f2[k].view(torch.int64 if f2[k].dtype == F64 else I32)):
            bad.append('fwd %s differs between two calls' % k)
    for k in b1:
        if not torch.equal(b1[k].view(I32), b2[k].view(I32)):
            bad.append('bwd %s differs between two calls' % k)
    if sample == 0 and ML:
        if not torch.equal(f1['Z'][:, :H], f1['ML'][:, :H]) or not torch.equal(f1['Z'][:, H:], f1['ML'][:, 2 * H:3 * H]):
            bad.append('sample = 0: Z is not mu')
    assert not bad, '\n'.join(bad)


def test_reference_fixture_directly():
    """N = 70, H = 64: the reference's own sample_*, KL values and gradients.  The fixture is float32 arithmetic, within
    (2H + N + 8) 2^-24 of the exact value on each entry's scale (tests/test_var_head_spec.py); the device within tau: the sum bounds
    their distance."""
    dev = _dev()
    z = load_golden('g4_vae')
    c = VR.fixture_case(z)
    want = VR.fixture_expected(z)
    r64 = VR.exact(c)
    tau = VR.taus(r64, VR.stand_in(c))
    extra = (2 * c['H'] + c['N'] + 8) * DR.U24
    f, bad1 = run_fwd(c, dev)
    b, bad2, a0 = run_bwd(c, dev, r64)
    fx = dict(r64, **{k: want[k] for k in ('Z', 'dST') + ACC})
    fx['kl'] = want['kl_loss'] / c['klcoef']
    bad = ['not intact: %s' % x for x in bad1 + bad2]
    bad += _compare('fwd', 'fixture', {k: f[k] for k in ('Z', 'kl')}, fx, tau, extra=extra)
    bad += _compare('bwd', 'fixture', b, fx, tau, a0=a0, extra=extra)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('H', VR.WIDTHS)
@pytest.mark.parametrize('eps', ['given', 'gen'])
def test_fused_route_against_composed_route(H, eps, monkeypatch):
    """ops.var_head: VarHeadFn against ops.linear + ReparamFn under autograd, within tau of each other on every output's scale (both
    lie within tau of float64); with generated noise the two routes draw the same numbers (same element numbering, same seed pair)."""
    dev = _dev()
    from deepgate import ops
    c = VR.case(H, 129, seed=6)
    if eps == 'gen':
        c = dict(c, eps=_device_noise(c, dev))
    r64 = VR.exact(c)
    tau = VR.taus(r64, VR.stand_in(c))
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, 'VAR_HEAD_FUSED', fused)
        assert ops.var_head_fused(H) is (fused and ops.use_x3(H))
        st = c['ST'][:, :2 * H].to(dev).requires_grad_(True)
        heads = []
        for h in (0, 1):
            W, b = c['Wp'][h].to(dev), c['bp'][h].to(dev)
            heads += [W[:H].clone().requires_grad_(True), b[:H].clone().requires_grad_(True), W[H:].clone().requires_grad_(True), b[H:].clone().requires_grad_(True)]
        zz, kl = ops.var_head(st, tuple(heads), eps=c['eps'][:, :2 * H].to(dev) if eps == 'given' else None, seed=c['seed'], sample=True)
        gk = torch.tensor(c['gkl'], dtype=F32, device=dev)
        ((zz * c['gZ'][:, :2 * H].to(dev)).sum() + (kl * gk).sum()).backward()
        g = [p.grad for p in heads]
        res[fused] = {'Z': zz.detach(), 'kl': kl.detach().double(), 'dST': st.grad, 'dWp_s': torch.cat([g[0], g[2]]), 'dbp_s': torch.cat([g[1], g[3]]),
                      'dWp_t': torch.cat([g[4], g[6]]), 'dbp_t': torch.cat([g[5], g[7]])}
    bad = _compare('fused', 'H=%d %s vs float64' % (H, eps), res[True], r64, tau)
    line = []
    for k, S in r64['S'].items():
        if k not in res[True]:
            continue
        extra = 2.0 ** -24 if k == 'kl' else 0.0                   # both routes hand the sums on as float32
        q = DR.ratio(res[True][k], res[False][k].cpu().to(F64), S)
        line.append('%s %.2g/%.2g' % (k, q, tau[k]))
        if not q <= tau[k] + extra:
            bad.append('fused vs composed %s: %.3g, bound %.3g' % (k, q, tau[k]))
    print('VH routes H=%d %s | %s' % (H, eps, ' | '.join(line)))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('H', VR.WIDTHS)
def test_refusals_leave_every_output_untouched(H):
    dev = _dev()
    c = VR.case(H, 70, seed=8)
    r64 = VR.exact(c)
    EINVAL, EUNSUPPORTED = -1, -2
    fwd_bad = [(dict(H=16), EUNSUPPORTED), (dict(H=128), EUNSUPPORTED), (dict(ldst=2 * H - 4), EINVAL), (dict(ldz=2 * H + 2), EINVAL), (dict(ST=None), EINVAL),
               (dict(kl=None), EINVAL), (dict(nws=VR.ws_floats(H, 70, False) - 1), EINVAL), (dict(sample=3), EINVAL), (dict(N=-1), EINVAL), (dict(N=0), 0)]
    for raw, want in fwd_bad:
        rc, clean = run_fwd(c, dev, raw=raw)
        assert rc == want and clean, ('fwd', raw, rc, clean)
    bwd_bad = [(dict(H=16), EUNSUPPORTED), (dict(H=48), EUNSUPPORTED), (dict(lddst=2 * H - 4), EINVAL), (dict(ldg=2 * H + 1), EINVAL), (dict(dST=None), EINVAL),
               (dict(tt_=None), EINVAL), (dict(dbs=None), EINVAL), (dict(nws=VR.ws_floats(H, 70, True) - 1), EINVAL), (dict(N=-1), EINVAL), (dict(N=0), 0)]
    for raw, want in bwd_bad:
        rc, clean = run_bwd(c, dev, r64, raw=raw)
        assert rc == want and clean, ('bwd', raw, rc, clean)
