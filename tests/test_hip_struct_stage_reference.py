"""The struct-stage half-round kernels (AggConv -> GRU -> LayerNorm and its backward), every implementation on its own against the
float64 restatement of tests/struct_stage_ref.py (pinned on the CPU by tests/test_struct_stage_spec.py, which also asserts the
properties of the case builders used here and shows that the defects these tests are there to catch are far outside their bound):

  f32    struct_stage.hip, exact fp32, H = 16 / 32 / 64                    rows   its general-feature form (xrow per node, d_xrow)
  x3     struct_stage_x3.hip: forward and the first backward, H = 32 (the first backward serves that width only: at H = 64 it
         returns MGV_EUNSUPPORTED, test_refusals_are_return_codes)
  bwd2   struct_stage_bwd2_x3.hip, the H = 64 backward, with the H = 64 forward of struct_stage_x3.hip: every case here checks that
         forward's h_out and {mean, rstd} as well

Every call here goes through the C ABI with 64 guard rows behind each output (NaN before the call, bit-identical after it),
NaN-filled workspaces and accumulators pre-filled with random values a0; test_through_ops repeats a selection through
deepgate.ops.  Outputs are compared ROW BY ROW (h_out, {mean, rstd}, g_direct, g_agg, d_xrow) and parameter gradients ENTRY BY ENTRY,
each on its own scale S from the float64 run: err <= tau S, tau = 8 max(r, floor), where r is the worst such ratio FOR THAT OUTPUT
of the CPU restatement in the kernel's arithmetic (float32, or the bf16x3 emulation) on the same inputs and floor = 2^-23 (fp32) or
2^-17 (bf16x3).  8: the device has one-ulp exp / reciprocal instructions, its own summation order in the MFMA accumulation and
cross-lane LayerNorm sums.  Nothing is taken from what the device produced.  An accumulator entry additionally gets 2^-24 |a0| (the
rounding of the final sum), and an entry with S = 0 (the absent class's dxtab row) must come back as a0 exactly.  Every check prints
the device's ratio beside tau.

Every check prints one line `SS <implementation> H=.. <case> | <output> ratio/tau | ...`; the table of the worst device ratio per
implementation and output is in NOTEBOOK.md (entry of 2026-10-17: the largest share of a bound in use on an MI355X is 0.59)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import struct_stage_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
FLOOR = {'f32': 2.0 ** -23, 'x3': 2.0 ** -17}
MM = {'f32': 'f32', 'rows': 'f32', 'x3': 'x3', 'bwd2': 'x3'}
GUARD = 64
ACCS = ('dWc', 'dbc', 'dWhh', 'dbhh', 'dxtab', 'dln_w', 'dln_b')


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)      # (one float64 run per case, shared by every implementation and test that uses the case)
def _case(H, size, lists='designed', mode='plain', C=6, ln=True, agg=True, rows=False):
    c = SR.case(H, size, lists=lists, mode=mode, C=C, ln=ln, agg=agg, rows=rows)
    return c, SR.half_round(c)


@functools.lru_cache(maxsize=None)
def _tau(mm, *key):
    c, r64 = _case(*key)
    r = SR.ratios(SR.half_round(c, F32, 'x3' if mm == 'x3' else 'exact'), r64)
    return {k: 8 * max(v, FLOOR[mm]) for k, v in r.items()}


def _guarded(n, width, dev):
    t = torch.full((n + GUARD, width), float('nan'), dtype=F32, device=dev)
    return t


def _guard_ok(t, n):
    g = t[n:].view(torch.int32)
    return bool((g == g[0, 0]).all()) and bool(torch.isnan(t[n:]).all())


def _run(impl, c, dev, need_input_grad=True, stats='kept', heavy=True, forward_only=False, ws_fill=float('nan'), seed=1):
    """One forward and one backward call of `impl` on case c through the C ABI.  Returns ({output: tensor}, {accumulator: a0})."""
    from deepgate import _hip, ops
    p = _hip.ptr
    H, N = c['H'], c['N']
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    x3 = impl in ('x3', 'bwd2')
    has_ln = c['ln_w'] is not None
    out = {}
    h_out = _guarded(N, H, dev)
    st = _guarded(N, 2, dev) if x3 and has_ln and stats == 'kept' else None
    hv = (0, None, None)
    if x3 and heavy and c['heavy'][0] > 0:
        hws = torch.full((2 * c['heavy'][0] * H + GUARD,), ws_fill, dtype=F32, device=dev)
        hv = (c['heavy'][0], p(d['heavy'][1].to(dev)), p(hws))
    if x3:
        wpack = ops.stage_wpack(d['Wc'], d['Whh'])
        tail = (*hv, p(d['own_idx']), int(c['tagged']))
        _hip.call('mgv_struct_stage_fwd_x3', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), c['C'], p(wpack), p(d['bc']),
                  p(d['bhh']), p(d['ln_w']), p(d['ln_b']), SR.LN_EPS, p(h_out), *tail, p(st))
    elif impl == 'rows':
        _hip.call('mgv_struct_stage_rows_fwd', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xrow']), p(d['Wc']), p(d['bc']), p(d['Whh']), p(d['bhh']),
                  p(d['ln_w']), p(d['ln_b']), SR.LN_EPS, p(h_out))
    else:
        assert c['own_idx'] is None
        _hip.call('mgv_struct_stage_fwd', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), c['C'], p(d['Wc']), p(d['bc']),
                  p(d['Whh']), p(d['bhh']), p(d['ln_w']), p(d['ln_b']), SR.LN_EPS, p(h_out))
    torch.cuda.synchronize()
    assert _guard_ok(h_out, N), 'forward wrote behind row N of h_out'
    out['h_out'] = h_out[:N]
    if st is not None:
        assert _guard_ok(st, N), 'forward wrote behind row N of ln_stats_out'
        out['mean'], out['rstd'] = st[:N, 0], st[:N, 1]
    if forward_only:
        return out, {}
    g = torch.Generator().manual_seed(seed)
    shapes = {'dWc': (3 * H, H), 'dbc': (3 * H,), 'dWhh': (3 * H, H), 'dbhh': (3 * H,), 'dln_w': (H,), 'dln_b': (H,)}
    shapes['dxrow' if impl == 'rows' else 'dxtab'] = (N, 3 * H) if impl == 'rows' else (c['C'], 3 * H)
    a0 = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    acc = {}
    for k, v in a0.items():
        if k == 'dxrow':
            acc[k] = _guarded(N, 3 * H, dev)
            acc[k][:N] = v.to(dev)
        else:
            acc[k] = v.to(dev).clone()
    gd = _guarded(N, H, dev) if need_input_grad else None
    ga = _guarded(N, H, dev) if need_input_grad else None
    lnacc = (p(acc['dln_w']), p(acc['dln_b']))
    if x3:
        head = (H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), c['C'], p(wpack), p(d['bc']), p(d['bhh']), p(d['ln_w']), p(d['ln_b']),
                SR.LN_EPS, p(d['gy_direct']), p(d['gy_agg']), p(gd), p(ga), p(acc['dWc']), p(acc['dbc']), p(acc['dWhh']), p(acc['dbhh']), p(acc['dxtab']), *lnacc)
        if impl == 'bwd2':
            nws = _hip.call_value('mgv_struct_stage_bwd2_ws_floats', H, N)
            ws = torch.full((nws + GUARD,), ws_fill, dtype=F32, device=dev)
            _hip.call('mgv_struct_stage_bwd2_x3', *head, p(ws), nws, *tail, p(st))
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws[nws:]).all()) if ws_fill != ws_fill else bool((ws[nws:] == ws_fill).all()), 'bwd2 wrote behind its workspace'
        else:
            _hip.call('mgv_struct_stage_bwd_x3', *head, *tail)
    else:
        WcT, WhhT = d['Wc'].t().contiguous(), d['Whh'].t().contiguous()
        mid = (p(d['xrow']),) if impl == 'rows' else (p(d['xcls']), p(d['xtab']), c['C'])
        _hip.call('mgv_struct_stage_rows_bwd' if impl == 'rows' else 'mgv_struct_stage_bwd', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), *mid,
                  p(d['Wc']), p(WcT), p(d['bc']), p(d['Whh']), p(WhhT), p(d['bhh']), p(d['ln_w']), p(d['ln_b']), SR.LN_EPS, p(d['gy_direct']), p(d['gy_agg']),
                  p(gd), p(ga), p(acc['dWc']), p(acc['dbc']), p(acc['dWhh']), p(acc['dbhh']), p(acc['dxrow' if impl == 'rows' else 'dxtab']), *lnacc)
    torch.cuda.synchronize()
    if need_input_grad:
        assert _guard_ok(gd, N) and _guard_ok(ga, N), 'backward wrote behind row N of an input gradient'
        out['g_direct'], out['g_agg'] = gd[:N], ga[:N]
    if impl == 'rows':
        assert _guard_ok(acc['dxrow'], N), 'backward wrote behind row N of d_xrow'
        acc['dxrow'] = acc['dxrow'][:N]
    if not has_ln:
        for k in ('dln_w', 'dln_b'):
            assert torch.equal(acc.pop(k).cpu(), a0.pop(k)), 'LayerNorm accumulators touched without a LayerNorm'
    out.update(acc)
    return out, a0


def _compare(tag, got, a0, r64, tau):
    """Ratio err / S per output against tau (module docstring); prints, then asserts."""
    line, bad = [], []
    for k, v in got.items():
        v = v.detach().cpu().to(F64)
        ref, S = r64[k], r64['S'][k]
        if k in a0:
            b = a0[k].to(F64)
            zero = S == 0
            if bool(zero.any()) and not torch.equal(v[zero].to(F32), a0[k][zero]):
                bad.append('%s: an entry nothing contributes to changed' % k)
            err = ((v - b) - ref).abs() - U24 * b.abs()
            if err.dim() == S.dim() + 1:
                err = err.amax(1)
            r = float((err.clamp(min=0) / S.clamp(min=1e-300))[~zero].max()) if bool((~zero).any()) else 0.0
            if not bool(torch.isfinite(v).all()):
                r = float('inf')
        else:
            r = SR.ratio(v, ref, S)
        line.append('%s %.2g/%.2g' % (k, r, tau[k]))
        if not r <= tau[k]:
            bad.append('%s: %.3g of its scale, bound %.3g' % (k, r, tau[k]))
    print('SS %s | %s' % (tag, ' | '.join(line)))
    assert not bad, (tag, bad)


def _check(impl, H, size, lists='designed', mode='plain', C=6, ln=True, agg=True, **opts):
    key = (H, size, lists, mode, C, ln, agg, impl == 'rows')
    c, r64 = _case(*key)
    got, a0 = _run(impl, c, _dev(), **opts)
    tag = '%s H=%d %s %s %s C=%d%s%s %s' % (impl, H, size, lists, mode, C, '' if ln else ' noLN', '' if agg else ' noagg',
                                           ' '.join('%s=%s' % kv for kv in sorted(opts.items())))
    _compare(tag, got, a0, r64, _tau(MM[impl], *key))


IMPLS = [('f32', 16), ('f32', 32), ('f32', 64), ('rows', 16), ('rows', 32), ('rows', 64), ('x3', 32), ('bwd2', 64)]
ALL_SIZES = tuple(SR.SIZES)
SOME_SIZES = ('n1', 'n65', 't9', 't17', 't257')


@pytest.mark.parametrize('impl,H', IMPLS, ids=['%s-%d' % i for i in IMPLS])
def test_every_size_against_float64(impl, H):
    """The designed list layout (tests/struct_stage_ref.py degrees(): chunked and generic tiles, 504 / 505 totals, a listed heavy row
    on the chunked path, the heavy ladder 64 .. 129 and a 600-entry hub, heavy rows as node 0, node N - 1 and in the partial tile)
    at every named size for the H = 64 kernels and the H = 32 bf16x3 ones, a selection for the other widths of the fp32 kernels
    (one template, the tile loop does not depend on H)."""
    sizes = ALL_SIZES if (impl, H) in (('f32', 64), ('x3', 32), ('bwd2', 64)) else SOME_SIZES
    for size in sizes:
        _check(impl, H, size)


@pytest.mark.parametrize('impl,H', IMPLS, ids=['%s-%d' % i for i in IMPLS])
def test_list_layouts_and_switches(impl, H):
    """Empty lists (E = 0, a one-element dummy idx) and lists of 0..7 entries only; LayerNorm off; gy_agg NULL; no input gradients
    (both output pointers NULL: the parameter gradients hold); C = 1 and C = 8; for the bf16x3 kernels the heavy layouts without the
    heavy list (rows walked in place) and the backward without kept statistics."""
    for size in ('n65', 't9'):
        _check(impl, H, size, lists='empty')
        _check(impl, H, size, lists='small')
    for size in ('n65', 't17'):
        _check(impl, H, size, ln=False)
        _check(impl, H, size, agg=False)
        _check(impl, H, size, need_input_grad=False)
    if H == 64:
        _check(impl, H, 't257', need_input_grad=False)
    if impl != 'rows':
        _check(impl, H, 't9', C=1)
        _check(impl, H, 't9', C=8)
    if impl in ('x3', 'bwd2'):
        for size in ('n2', 't9', 't257'):
            _check(impl, H, size, heavy=False)
        _check(impl, H, 't9', ln=False, agg=False, heavy=False, need_input_grad=False)
    if impl == 'bwd2':
        for size in ('n1', 't9', 't257'):
            _check(impl, H, size, stats=None)


@pytest.mark.parametrize('impl,H', [('f32', 16), ('f32', 32), ('f32', 64), ('rows', 32), ('x3', 32), ('bwd2', 64)])
def test_index_forms(impl, H):
    """h_in longer than the stage (every implementation); for the bf16x3 kernels the tagged table form (entries node | row << 24, rows
    >= 128 negative as int32, own rows through the index; at H = 64 with bwd2, at H = 32 the forward alone, as the product never
    calls the first backward tagged) and the untagged own-index form of the quotient stages with h_in shorter and longer than N."""
    for size in ('n1', 'n65', 't9', 't17') + (('t257',) if H == 64 else ()):
        _check(impl, H, size, mode='n_rows')
        if impl in ('x3', 'bwd2'):
            _check(impl, H, size, mode='own_few')
            _check(impl, H, size, mode='own_more')
            if H == 64:
                _check(impl, H, size, mode='tagged')
    if impl in ('x3', 'bwd2') and H == 64:
        _check(impl, H, 't17', mode='tagged', heavy=False)
        _check(impl, H, 't9', mode='tagged', agg=False, need_input_grad=False)
    if impl == 'x3' and H == 32:
        c, r64 = _case(32, 't9', 'designed', 'tagged')
        got, _ = _run('x3', c, _dev(), forward_only=True)          # the H = 32 forward supports the tagged form
        _compare('x3 H=32 t9 tagged forward', got, {}, r64, _tau('x3', 32, 't9', 'designed', 'tagged'))


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def test_bwd2_is_bit_identical_with_other_garbage_in_the_workspace():
    """513 tiles (three per workgroup; heavy, generic and chunked tiles): two calls, NaN and then 1e30 in the slab workspace and the
    heavy-row scratch before the call, other values in the accumulators' stead: every output, accumulators included, bit for bit."""
    dev = _dev()
    c, _ = _case(64, 't513')
    a, a0 = _run('bwd2', c, dev, ws_fill=float('nan'))
    b, b0 = _run('bwd2', c, dev, ws_fill=1e30)
    assert all(torch.equal(a0[k], b0[k]) for k in a0)
    diff = [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]
    print('SS bwd2 twice at %d rows: outputs that differ: %s' % (c['N'], diff or 'none'))
    assert not diff


@pytest.mark.parametrize('impl,H', [('f32', 16), ('f32', 32), ('f32', 64), ('rows', 64), ('x3', 32), ('x3', 64)])
def test_forward_is_bit_identical_twice(impl, H):
    dev = _dev()
    for size, mode in (('t9', 'plain'), ('t257', 'plain')) + ((('t9', 'own_few'),) if impl == 'x3' else ()):
        c, _ = _case(H, size, 'designed', mode, 6, True, True, impl == 'rows')
        a, _ = _run(impl, c, dev, forward_only=True, ws_fill=float('nan'))
        b, _ = _run(impl, c, dev, forward_only=True, ws_fill=-3.0)
        assert all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a), (impl, H, size)


@pytest.mark.parametrize('precision,H', [('f32', 16), ('f32', 32), ('f32', 64), ('x3', 32), ('x3', 64)])
def test_through_ops(precision, H):
    """deepgate.ops.struct_stage_fwd / struct_stage_bwd (their own allocation, heavy scratch, slab workspace and weight pack) under
    both settings of ops.PRECISION, same bound; kept statistics and stats=None; and the forms an implementation does not support are
    refused before anything is launched."""
    dev = _dev()
    from deepgate import ops
    from deepgate._hip import HipLibraryError
    old = ops.PRECISION
    ops.PRECISION = precision
    try:
        x3 = ops.use_x3(H)
        assert x3 == (precision == 'x3')
        modes = ('plain', 'n_rows') + (('own_few',) if x3 else ()) + (('tagged',) if x3 and H == 64 else ())
        for size in ('n65', 't257'):
            for mode in modes:
                for keep in ((True, False) if x3 and H == 64 else (False,)):
                    key = (H, size, 'designed', mode, 6, True, True, False)
                    c, r64 = _case(*key)
                    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
                    N = c['N']
                    heavy = (c['heavy'][0], c['heavy'][1].to(dev))
                    kw = dict(heavy=heavy, table_own=d['own_idx'], n_rows=N if mode == 'n_rows' else None, tagged=c['tagged'])
                    w = (d['xcls'], d['xtab'], d['Wc'], d['bc'], d['Whh'], d['bhh'], d['ln_w'], d['ln_b'])
                    st = torch.empty(N, 2, device=dev) if keep else None
                    h = ops.struct_stage_fwd(d['h_in'], d['ptr'], d['idx'], *w, stats_out=st, **kw)
                    acc = {k: torch.zeros_like(d[k[1:]]) for k in ('dWc', 'dbc', 'dWhh', 'dbhh', 'dxtab')}
                    acc['dln_w'], acc['dln_b'] = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
                    gd, ga = ops.struct_stage_bwd(d['h_in'], d['ptr'], d['idx'], *w, d['gy_direct'], d['gy_agg'], acc, stats=st, **kw)
                    got = dict(acc, h_out=h, g_direct=gd, g_agg=ga)
                    if keep:
                        got['mean'], got['rstd'] = st[:, 0], st[:, 1]
                    assert h.shape == (N, H) and gd.shape == (N, H) and ga.shape == (N, H)
                    _compare('ops %s H=%d %s %s stats=%s' % (precision, H, size, mode, keep), got, {}, r64, _tau(precision, *key))
        # unsupported forms: refused by ops, nothing launched, nothing written
        c, _ = _case(H, 'n65', 'designed', 'tagged' if x3 else 'own_more')
        if not (x3 and H == 64):
            d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
            w = (d['xcls'], d['xtab'], d['Wc'], d['bc'], d['Whh'], d['bhh'], d['ln_w'], d['ln_b'])
            acc = {k: torch.zeros_like(d[k[1:]]) for k in ('dWc', 'dbc', 'dWhh', 'dbhh', 'dxtab')}
            acc['dln_w'], acc['dln_b'] = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
            with pytest.raises((AssertionError, HipLibraryError)):
                ops.struct_stage_bwd(d['h_in'], d['ptr'], d['idx'], *w, d['gy_direct'], d['gy_agg'], acc, table_own=d['own_idx'], tagged=c['tagged'])
            assert all(float(v.abs().max()) == 0 for v in acc.values())
            if not x3:
                with pytest.raises((AssertionError, HipLibraryError)):
                    ops.struct_stage_fwd(d['h_in'], d['ptr'], d['idx'], *w, table_own=d['own_idx'], tagged=False)
    finally:
        ops.PRECISION = old


def test_refusals_are_return_codes():
    """Every refusal comes back as MGV_EINVAL / MGV_EUNSUPPORTED from the argument check, with the outputs untouched; no call here
    could launch anything (a refused call returns before its first launch).  bwd_x3() is the first backward at H = 64: its rows with a
    bad argument are refused by the argument check, and with every argument valid the width is (MGV_EUNSUPPORTED: H = 32 only)."""
    dev = _dev()
    from deepgate import _hip, ops
    from deepgate._hip import HipLibraryError
    p = _hip.ptr
    c, _ = _case(64, 'n65', 'designed', 'tagged')
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
    N = c['N']
    wpack = ops.stage_wpack(d['Wc'], d['Whh'])
    WcT, WhhT = d['Wc'].t().contiguous(), d['Whh'].t().contiguous()
    outs = {k: torch.full(s, 7.25, device=dev) for k, s in (('h_out', (N, 64)), ('st', (N, 2)), ('gd', (N, 64)), ('ga', (N, 64)), ('dWc', (192, 64)), ('dbc', (192,)),
                                                            ('dWhh', (192, 64)), ('dbhh', (192,)), ('dxtab', (8, 192)), ('dln_w', (64,)), ('dln_b', (64,)))}
    nws = _hip.call_value('mgv_struct_stage_bwd2_ws_floats', 64, N)
    ws = torch.full((nws,), 7.25, device=dev)
    assert nws > 0 and nws % SR.grid_for((N + 63) // 64) == 0
    assert _hip.call_value('mgv_struct_stage_bwd2_ws_floats', 32, N) == 0

    def fwd_x3(H=64, N=N, C=6, ln_w=d['ln_w'], ln_b=d['ln_b'], own=None, tagged=0):
        _hip.call('mgv_struct_stage_fwd_x3', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), C, p(wpack), p(d['bc']), p(d['bhh']),
                  p(ln_w), p(ln_b), SR.LN_EPS, p(outs['h_out']), 0, None, None, p(own), tagged, p(outs['st']))

    def bwd_x3(entry='mgv_struct_stage_bwd_x3', H=64, N=N, C=6, ln_w=d['ln_w'], ln_b=d['ln_b'], gd=outs['gd'], ga=outs['ga'], own=None, tagged=0, nws=nws):
        extra = (p(ws), nws) if entry.endswith('bwd2_x3') else ()
        last = (p(outs['st']),) if entry.endswith('bwd2_x3') else ()
        _hip.call(entry, H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), C, p(wpack), p(d['bc']), p(d['bhh']), p(ln_w), p(ln_b),
                  SR.LN_EPS, p(d['gy_direct']), p(d['gy_agg']), p(gd), p(ga), p(outs['dWc']), p(outs['dbc']), p(outs['dWhh']), p(outs['dbhh']), p(outs['dxtab']),
                  p(outs['dln_w']), p(outs['dln_b']), *extra, 0, None, None, p(own), tagged, *last)

    def f32(bwd, H=64, N=N, C=6, ln_w=d['ln_w'], ln_b=d['ln_b'], gd=outs['gd'], ga=outs['ga']):
        if not bwd:
            return _hip.call('mgv_struct_stage_fwd', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), C, p(d['Wc']), p(d['bc']), p(d['Whh']),
                             p(d['bhh']), p(ln_w), p(ln_b), SR.LN_EPS, p(outs['h_out']))
        _hip.call('mgv_struct_stage_bwd', H, N, p(d['h_in']), p(d['ptr']), p(d['idx']), p(d['xcls']), p(d['xtab']), C, p(d['Wc']), p(WcT), p(d['bc']), p(d['Whh']),
                  p(WhhT), p(d['bhh']), p(ln_w), p(ln_b), SR.LN_EPS, p(d['gy_direct']), p(d['gy_agg']), p(gd), p(ga), p(outs['dWc']), p(outs['dbc']), p(outs['dWhh']),
                  p(outs['dbhh']), p(outs['dxtab']), p(outs['dln_w']), p(outs['dln_b']))

    B2 = 'mgv_struct_stage_bwd2_x3'
    refused = [
        ('MGV_EUNSUPPORTED', lambda: fwd_x3(H=16)), ('MGV_EUNSUPPORTED', lambda: bwd_x3(H=16)), ('MGV_EUNSUPPORTED', lambda: bwd_x3(B2, H=32)),
        ('MGV_EUNSUPPORTED', lambda: bwd_x3(B2, H=16)), ('MGV_EUNSUPPORTED', lambda: f32(False, H=48)), ('MGV_EUNSUPPORTED', lambda: f32(True, H=128)),
        ('MGV_EINVAL', lambda: bwd_x3(B2, nws=nws - 1)), ('MGV_EUNSUPPORTED', lambda: bwd_x3()),
    ]
    for C in (0, 9):
        refused += [('MGV_EINVAL', lambda C=C: fwd_x3(C=C)), ('MGV_EINVAL', lambda C=C: bwd_x3(C=C)), ('MGV_EINVAL', lambda C=C: bwd_x3(B2, C=C)),
                    ('MGV_EINVAL', lambda C=C: f32(False, C=C)), ('MGV_EINVAL', lambda C=C: f32(True, C=C))]
    for kw in (dict(ln_w=None), dict(ln_b=None)):
        refused += [('MGV_EINVAL', lambda kw=kw: fwd_x3(**kw)), ('MGV_EINVAL', lambda kw=kw: bwd_x3(**kw)), ('MGV_EINVAL', lambda kw=kw: bwd_x3(B2, **kw)),
                    ('MGV_EINVAL', lambda kw=kw: f32(False, **kw)), ('MGV_EINVAL', lambda kw=kw: f32(True, **kw))]
    for kw in (dict(gd=None), dict(ga=None)):
        refused += [('MGV_EINVAL', lambda kw=kw: bwd_x3(**kw)), ('MGV_EINVAL', lambda kw=kw: bwd_x3(B2, **kw)), ('MGV_EINVAL', lambda kw=kw: f32(True, **kw))]
    # tagged mode holds the node in 24 bits: N = 2^24 is refused from the argument check alone (N is a number here, no array has that size)
    big = dict(N=1 << 24, own=d['own_idx'], tagged=1)
    refused += [('MGV_EINVAL', lambda: fwd_x3(**big)), ('MGV_EINVAL', lambda: bwd_x3(**big)), ('MGV_EINVAL', lambda: bwd_x3(B2, **big))]
    for code, fn in refused:
        with pytest.raises(HipLibraryError, match=code):
            fn()
    # N = 0: accepted, nothing enqueued
    fwd_x3(N=0); bwd_x3(N=0); bwd_x3(B2, N=0); f32(False, N=0); f32(True, N=0)
    torch.cuda.synchronize()
    assert all(bool((v == 7.25).all()) for v in outs.values()) and bool((ws == 7.25).all())
    print('SS refusals: %d calls refused by return code, 5 empty calls accepted, every output untouched' % len(refused))
