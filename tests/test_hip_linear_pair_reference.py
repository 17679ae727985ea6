"""mgv_linear_pair_fwd_x3 / mgv_linear_pair_bwd_x3 (csrc/linear_x3.hip, the hs seam) through the C ABI, and ops.LinearPairFn on top of
them, every output entry by entry against the float64 restatement dense_ref.pair (pinned to two torch Linears under autograd by
tests/test_dense_spec.py, which also shows every defect these tests are there to catch at least 10x outside its bound).

Sizes: dense_ref.SMALL_ROWS (one tile per workgroup), cap_rows + 1 = 32,769 (workgroup 0 of the 512 comes round for a second tile:
the loop-carried prefetch, the barrier that lets the next tile's planes overwrite the staged rows, and the accumulators carried from
tile to tile are executed) and large_rows = 65,875 (workgroups 0..5 visit three tiles, the others two, the last tile is partial, the
prefetch condition is true and false within one launch).  tests/test_hip_linear_pair.py compares the same kernels bit for bit with
the launches they replace; here nothing is taken from the device.

Forms (VARIANTS): contiguous / every row matrix (inputs, outputs, and the HS the backward reads) a column slice of a NaN-holding
wider one; bl, bd given / NULL; gHS given / NULL; dbl, dbd given / NULL; coherent inputs (dense_ref.linear_case).  On every call: 64
NaN guard rows behind each row output and the foreign columns of a strided one bit-identical afterwards, a NaN-filled workspace with
a guard of its own, the accumulators dWl / dbl / dWd / dbd starting from a0 of each entry's own magnitude, every call made twice
with identical bits.

Bounds: err <= tau S entry by entry, tau = 8 max(r, 2^-17), r the worst ratio for that output of the CPU bf16x3 emulation against
float64 on the same case (dense_ref.pair_runs); accumulators additionally 2^-24 |a0|.  HS is judged against float64 from S and T; ST
against float64 of the device's OWN HS ('ST_given': its error in HS is HS's business, as var_head treats it); the backward takes the
device HS of the stand-alone forward as its given input, in the reference as on the device.  DERIVED_L is empty: no output of a
correct kernel was measured outside tau (NOTEBOOK.md has the table of the worst device ratio per entry and output).

Every check prints one line `LP <entry> <case> | <output> ratio/tau | ...`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_dev as DD  # noqa: E402
import dense_ref as DR  # noqa: E402
from dense_dev import Out  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, I32 = torch.float64, torch.float32, torch.int32
DERIVED_L = set()
FWD, BWD = 'linear_pair_fwd_x3', 'linear_pair_bwd_x3'
CAP1 = DR.cap_rows(BWD, DR.PAIR) + 1
BIG = DR.large_rows(BWD, DR.PAIR)
# (strided, bias, ghs, dbl / dbd given, coherent)
VARIANTS = [(False, True, True, True, False), (True, True, True, True, False), (False, False, True, True, False), (True, True, False, True, False),
            (False, True, True, False, False), (False, True, True, True, True), (True, False, False, False, False)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _hip():
    from deepgate import _hip
    return _hip


def _compare(entry, tag, got, r64, tau, a0=None):
    return DD.compare('LP', DERIVED_L, entry, tag, got, r64, tau, a0)


def _cache_small(fn):
    """One case and one float64 / bf16x3 run of it per key; of the cases past 4096 rows only the last is kept."""
    small, big = functools.lru_cache(maxsize=None)(fn), functools.lru_cache(maxsize=1)(fn)
    return lambda N, *key: small(N, *key) if N <= 4096 else big(N, *key)


@_cache_small
def _case(N, strided, bias, ghs, coherent):
    """(case, float64 run, tau per output): dense_ref.pair_runs, the backward's given HS the CPU emulation's."""
    c = DR.pair_case(N, strided=strided, bias=bias, ghs=ghs, coherent=coherent)
    r64, _, tau = DR.pair_runs(c)
    return c, r64, tau


def _pack(W, transpose, dev):
    h = _hip()
    n = W.numel()
    R, K = (W.shape[1], W.shape[0]) if transpose else W.shape
    pack = torch.full((2 * n + DD.GUARD,), DD.NAN, dtype=torch.bfloat16, device=dev)
    h.call('mgv_wpack_bf16x3', h.ptr(W), R, K, W.stride(0), int(transpose), h.ptr(pack[:n]), h.ptr(pack[n:]))
    return pack


def _on(c, dev):
    d = {k: (None if c[k] is None else c[k].on(dev)) for k in ('S', 'T', 'dST', 'gHS')}
    d.update({k: (None if c[k] is None else c[k].to(dev)) for k in ('Wl', 'bl', 'Wd', 'bd')})
    for k, W in (('l', d['Wl']), ('d', d['Wd'])):
        d['w' + k], d['w' + k + 't'] = _pack(W, False, dev), _pack(W, True, dev)
    return d


def _fwd(c, d, dev):
    h = _hip()
    p = h.ptr
    N = c['N']
    HS, ST = Out(N, 64, dev, c['strided']), Out(N, 128, dev, c['strided'])
    h.call('mgv_linear_pair_fwd_x3', N, p(d['S']), d['S'].stride(0), p(d['T']), d['T'].stride(0), p(d['wl']), p(d['bl']), p(d['wd']), p(d['bd']),
           p(HS.v), HS.ld, p(ST.v), ST.ld)
    torch.cuda.synchronize()
    assert HS.intact() and ST.intact(), 'the pair forward wrote outside its rows and columns'
    return HS, ST


def _bwd(c, d, HS, a0, with_db, dev):
    """One backward call from the accumulator contents a0, its given HS the forward's own output buffer (strided where the case is)."""
    h = _hip()
    p = h.ptr
    N = c['N']
    dS, dT = Out(N, 64, dev, c['strided']), Out(N, 64, dev, c['strided'])
    acc = {'dWl': Out(64, 128, dev, fill=a0['dWl'].to(dev)), 'dbl': Out(1, 64, dev, fill=a0['dbl'].to(dev)[None]),
           'dWd': Out(128, 64, dev, fill=a0['dWd'].to(dev)), 'dbd': Out(1, 128, dev, fill=a0['dbd'].to(dev)[None])}
    nws = h.call_value('mgv_linear_pair_bwd_x3_ws_floats', N)
    assert nws == DR.grid(BWD, DR.PAIR, N) * DR.PAIR_SLAB
    ws = DD.ws(nws, dev)
    g = d['gHS']
    h.call('mgv_linear_pair_bwd_x3', N, p(d['dST']), d['dST'].stride(0), p(g), 0 if g is None else g.stride(0), p(HS.v), HS.ld,
           p(d['S']), d['S'].stride(0), p(d['T']), d['T'].stride(0), p(d['wlt']), p(d['wdt']), p(dS.v), dS.ld, p(dT.v), dT.ld,
           p(acc['dWl'].v), p(acc['dbl'].v) if with_db else None, p(acc['dWd'].v), p(acc['dbd'].v) if with_db else None, p(ws), nws)
    torch.cuda.synchronize()
    assert DD.ws_intact(ws, nws), 'the pair backward wrote behind its workspace'
    assert dS.intact() and dT.intact() and all(o.intact() for o in acc.values()), 'the pair backward wrote outside its outputs'
    out = {'dS': dS.v, 'dT': dT.v, 'dWl': acc['dWl'].v, 'dWd': acc['dWd'].v}
    if with_db:
        out.update(dbl=acc['dbl'].v[0], dbd=acc['dbd'].v[0])
    else:
        assert torch.equal(acc['dbl'].v[0].cpu(), a0['dbl']) and torch.equal(acc['dbd'].v[0].cpu(), a0['dbd']), 'a bias gradient touched through a NULL pointer?'
    return out, [dS.parent, dT.parent] + [o.parent for o in acc.values()]


def _check(N, strided, bias, ghs, with_db, coherent, dev):
    c, r64, tau = _case(N, strided, bias, ghs, coherent)
    d = _on(c, dev)
    tag = 'N=%d%s%s%s%s%s' % (N, ' strided' if strided else '', '' if bias else ' nobias', '' if ghs else ' noghs', '' if with_db else ' nodb', ' coherent' if coherent else '')
    HS, ST = _fwd(c, d, dev)
    HS2, ST2 = _fwd(c, d, dev)
    assert torch.equal(DD.bits(HS.parent), DD.bits(HS2.parent)) and torch.equal(DD.bits(ST.parent), DD.bits(ST2.parent)), 'the pair forward differs between two identical calls'
    # float64 of the device's own HS: ST_given, and the backward whose given input that HS is
    rdev = DR.pair_ref(c, HS.v.cpu().to(F64))
    bad = _compare(FWD, tag, {'HS': HS.v, 'ST_given': ST.v}, rdev, tau)
    a0 = {k: DD.a0(rdev['S'][k], 11 + i) for i, k in enumerate(('dWl', 'dbl', 'dWd', 'dbd'))}
    got, raw = _bwd(c, d, HS, a0, with_db, dev)
    _, again = _bwd(c, d, HS, a0, with_db, dev)
    assert all(torch.equal(DD.bits(a), DD.bits(b)) for a, b in zip(raw, again)), 'the pair backward differs between two identical calls'
    return bad + _compare(BWD, tag, got, rdev, tau, {k: a0[k] for k in got if k in a0})


def test_pair_entries_below_the_grid_cap():
    """1 .. 129 rows with the forms in turn, then every form at 129 rows (three tiles, the last of one row)."""
    dev, bad = _dev(), []
    assert all(max(DR.visits(k, DR.PAIR, n)) == 1 for k in (FWD, BWD) for n in DR.SMALL_ROWS)
    for i, N in enumerate(DR.SMALL_ROWS):
        bad += _check(N, *VARIANTS[i % len(VARIANTS)], dev)
    for strided, bias, ghs, with_db, coherent in VARIANTS:
        bad += _check(129, strided, bias, ghs, with_db, coherent, dev)
    assert not bad, bad


@pytest.mark.parametrize('strided,bias,ghs,with_db,coherent', VARIANTS)
def test_pair_entries_one_row_past_the_grid_cap(strided, bias, ghs, with_db, coherent):
    """32,769 rows: 513 tiles on 512 workgroups, workgroup 0 visits tile 0 (whose rows are on top: dense_ref.pair_case) and tile 512."""
    dev = _dev()
    for k in (FWD, BWD):
        vis = DR.visits(k, DR.PAIR, CAP1)
        assert len(vis) == 512 and max(vis) >= 2 and vis[0] == 2
    bad = _check(CAP1, strided, bias, ghs, with_db, coherent, dev)
    assert not bad, bad


def test_pair_entries_two_and_three_tiles_per_workgroup():
    """65,875 rows, strided, everything given: three visits for workgroups 0..5, two for the others, a last tile of 19 rows."""
    dev = _dev()
    for k in (FWD, BWD):
        vis = DR.visits(k, DR.PAIR, BIG)
        assert max(vis) >= 3 and vis[:6] == [3] * 6 and min(vis) == 2 and BIG % DR.TILE == 19
    bad = _check(BIG, True, True, True, True, False, dev)
    assert not bad, bad


def test_pair_entries_refuse_on_the_device_and_write_nothing():
    """dense_ref.PAIR_REFUSALS (every clause of the two MGV_CHECK_ARG lines; tests/test_dense_spec.py makes the same calls without a
    device) over real buffers: MGV_EINVAL and every buffer bit-identical afterwards.  gHS NULL with any ldghs is served."""
    dev = _dev()
    h = _hip()
    N = 65
    c, r64, tau = _case(N, True, True, True, False)
    d = _on(c, dev)
    buf = {'HS': Out(N, 64, dev, True), 'ST': Out(N, 128, dev, True), 'dS': Out(N, 64, dev, True), 'dT': Out(N, 64, dev, True),
           'dWl': Out(64, 128, dev), 'dbl': Out(1, 64, dev), 'dWd': Out(128, 64, dev), 'dbd': Out(1, 128, dev)}
    nws = h.call_value('mgv_linear_pair_bwd_x3_ws_floats', N)
    ws = DD.ws(nws, dev)
    hs_in = Out(N, 64, dev, True, fill=torch.ones(N, 64, device=dev))
    fwd = dict(N=N, S=d['S'], lds=d['S'].stride(0), T=d['T'], ldt=d['T'].stride(0), wlpack_bf16=d['wl'], bl=d['bl'], wdpack_bf16=d['wd'], bd=d['bd'],
               HS=buf['HS'].v, ldhs=buf['HS'].ld, ST=buf['ST'].v, ldst=buf['ST'].ld)
    bwd = dict(N=N, dST=d['dST'], lddst=d['dST'].stride(0), gHS=d['gHS'], ldghs=d['gHS'].stride(0), HS=hs_in.v, ldhs=hs_in.ld, S=d['S'], lds=d['S'].stride(0),
               T=d['T'], ldt=d['T'].stride(0), wltpack_bf16=d['wlt'], wdtpack_bf16=d['wdt'], dS=buf['dS'].v, ldds=buf['dS'].ld, dT=buf['dT'].v, lddt=buf['dT'].ld,
               dWl=buf['dWl'].v, dbl=buf['dbl'].v, dWd=buf['dWd'].v, dbd=buf['dbd'].v, workspace=ws, workspace_floats=nws)

    def rc(name, **over):
        a = dict(fwd if name.endswith('fwd_x3') else bwd, **over)
        args = [h.ptr(x) if isinstance(x, torch.Tensor) else x for x in a.values()]
        return int(getattr(h.load(), name)(*args, h.stream()))

    for name, arg, value in DR.PAIR_REFUSALS:
        assert arg in (fwd if name.endswith('fwd_x3') else bwd)
        assert rc(name, **{arg: value}) == -1, (name, arg, value)
    torch.cuda.synchronize()
    assert all(bool((o.parent.view(I32) == DD.NANBITS).all()) for o in buf.values()) and bool((ws.view(I32) == DD.NANBITS).all()), 'a refused call wrote'
    for ld in DR.PAIR_GHS_NULL_ACCEPTS:
        assert rc('mgv_linear_pair_bwd_x3', gHS=None, ldghs=ld) == 0
    torch.cuda.synchronize()
    assert all(o.intact() for o in buf.values()) and DD.ws_intact(ws, nws)
    print('LP refusals: %d calls refused with MGV_EINVAL, every buffer untouched; gHS NULL served with ldghs in %s' % (len(DR.PAIR_REFUSALS), (DR.PAIR_GHS_NULL_ACCEPTS,)))


# ------------------------------------------------------------------------------------------------ through ops.LinearPairFn
PAIR_FWD, PAIR_BWD, LIN_FWD, LIN_BWD = 'mgv_linear_pair_fwd_x3', 'mgv_linear_pair_bwd_x3', 'mgv_linear_fwd_x3', 'mgv_linear_bwd_x3'
# route: (bias, the loss reads st, the loss reads hs, Wl trainable, s and t column slices of one tensor, launcher names of the backward)
ROUTES = {
    'both outputs': (True, True, True, True, False, [PAIR_BWD]),
    'st only': (True, True, False, True, False, [PAIR_BWD]),
    'hs only': (True, False, True, True, False, [LIN_BWD]),
    'Wl frozen': (True, True, True, False, False, [LIN_BWD, LIN_BWD]),
    'no biases': (False, True, True, True, False, [PAIR_BWD]),
    'column slices': (True, True, True, True, True, [PAIR_BWD]),
}


@functools.lru_cache(maxsize=2)
def _op_case(N, bias, use_st, use_hs):
    """The case, the float64 run of the chain on its own HS (scales and, against the emulation of the same chain, tau), and the
    float64 AUTOGRAD values the device is compared with.  A loss that does not read st has dST = 0, one that does not read hs no gHS."""
    c = DR.pair_case(N, bias=bias, ghs=use_hs)
    if not use_st:
        c['dST'] = DR.Operand(torch.zeros(N, 128))
    r64 = DR.pair_ref(c)
    tau = DR.taus(r64, DR.pair_ref(c, None, F32, 'x3'), 'x3')
    leaf = lambda t: None if t is None else t.to(F64).requires_grad_(True)       # noqa: E731
    S, T, Wl, bl, Wd, bd = (leaf(t) for t in (c['S'].v, c['T'].v, c['Wl'], c['bl'], c['Wd'], c['bd']))
    hs = torch.nn.functional.linear(torch.cat([S, T], 1), Wl, bl)
    st = torch.nn.functional.linear(hs, Wd, bd)
    loss = (st * c['dST'].v.to(F64)).sum() if use_st else 0
    if use_hs:
        loss = loss + (hs * c['gHS'].v.to(F64)).sum()
    loss.backward()
    z = lambda t, like: torch.zeros_like(like) if t is None or t.grad is None else t.grad       # noqa: E731
    auto = {'HS': hs.detach(), 'ST': st.detach(), 'dS': S.grad, 'dT': T.grad, 'dWl': Wl.grad, 'dWd': z(Wd, r64['dWd'])}
    if bias:
        auto.update(dbl=bl.grad, dbd=z(bd, r64['dbd']))
    auto['S'] = r64['S']
    return c, auto, tau


def _run_route(fn, c, route, dev, names=None, slices_ok=True):
    """fn(s, t, Wl, bl, Wd, bd) -> (hs, st) under the route's loss; the outputs and the gradients of the leaves that have one.
    slices_ok False: s and t contiguous whatever the route says (ops.linear's forward takes no column slice)."""
    bias, use_st, use_hs, train_wl, slices, _ = ROUTES[route]
    slices = slices and slices_ok
    N = c['N']
    if slices:
        wide = torch.full((N, 144), DD.NAN, dtype=F32, device=dev)
        wide[:, 4:68], wide[:, 72:136] = c['S'].v.to(dev), c['T'].v.to(dev)
        wide.requires_grad_(True)
        s, t = wide[:, 4:68], wide[:, 72:136]
    else:
        s, t = c['S'].v.to(dev).requires_grad_(True), c['T'].v.to(dev).requires_grad_(True)
    Wl, Wd = c['Wl'].to(dev).requires_grad_(train_wl), c['Wd'].to(dev).requires_grad_(True)
    bl, bd = (c[k].to(dev).requires_grad_(True) if bias else None for k in ('bl', 'bd'))
    hs, st = fn(s, t, Wl, bl, Wd, bd)
    loss = (st * c['dST'].v.to(dev)).sum() if use_st else 0
    if use_hs:
        loss = loss + (hs * c['gHS'].v.to(dev)).sum()
    if names is not None:
        names.append('backward')        # a mark: the backward's launches follow
    loss.backward()
    torch.cuda.synchronize()
    got = {'HS': hs.detach(), 'ST': st.detach(), 'dS': wide.grad[:, 4:68] if slices else s.grad, 'dT': wide.grad[:, 72:136] if slices else t.grad}
    got.update({k: w.grad for k, w in (('dWl', Wl), ('dbl', bl), ('dWd', Wd), ('dbd', bd)) if w is not None and w.grad is not None})
    return got


# (the routes that share a loss, and with it a reference, follow one another: _op_case keeps the last two)
OP_CASES = [(r, n) for n in (129, CAP1) for r in ('both outputs', 'Wl frozen', 'column slices', 'st only', 'hs only', 'no biases')]


@pytest.mark.parametrize('route,N', OP_CASES, ids=['%s-%d' % (r.replace(' ', '_'), n) for r, n in OP_CASES])
def test_linear_pair_fn(route, N, monkeypatch):
    """ops.LinearPairFn called directly (ops.LINEAR_PAIR_MIN_ROWS plays no part) under each route's loss: which launchers the
    backward calls; every output and gradient against float64 autograd within the per-entry bounds; and hs, st, ds, dt, dWl, dbl bit
    for bit what ops.linear called twice gives."""
    dev = _dev()
    from deepgate import _hip, ops
    if ops.PRECISION != 'x3':
        pytest.skip('the pair serves the bf16x3 mode')
    assert N == 129 or max(DR.visits(BWD, DR.PAIR, N)) >= 2
    bias, use_st, use_hs, train_wl, slices, want_names = ROUTES[route]
    c, auto, tau = _op_case(N, bias, use_st, use_hs)
    names, args = [], {}
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a: (names.append(name), args.__setitem__(name, a), real(name, *a))[2])
    got = _run_route(ops.LinearPairFn.apply, c, route, dev, names)
    monkeypatch.setattr(_hip, 'call', real)
    mark = names.index('backward')
    assert [n for n in names[:mark] if n != 'mgv_wpack_bf16x3'] == [PAIR_FWD], (route, names)
    assert [n for n in names[mark + 1:] if n != 'mgv_wpack_bf16x3'] == want_names, (route, names)
    if slices:      # the slices reach the launchers as they are: row stride 144, no copy (lds is argument 2 forward, 8 backward)
        assert args[PAIR_FWD][2] == 144 and args[PAIR_FWD][4] == 144 and args[PAIR_BWD][8] == 144 and args[PAIR_BWD][10] == 144
    assert ('dWl' in got) == train_wl and ('dWd' in got) == use_st and ('dbl' in got) == bias
    bad = _compare('ops.LinearPairFn', '%s N=%d' % (route, N), got, auto, tau)
    two = _run_route(lambda s, t, Wl, bl, Wd, bd: (lambda hs: (hs, ops.linear(hs, Wd, bd)))(ops.linear(s, Wl, bl, x2=t)), c, route, dev, slices_ok=False)
    for k in ('HS', 'ST', 'dS', 'dT', 'dWl', 'dbl'):
        assert (k in got) == (k in two)
        if k in got:
            assert torch.equal(DD.bits(got[k]), DD.bits(two[k])), '%s: %s differs from ops.linear called twice' % (route, k)
    assert not bad, bad
