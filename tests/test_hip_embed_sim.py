"""The functional-similarity entries of csrc/pair_scores.hip — mgv_row_unit, mgv_sim_select_count, mgv_sim_select_fill — through the C
ABI and through the surface (ops.row_unit / sim_topk / sim_pairs / sim_at, Model.similar_gates / equivalence_candidates /
functional_similarity, examples/feature_extract.py --similar / --equivalences), against tests/embed_sim_ref.py (pinned on the CPU by
tests/test_embed_sim_spec.py, which also asserts the properties of the case builders used here and shows the planted defects of a
restated upper fill to be caught by the checkers used here).

Unit rows: every entry within (H/2 + 3) 2^-24 |y| of float64, norms within (H/2 + 2) 2^-24 relative; zero, tiny, NaN and power-of-two
scaled rows exactly as the header says; sizes on both sides of the launch's grid cap (embed_sim_ref.unit_sizes).
Selection, on the device's own unit rows: exact against dense = mgv_pair_scores_fwd(y, y, sigmoid = 0) — dense equals its transpose in
bits, the lists equal nonzero((dense > thr) & upper_mask) in row-major order with the scores' bits, and together with their transposes
they are mgv_pair_select_* on (y, y, skip_self = 1); against float64 with no exclusions and the bound (2H + 6) 2^-24 S, after the band
has been measured.

Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold NaN; every output
has 64 guard rows behind it and is filled before the call (col -77, score NaN).  Every check prints one line `SIM <what> | figures`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import losses_ref as LR  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402
import test_hip_pair_scores as TP  # noqa: E402  (Out, the operand slices and the launcher helpers of the pair-score tests)
import test_hip_pair_select as TS  # noqa: E402  (Run: the general selection through the raw ABI)

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
SEEDS = (1, 2, 3)
NAN = TP.NAN
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
Out, _dev, _ptr, _rc, _call, _bits, _slice = TP.Out, TP._dev, TP._ptr, TP._rc, TP._call, TP._bits, TP._slice


class Rows(Out):
    """An [n][H] float output as the row kernels take it: columns 4 .. 4 + H of a matrix 8 wider (16-byte aligned rows, a stride that
    is a multiple of 4 and > H), GUARD rows behind it, NaN everywhere before the call."""

    def __init__(self, n, H, dev):
        self.n, self.w, self.off, self.fill = n, H, 4, NAN
        self.parent = torch.full((n + TP.GUARD, H + 8), NAN, dtype=F32, device=dev)
        self.v = self.parent[:n, 4:4 + H]
        self.ld = H + 8


@functools.lru_cache(maxsize=None)
def _case(H, seed=1, kind='sim'):
    c = ER.CASES[kind](H, seed)
    return c, ER.cos_ref(c['x'])


def _unit(dev, x, want_norm=True, eps=ER.EPS):
    """mgv_row_unit on a column slice of a NaN matrix -> (Rows y, Out norm or None)."""
    N, H = x.shape
    xv, ldx = _slice(x, dev)
    y, norm = Rows(N, H, dev), (Out(N, 1, dev) if want_norm else None)
    _call('mgv_row_unit', H, N, _ptr(xv), ldx, eps, _ptr(y.v), y.ld, None if norm is None else _ptr(norm.v))
    return y, norm


@functools.lru_cache(maxsize=None)
def _device_rows(H, seed=1, kind='sim'):
    """The device's own unit rows of a case, on the host (the operands of every selection test), and their dense scores."""
    dev = _dev()
    c, _ = _case(H, seed, kind)
    y = _unit(dev, c['x'], want_norm=False)[0].v.cpu().contiguous()
    dense = TP._fwd(dev, y, y, False)[0].v.cpu()
    return y, dense


# ------------------------------------------------------------------------------------------------ mgv_row_unit
@functools.lru_cache(maxsize=None)
def _unit_case(H):
    """Rows for every size of ER.unit_sizes(H): the 530 rows of sim_case (zero rows, the row below eps, the trio) in front, then rows
    up to one past the grid cap with a zero row, a NaN row and a row below eps at the very end (the strided part of the launch)."""
    c, _ = _case(H)
    n = ER.UNIT_CAP_ROWS[H] + 1
    g = torch.Generator().manual_seed(977 + H)
    x = torch.cat([c['x'], PR._rows(n - c['N'], H, g, 3.0)])
    x[n - 1] = 0
    x[n - 2, H - 1] = NAN
    x[n - 3] = (1e-10 * torch.randn(H, generator=g, dtype=F64)).to(F32)
    return x, ER.unit_ref(x), c['info']


@pytest.mark.parametrize('H', HS)
def test_row_unit_every_size(H):
    dev = _dev()
    x, ref, info = _unit_case(H)
    eps32 = float(torch.tensor(ER.EPS, dtype=F32))
    bad, wy, wn = [], 0.0, 0.0
    for N in ER.unit_sizes(H):
        xs = x[:N]
        y, norm = _unit(dev, xs)
        got, gn = y.v.cpu(), norm.v.cpu().flatten()
        ry, rn = ref['y'][:N], ref['norm'][:N]
        a, b = ER.worst_ratio(got, ry, ref['bound'][:N]), ER.worst_ratio(gn, rn, ref['norm_bound'][:N])
        wy, wn = max(wy, a), max(wn, b)
        if not (a <= 1 and b <= 1):
            bad.append('N=%d: unit rows %.3g, norms %.3g of their bounds' % (N, a, b))
        if not (torch.equal(torch.isnan(got), torch.isnan(ry)) and torch.equal(torch.isnan(gn), torch.isnan(rn))):
            bad.append('N=%d: the NaN entries are not those of the reference (a row with a NaN is a row of NaNs)' % N)
        zero = torch.nonzero(rn == 0).flatten()
        if not (got[zero] == 0).all():
            bad.append('N=%d: a zero row does not come out as a zero row' % N)
        tiny = torch.nonzero((rn > 0) & (rn < ER.EPS)).flatten()
        if tiny.numel() and not bool(((got[tiny].to(F64) - xs[tiny].to(F64) / eps32).abs() <= ER.U24 * got[tiny].to(F64).abs()).all()):
            bad.append('N=%d: a row below eps does not come out as x / eps' % N)
        if not (y.intact() and norm.intact()):
            bad.append('N=%d: guard rows or foreign columns changed' % N)
        if N >= 530:
            t0, t1, t2 = info['trio']
            if not (torch.equal(_bits(got[t0]), _bits(got[t1])) and torch.equal(_bits(got[t0]), _bits(got[t2]))):
                bad.append('N=%d: the power-of-two scaled trio does not come out as one unit row' % N)
            assert int(zero.numel()) >= 2 and int(tiny.numel()) >= 1
        # a second call, a call without norm, and in place: the same bits
        y2, _ = _unit(dev, xs)
        bare, _ = _unit(dev, xs, want_norm=False)
        inp = Rows(N, H, dev)
        inp.v.copy_(xs)
        _call('mgv_row_unit', H, N, _ptr(inp.v), inp.ld, ER.EPS, _ptr(inp.v), inp.ld, None)
        for tag, o in (('a second call', y2), ('norm = NULL', bare), ('in place', inp)):
            if not torch.equal(_bits(o.parent), _bits(y.parent)):
                bad.append('N=%d: %s gives other bits' % (N, tag))
    print('SIM row_unit H=%d sizes %s | unit rows %.2g/1 | norms %.2g/1 | %d findings' % (H, ER.unit_sizes(H), wy, wn, len(bad)))
    assert not bad, bad[:10]


def test_row_unit_refusals_and_no_rows():
    dev = _dev()
    n = 40
    x48, x = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)

    def rc(H, N, src, ldx, ldy=24, xp=None, yp=None):
        y, norm = Rows(n, 16, dev), Out(n, 1, dev)
        code = _rc('mgv_row_unit', H, N, _ptr(src) if xp is None else xp, ldx, 1e-8, _ptr(y.v) if yp is None else yp(y), ldy, _ptr(norm.v))
        return code, y.untouched() and norm.untouched()
    assert rc(48, n, x48, 48) == (MGV_EUNSUPPORTED, True)
    assert rc(0, n, x, 16) == (MGV_EUNSUPPORTED, True)
    assert rc(48, -1, x48, 12) == (MGV_EUNSUPPORTED, True)                         # the width comes first
    assert rc(16, -1, x, 16) == (MGV_EINVAL, True)
    assert rc(16, n, x, 12) == (MGV_EINVAL, True)                                  # row stride below H
    assert rc(16, n, x, 18) == (MGV_EINVAL, True)                                  # row stride no multiple of 4
    assert rc(16, n, x, 16, ldy=12) == (MGV_EINVAL, True)
    assert rc(16, n, x, 16, ldy=22) == (MGV_EINVAL, True)
    assert rc(16, n, x, 16, xp=TP._hip().ptr(x.view(-1)[1:])) == (MGV_EINVAL, True)               # base not 16-byte aligned
    assert rc(16, n, x, 16, yp=lambda y: TP._hip().ptr(y.parent.view(-1)[5:])) == (MGV_EINVAL, True)
    assert rc(16, n, x, 16, xp=0) == (MGV_EINVAL, True) and rc(16, n, x, 16, yp=lambda y: None) == (MGV_EINVAL, True)
    assert rc(16, 0, x, 16) == (0, True)                                           # nothing is launched
    assert rc(16, n, x, 16) == (0, False)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.row_unit(x48)
    y, norm = ops.row_unit(x, want_norm=True)
    assert y.shape == x.shape and norm.shape == (n,) and not y.requires_grad
    assert float((y.norm(dim=1) - 1).abs().max()) < 1e-5 and float((norm - x.norm(dim=1)).abs().max()) < 1e-4
    assert ops.row_unit(torch.zeros(0, 16, device=dev)).shape == (0, 16)
    # a strided view of st-like storage goes in as it is; the result is the contiguous one's
    wide = torch.randn(n, 32, device=dev)
    assert torch.equal(ops.row_unit(wide[:, 16:]), ops.row_unit(wide[:, 16:].contiguous()))


# ------------------------------------------------------------------------------------------------ the symmetric selection
class SimRun:
    """One count / scan / fill through the raw ABI on a strided operand; every output an Out of the test's own."""

    def __init__(self, dev, y, gp, thr, with_score=True, row_ptr=None, cap=None, slots=None):
        N, H = y.shape
        self.yv, ldy = _slice(y, dev)
        self.gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        self.args = (H, N, _ptr(self.yv), ldy, _ptr(self.gpd), 0 if gp is None else len(gp) - 1, float(thr))
        self.n_sel = Out(N, 1, dev, dtype=I32)
        _call('mgv_sim_select_count', *self.args, _ptr(self.n_sel.v))
        self.true_ptr = torch.zeros(N + 1, dtype=I64, device=dev)
        self.true_ptr[1:] = torch.cumsum(self.n_sel.v.flatten().to(I64), 0)
        self.total = int(self.true_ptr[-1])
        self.row_ptr = self.true_ptr if row_ptr is None else row_ptr.to(device=dev, dtype=I64).contiguous()
        self.cap = self.total if cap is None else cap
        slots = self.total if slots is None else slots      # the buffers' real size: never below what any row_ptr / cap may reach
        self.col, self.score = Out(slots, 1, dev, dtype=I32), (Out(slots, 1, dev) if with_score else None)
        self.fill()

    def fill(self):
        _call('mgv_sim_select_fill', *self.args, _ptr(self.row_ptr), self.cap, _ptr(self.col.v),
              None if self.score is None else _ptr(self.score.v))

    def intact(self):
        return self.n_sel.intact() and self.col.intact() and (self.score is None or self.score.intact())

    def lists(self):
        k = self.total
        return self.row_ptr.cpu(), self.col.v.flatten()[:k].cpu(), None if self.score is None else self.score.v.flatten()[:k].cpu()


@pytest.mark.parametrize('H', HS)
def test_sim_select_equals_the_upper_triangle_of_the_dense_matrix(H):
    """The three cases (graphs of (1, 2, 63, 64, 65, 130, 5, 200) nodes; graphs without nodes; one graph with a NaN row, graph_ptr
    NULL), thresholds 0.999, 0.25, 0.0, -2 and 1.5."""
    dev = _dev()
    bad, totals = [], []
    for kind in ER.CASES:
        c, _ = _case(H, 1, kind)
        gp, N = c['graph_ptr'], c['N']
        y, dense = _device_rows(H, 1, kind)
        nan = torch.isnan(dense)
        if not (torch.equal(nan, nan.T) and torch.equal(_bits(dense)[~nan], _bits(dense.T.contiguous())[~nan])):
            bad.append('%s: the dense scores of (y, y) differ from their transpose in bits' % kind)
        assert (kind == 'nan') == bool(nan.any())
        um = ER.upper_mask(N, gp)
        hi = PR.row_range(gp, N)[1]
        for thr in ER.THRESHOLDS:
            tag = '%s H=%d thr=%g' % (kind, H, thr)
            run = SimRun(dev, y, gp, thr)
            row_ptr, col, score = run.lists()
            bad += ['%s: %s' % (tag, b) for b in ER.check_upper(row_ptr, col, score, dense, gp, thr)]
            if not run.intact():
                bad.append('%s: guard rows changed' % tag)
            totals.append(run.total)
            n = run.n_sel.v.flatten().cpu().to(I64)
            if thr == -2.0:
                if not torch.equal(n, (um & ~nan).sum(1)):
                    bad.append('%s: n_sel is not the number of upper candidates' % tag)
                if kind != 'nan' and not torch.equal(n, hi - torch.arange(N) - 1):
                    bad.append('%s: n_sel[u] is not hi(u) - u - 1' % tag)
            if thr == 1.5 and not (run.total == 0 and run.col.untouched() and run.score.untouched()):
                bad.append('%s: something is above 1.5' % tag)
            # the lists with their transposes: the general entries on (y, y) without self
            gen = TS.Run(dev, y, y, gp, False, thr, True)
            g_ptr, g_col, g_score = gen.lists()
            b_ptr, b_col = ER.both_sides(row_ptr, col, N)
            if not (torch.equal(b_ptr, g_ptr) and torch.equal(b_col, g_col.to(I64))):
                bad.append('%s: the lists and their transposes are not mgv_pair_select_* on (y, y, skip_self)' % tag)
            elif run.total:
                rows = torch.repeat_interleave(torch.arange(N), g_ptr[1:] - g_ptr[:-1])
                up = g_col.to(I64) > rows
                if not torch.equal(_bits(g_score[up]), _bits(score)):
                    bad.append('%s: a cosine differs in bits from the general entry\'s' % tag)
            # two fills give the same bytes; score = NULL leaves col as it is
            first = (_bits(run.col.parent), _bits(run.score.parent))
            run.col.parent.fill_(-77)
            run.score.parent.fill_(NAN)
            run.fill()
            if not (torch.equal(first[0], _bits(run.col.parent)) and torch.equal(first[1], _bits(run.score.parent))):
                bad.append('%s: a second fill gives other bytes' % tag)
            if not torch.equal(SimRun(dev, y, gp, thr, with_score=False).col.parent, run.col.parent):
                bad.append('%s: col changes when no scores are asked for' % tag)
        if kind == 'sim':
            info = c['info']
            run = SimRun(dev, y, gp, 0.999)
            row_ptr, col, _ = run.lists()
            rows = torch.repeat_interleave(torch.arange(N), row_ptr[1:] - row_ptr[:-1])
            t0, t1, t2 = info['trio']
            want = sorted([(t0, t1), (t0, t2), (t1, t2), (t0, info['near']), (t1, info['near']), (t2, info['near']), info['scaled']])
            if list(zip(rows.tolist(), col.tolist())) != want:
                bad.append('H=%d: the pairs above 0.999 are not the 7 planted ones: %s' % (H, list(zip(rows.tolist(), col.tolist()))))
    print('SIM exact H=%d | pairs per configuration %d .. %d | %d findings' % (H, min(totals), max(totals), len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', HS)
def test_sim_select_against_float64(H):
    """Seeds 1 - 3 of the three cases, all five thresholds, no exclusions: an emitted pair has cos + bound > thr, every other upper
    candidate cos - bound <= thr, with cos_ref of the case's float32 rows and its bound (2H + 6) 2^-24 S."""
    dev = _dev()
    bad, band, pairs = [], 0, 0
    for seed in SEEDS:
        for kind in ER.CASES:
            c, r = _case(H, seed, kind)
            gp, N = c['graph_ptr'], c['N']
            y, _ = _device_rows(H, seed, kind)
            mask = ER.upper_mask(N, gp)
            for thr in ER.THRESHOLDS:
                near = ER.band_count(r['cos'], r['bound'], thr, mask)
                band = max(band, near)
                assert near <= ER.band_limit(mask), (seed, kind, thr, near)
                run = SimRun(dev, y, gp, thr, with_score=False)
                row_ptr, col, _ = run.lists()
                pairs += run.total
                bad += ['seed %d %s thr=%g: %s' % (seed, kind, thr, b) for b in ER.check_upper_band(row_ptr, col, r['cos'], r['bound'], gp, thr)]
    print('SIM float64 H=%d | %d pairs checked, every candidate on its side of its bound | at most %d pairs inside their bound of a '
          'threshold | %d findings' % (H, pairs, band, len(bad)))
    assert not bad, bad[:10]


def test_the_fill_stays_inside_the_slots_it_is_given():
    dev = _dev()
    c, _ = _case(64)
    gp = c['graph_ptr']
    y, _ = _device_rows(64)
    thr = 0.1
    full = SimRun(dev, y, gp, thr)
    true_ptr, want_col, want_score = full.lists()
    n = true_ptr[1:] - true_ptr[:-1]
    total = full.total
    u = int(torch.argmax(n[:-1] * (n[1:] > 0)))             # the longest list that has a non-empty successor
    short = 5
    assert int(n[u]) > 16 + short
    # one row gets fewer slots than it selects: it writes its first entries only, everything else is where it was
    row_ptr = true_ptr.clone()
    row_ptr[u + 1:] -= int(n[u]) - short
    run = SimRun(dev, y, gp, thr, row_ptr=row_ptr, slots=total)
    keep = torch.ones(total, dtype=torch.bool)
    keep[int(true_ptr[u]) + short:int(true_ptr[u + 1])] = False
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    used = int(keep.sum())
    assert torch.equal(got_col[:used], want_col[keep]) and torch.equal(_bits(got_score[:used]), _bits(want_score[keep]))
    assert bool((got_col[used:] == -77).all()) and bool(torch.isnan(got_score[used:]).all()) and run.intact()
    # no row has a slot; descending or negative entries; entries beyond the buffers: nothing is written
    for odd in (torch.zeros_like(true_ptr), true_ptr.flip(0), true_ptr - total - 7, torch.full_like(true_ptr, total + 1000)):
        run = SimRun(dev, y, gp, thr, row_ptr=odd, slots=total)
        assert run.col.untouched() and run.score.untouched()
    # cap below the total: nothing at or behind cap
    cap = int(true_ptr[u]) + 3                              # ends inside row u's list
    run = SimRun(dev, y, gp, thr, cap=cap, slots=total)
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    assert torch.equal(got_col[:cap], want_col[:cap]) and torch.equal(_bits(got_score[:cap]), _bits(want_score[:cap]))
    assert bool((got_col[cap:] == -77).all()) and bool(torch.isnan(got_score[cap:]).all()) and run.intact()
    run = SimRun(dev, y, gp, thr, cap=0, slots=total)
    assert run.col.untouched() and run.score.untouched()
    print('SIM fill bounds | row %d of %d pairs cut to %d, odd row_ptr, cap %d of %d | ok' % (u, int(n[u]), short, cap, total))


def test_sim_select_refusals_are_return_codes_before_anything_is_launched():
    dev = _dev()
    n = 40
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    ptr0 = torch.arange(0, 4 * (n + 1), 4, dtype=I64, device=dev)

    def both(H, N, x, ld, gp, cap=None, base=None):
        """(count's code, fill's code, every output untouched)"""
        n_sel, col, score = Out(n, 1, dev, dtype=I32), Out(4 * n, 1, dev, dtype=I32), Out(4 * n, 1, dev)
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        common = (H, N, _ptr(x) if base is None else base, ld, _ptr(gpd), 0 if gp is None else len(gp) - 1, -2.0)
        a = _rc('mgv_sim_select_count', *common, _ptr(n_sel.v))
        b = _rc('mgv_sim_select_fill', *common, _ptr(ptr0), 4 * n if cap is None else cap, _ptr(col.v), _ptr(score.v))
        return a, b, n_sel.untouched() and col.untouched() and score.untouched()
    assert both(48, n, y48, 48, None) == (MGV_EUNSUPPORTED, MGV_EUNSUPPORTED, True)
    assert both(0, n, y, 16, None) == (MGV_EUNSUPPORTED, MGV_EUNSUPPORTED, True)
    assert both(16, n, y, 12, None) == (MGV_EINVAL, MGV_EINVAL, True)             # row stride below H
    assert both(16, n, y, 18, None) == (MGV_EINVAL, MGV_EINVAL, True)             # row stride no multiple of 4
    assert both(16, n, y, 16, None, base=TP._hip().ptr(y.view(-1)[1:])) == (MGV_EINVAL, MGV_EINVAL, True)      # base not 16-byte aligned
    assert both(16, 2 ** 31, y, 16, None) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, -1, y, 16, None) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, n, y, 16, [0, 10, n - 1]) == (MGV_EINVAL, MGV_EINVAL, True)   # does not end at N
    assert both(16, n, y, 16, [0, 10, n + 1]) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, n, y, 16, [1, 10, n]) == (MGV_EINVAL, MGV_EINVAL, True)       # does not start at 0
    assert both(16, n, y, 16, None, cap=-1) == (0, MGV_EINVAL, False)             # the count ran
    n_sel, col, score = Out(n, 1, dev, dtype=I32), Out(4 * n, 1, dev, dtype=I32), Out(4 * n, 1, dev)
    assert _rc('mgv_sim_select_fill', 16, n, _ptr(y), 16, None, 0, -2.0, _ptr(ptr0), -1, _ptr(col.v), _ptr(score.v)) == MGV_EINVAL
    assert col.untouched() and score.untouched()
    assert both(16, n, y, 16, [0, 10, n]) == (0, 0, False)
    # N = 0: nothing is launched, nothing is written
    empty = torch.full((1, 16), NAN, device=dev)
    for gpd, G in ((None, 0), (torch.zeros(1, dtype=I32, device=dev), 0), (torch.zeros(3, dtype=I32, device=dev), 2)):
        _call('mgv_sim_select_count', 16, 0, _ptr(empty), 16, _ptr(gpd), G, 0.5, _ptr(n_sel.v))
        _call('mgv_sim_select_fill', 16, 0, _ptr(empty), 16, _ptr(gpd), G, 0.5, _ptr(ptr0), 0, _ptr(col.v), None)
        assert n_sel.untouched() and col.untouched()
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.sim_pairs(y, graph_ptr=[0, 10, n - 1])
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.sim_pairs(y48)
    pi, row_ptr, score = ops.sim_pairs(torch.zeros(0, 16, device=dev), graph_ptr=[0], with_scores=True)
    assert pi.shape == (2, 0) and pi.dtype == I64 and row_ptr.tolist() == [0] and score.shape == (0,)


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize('H', HS)
def test_sim_topk_pairs_and_at_report_one_cosine(H):
    """ops.sim_topk against float64 of the device's unit rows (PR.check_topk, no exclusions); its cosines are the bits of ops.sim_at and
    of ops.sim_pairs for the same pair; n_above counts a pair from both of its nodes."""
    dev = _dev()
    from deepgate import ops
    c, _ = _case(H)
    gp, N = c['graph_ptr'], c['N']
    xd = c['x'].to(dev)
    y = ops.row_unit(xd)
    assert torch.equal(_bits(y), _bits(_device_rows(H)[0]))
    k, thr = 8, 0.25
    idx, cos, n_above = ops.sim_topk(xd, k, graph_ptr=gp, threshold=thr)
    assert idx.dtype == I32 and idx.shape == (N, k) and cos.shape == (N, k) and n_above.dtype == I32 and idx.is_cuda
    r = PR.scores_ref(y.cpu(), y.cpu())
    bad = PR.check_topk(idx.cpu(), cos.cpu(), r, gp, k, True, False)
    pi, row_ptr, score = ops.sim_pairs(xd, graph_ptr=gp, threshold=thr, with_scores=True)
    assert pi.dtype == I64 and pi.shape[0] == 2 and bool((pi[0] < pi[1]).all()) and row_ptr.dtype == I64 and score.dtype == F32
    assert ops.sim_pairs(xd, graph_ptr=gp, threshold=thr)[2] is None
    assert ER.check_upper(row_ptr, pi[1], score, _device_rows(H)[1], gp, thr) == []
    assert torch.equal(_bits(ops.sim_at(xd, pi)), _bits(score)) and torch.equal(_bits(ops.sim_at(xd, pi.flip(0))), _bits(score))
    # the top-k cosines: the bits of sim_at, and of sim_pairs wherever the pair is listed there
    rows = torch.arange(N, device=dev)[:, None].expand(N, k)
    have = idx >= 0
    listed = torch.stack([rows[have], idx[have].long()])
    assert torch.equal(_bits(ops.sim_at(xd, listed)), _bits(cos[have]))
    where = {(int(a), int(b)): int(s) for a, b, s in zip(pi[0].tolist(), pi[1].tolist(), _bits(score).tolist())}
    shared = 0
    for a, b, s in zip(listed[0].tolist(), listed[1].tolist(), _bits(cos[have]).tolist()):
        key = (min(a, b), max(a, b))
        if key in where:
            shared += 1
            if where[key] != s:
                bad.append('pair %s: sim_topk and sim_pairs report other bits' % (key,))
    assert shared >= 14                                     # at least the seven planted pairs, from both of their nodes
    # n_above is symmetric: a pair above the threshold counts for both of its nodes
    both = torch.zeros(N, dtype=I64).index_add_(0, pi.cpu().flatten(), torch.ones(2 * pi.shape[1], dtype=I64))
    if not torch.equal(n_above.cpu().to(I64), both):
        bad.append('n_above is not the number of listed pairs a node is in')
    # planted: the trio's members find each other first, the zero rows find only zeros, the border copy is never listed
    t0, t1, t2 = c['info']['trio']
    near = c['info']['near']
    if sorted(idx[t0, :3].tolist()) != sorted([t1, t2, near]):
        bad.append('row %d: its three closest are not the trio and the near-duplicate: %s' % (t0, idx[t0].tolist()))
    z = c['info']['zeros'][0]
    if bool(cos[z].any()) or int(n_above[z]) != 0:
        bad.append('a zero row has a cosine that is not 0')
    last, nxt = c['info']['border']
    if nxt in idx[last].tolist() or last in idx[nxt].tolist():
        bad.append('the copy across the graph border is listed')
    print('SIM surface H=%d | %d pairs above %g, %d of them among the top-%d lists | %d findings' % (H, pi.shape[1], thr, shared, k, len(bad)))
    assert not bad, bad[:10]


def test_sim_pairs_refuses_before_the_fill():
    dev = _dev()
    from deepgate import _hip, ops
    c, _ = _case(64)
    xd = c['x'].to(dev)
    total = ops.sim_pairs(xd, graph_ptr=c['graph_ptr'], threshold=0.25)[0].shape[1]
    calls = []
    real = _hip.call
    try:
        _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        with pytest.raises(_hip.HipLibraryError, match=str(total)) as err:
            ops.sim_pairs(xd, graph_ptr=c['graph_ptr'], threshold=0.25, max_pairs=total - 1)
    finally:
        _hip.call = real
    assert 'mgv_sim_select_count' in calls and 'mgv_sim_select_fill' not in calls
    assert 'sim_topk' in str(err.value) and 'threshold' in str(err.value)
    assert ops.sim_pairs(xd, graph_ptr=c['graph_ptr'], threshold=0.25, max_pairs=total)[0].shape[1] == total


def test_the_model_methods_on_a_small_batch():
    """3 graphs of 300 nodes: equivalence_candidates, similar_gates and functional_similarity on the model's own hf; 1 - cosine of the
    truth-table pairs against dis of mgv_func_loss_fwd on the same hf, within the two float32 bounds added."""
    dev = _dev()
    import deepgate
    from deepgate import _hip, ops, synthetic as syn
    H = 64
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev).eval()
    graphs = [syn.make_graph('aig', 300, 12, 50 + i, n_inputs=24) for i in range(3)]
    batch = deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)
    with torch.no_grad():
        _, hf = model(batch)
    N, gp = hf.shape[0], batch.graph_ptr.tolist()
    assert N == 900 and gp == [0, 300, 600, 900]
    y = ops.row_unit(hf)
    dense = ops.pair_scores(y, y, sigmoid=False).cpu()
    inputs = torch.nonzero(hf.abs().sum(1) == 0).flatten().cpu()
    assert inputs.numel() >= 3 * 24                          # the primary inputs are never updated: hf = 0
    # equivalence candidates
    pi, row_ptr, cos = model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, with_scores=True)
    assert ER.check_upper(row_ptr, pi[1], cos, dense, gp, 0.999) == []
    assert bool((pi[0] < pi[1]).all()) and bool((pi[0] // 300 == pi[1] // 300).all()) and not bool(torch.isin(pi.cpu(), inputs).any())
    assert model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr)[2] is None
    loose = model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=0.5)[0].shape[1]
    assert loose >= pi.shape[1]
    with pytest.raises(_hip.HipLibraryError, match='max_pairs'):
        model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=-2.0, max_pairs=1000)
    # similar gates
    idx, sc, n_above = model.similar_gates(hf, 4, graph_ptr=batch.graph_ptr)
    want = ops.sim_topk(hf, 4, graph_ptr=gp)                 # (held to float64 by the test above)
    assert torch.equal(idx, want[0]) and torch.equal(_bits(sc), _bits(want[1])) and torch.equal(n_above, want[2])
    listed = torch.stack([torch.arange(N, device=dev)[:, None].expand(N, 4)[idx >= 0], idx[idx >= 0].long()])
    assert torch.equal(_bits(model.functional_similarity(hf, listed)), _bits(sc[idx >= 0]))
    both = torch.zeros(N, dtype=I64).index_add_(0, pi.cpu().flatten(), torch.ones(2 * pi.shape[1], dtype=I64))
    assert torch.equal(n_above.cpu().to(I64), both)
    # functional similarity against the loss's own distance
    pairs, tt = batch['tt_pair_index'], batch['tt_sim']
    P = pairs.shape[1]
    got = model.functional_similarity(hf, pairs)
    pa, pb = pairs[0].contiguous(), pairs[1].contiguous()
    dis = torch.empty(P, dtype=F32, device=dev)
    ws = torch.zeros(8, dtype=F64, device=dev)
    _hip.call('mgv_func_loss_fwd', H, P, _ptr(hf.contiguous()), _ptr(pa), _ptr(pb), _ptr(tt.to(F32).contiguous()), 1e-8, _ptr(dis), _ptr(ws),
              *ops._sw(dev))
    ref = LR.func(hf.cpu(), pairs.cpu(), tt.cpu())
    cr = ER.cos_ref(hf.cpu())
    a, b = pairs[0].cpu(), pairs[1].cpu()
    bound = ref['bound_dis'] + cr['bound'][a, b]
    err = ((1 - got.cpu().to(F64)) - dis.cpu().to(F64)).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    w64 = ER.worst_ratio(got.cpu(), cr['cos'][a, b], cr['bound'][a, b])
    print('SIM model N=%d | %d pairs above 0.999, %d above 0.5 | 1 - cos against the loss\'s dis %.2g/1 of the two bounds added | cos '
          'against float64 %.2g/1' % (N, pi.shape[1], loose, worst, w64))
    assert worst <= 1 and w64 <= 1


def test_feature_extract_similar_and_equivalences(tmp_path):
    """examples/feature_extract.py --similar K --equivalences THR: name/sim_idx and name/sim_cos, name/eq_pairs and name/eq_cos with
    ids local to the graph, beside the embeddings."""
    _dev()
    import importlib

    import numpy as np
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '2', '--rounds', '1', '--batch_size', '2', '--similar', '4', '--equivalences', '0.999',
             '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(2) for k in ('hs', 'hf', 'sim_idx', 'sim_cos', 'eq_pairs',
                                                                                       'eq_cos'))
    for i in range(2):
        n = emb['graph%d/hf' % i].shape[0]
        idx, cos = emb['graph%d/sim_idx' % i], emb['graph%d/sim_cos' % i]
        assert idx.shape == (n, 4) and cos.shape == (n, 4) and idx.dtype == np.int32
        assert idx.min() >= -1 and idx.max() < n and (idx != np.arange(n)[:, None]).all()
        assert (np.diff(cos, axis=1) <= 0).all()
        eq, ec = emb['graph%d/eq_pairs' % i], emb['graph%d/eq_cos' % i]
        assert eq.ndim == 2 and eq.shape[0] == 2 and eq.dtype == np.int32 and ec.shape == (eq.shape[1],)
        if eq.shape[1]:
            assert eq.min() >= 0 and eq.max() < n and (eq[0] < eq[1]).all() and (ec > 0.999).all()
            key = eq[0].astype(np.int64) * n + eq[1]
            assert (np.diff(key) > 0).all()                                    # per smaller id, ascending, no pair twice
