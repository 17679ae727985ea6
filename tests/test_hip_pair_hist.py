"""The score-distribution entries of csrc/pair_scores.hip — mgv_pair_hist, mgv_sim_hist — through the C ABI and through the surface
(ops.pair_profile / sim_profile / counts_above / reconstruction_curve / sim_threshold_for, Model.similarity_profile /
equivalence_threshold / reconstruction_curve, the decoder's and DirectedGAE's reconstruction_curve, examples/feature_extract.py
--similarity_profile / --equivalences_max / --recon_curve), against tests/pair_hist_ref.py (pinned on the CPU by
tests/test_pair_hist_spec.py, which also shows the planted defects of a restated walk to change the bins compared here).

Exact, as integers: the bins equal the CPU binning of the device's own dense scores (mgv_pair_scores_fwd on the same operands) under the
reference's masks; counts_above equals the per-graph sums of n_sel of mgv_pair_select_count / mgv_sim_select_count at every edge; a
graph's bins sum to its candidates that are no NaN; two calls give the same bytes; hist filled with garbage is overwritten; the rows
behind hist are untouched.  Against float64 (ER.cos_ref): the count above an edge differs from the reference's by at most the pairs
inside their bound of that edge, after that band has been held to ER.band_limit.

Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold NaN; hist has 64
guard rows behind it and holds -77 before the call.  Every check prints one line `HIST <what> | figures`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import pair_hist_ref as HR  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402
import test_hip_embed_sim as TE  # noqa: E402  (the device's own unit rows of the similarity cases)
import test_hip_pair_scores as TP  # noqa: E402  (the operand slices and the launcher helpers of the pair-score tests)

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
GUARD = TP.GUARD
FILL = -77
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
_dev, _ptr, _rc, _call, _slice = TP._dev, TP._ptr, TP._rc, TP._call, TP._slice
SYM_KINDS = ('sim', 'empty_middle', 'nan', 'many')
SYM_TABLES = ('A', 'B', 'D', 'one', 'wide')
GEN_TABLES = ('A', 'D', 'wide')
GEN_MODES = ((True, False), (False, True))                 # (sigmoid, skip_self)


class Hist:
    """int64 [max(G, 1)][B + 1] with GUARD rows behind it, -77 everywhere before the call."""

    def __init__(self, G, B, dev):
        self.rows = max(G, 1)
        self.parent = torch.full((self.rows + GUARD, B + 1), FILL, dtype=I64, device=dev)
        self.v = self.parent[:self.rows]

    def intact(self):
        return bool((self.parent[self.rows:] == FILL).all())

    def untouched(self):
        return bool((self.parent == FILL).all())


class Walk:
    """The operands of one case on the device (strided), and both entries and their count yardsticks on them."""

    def __init__(self, dev, s, t, gp, sym):
        self.dev, self.sym, self.gp = dev, sym, gp
        self.N, self.H = s.shape
        self.sv, self.lds = _slice(s, dev)
        self.tv, self.ldt = (self.sv, self.lds) if sym else _slice(t, dev)
        self.gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        self.G = 0 if gp is None else len(gp) - 1
        gid, self.rows = HR.graph_ids(gp, self.N)
        self.gid = gid.to(dev)

    def hist(self, table, sigmoid=False, skip=False, out=None):
        e = HR.edges_f32(table).to(self.dev)
        h = Hist(self.G, e.numel(), self.dev) if out is None else out
        if self.sym:
            _call('mgv_sim_hist', self.H, self.N, _ptr(self.sv), self.lds, _ptr(self.gpd), self.G, _ptr(e), e.numel(), _ptr(h.v))
        else:
            _call('mgv_pair_hist', self.H, self.N, _ptr(self.sv), self.lds, _ptr(self.tv), self.ldt, _ptr(self.gpd), self.G, int(sigmoid),
                  int(skip), _ptr(e), e.numel(), _ptr(h.v))
        return h

    def select_totals(self, table, sigmoid=False, skip=False):
        """int64 [rows, B]: per graph, the sum of n_sel of the count entry at threshold = every edge."""
        e = HR.edges_f32(table)
        out = torch.zeros((self.rows, e.numel()), dtype=I64, device=self.dev)
        if self.N == 0:
            return out.cpu()
        n_sel = torch.full((self.N,), FILL, dtype=I32, device=self.dev)
        for j, thr in enumerate(e.tolist()):
            if self.sym:
                _call('mgv_sim_select_count', self.H, self.N, _ptr(self.sv), self.lds, _ptr(self.gpd), self.G, thr, _ptr(n_sel))
            else:
                _call('mgv_pair_select_count', self.H, self.N, _ptr(self.sv), self.lds, _ptr(self.tv), self.ldt, _ptr(self.gpd), self.G,
                      int(sigmoid), thr, int(skip), _ptr(n_sel))
            out[:, j].index_add_(0, self.gid, n_sel.to(I64))
        return out.cpu()


@functools.lru_cache(maxsize=None)
def _many(H):
    return HR.many_graphs_case(H, 1)


@functools.lru_cache(maxsize=None)
def _sym_case(H, kind):
    """(case, the device's own unit rows on the host, their dense scores on the host)."""
    dev = _dev()
    if kind in ER.CASES:
        c, _ = TE._case(H, 1, kind)
        y, dense = TE._device_rows(H, 1, kind)
        return c, y, dense
    c = _many(H)
    y = TE._unit(dev, c['x'], want_norm=False)[0].v.cpu().contiguous()
    return c, y, TP._fwd(dev, y, y, False)[0].v.cpu()


@functools.lru_cache(maxsize=None)
def _gen_case(H, kind):
    c = SR.select_case(H, 1) if kind == 'select' else _many(H)
    return c


def _exact(tag, walk, dense, table, sigmoid=False, skip=False, yardstick=True):
    """Every exact check of one (case, table) -> (findings, the bins on the host)."""
    bad = []
    h = walk.hist(table, sigmoid, skip)
    got = h.v.cpu()
    want = HR.brute_hist(dense, walk.gp, table, walk.sym, skip)
    if not torch.equal(got, want):
        d = torch.nonzero(got != want)
        bad.append('%s: %d bins differ from the binning of the dense scores, first [g=%d, k=%d]: %d, expected %d'
                   % (tag, d.shape[0], int(d[0, 0]), int(d[0, 1]), int(got[tuple(d[0])]), int(want[tuple(d[0])])))
    if not h.intact():
        bad.append('%s: the rows behind hist changed' % tag)
    cand = HR.mask_of(walk.N, walk.gp, walk.sym, skip) & ~torch.isnan(dense)
    per_graph = torch.zeros(walk.rows, dtype=I64).index_add_(0, walk.gid.cpu(), cand.sum(1))
    if not torch.equal(got.sum(1), per_graph):
        bad.append('%s: a graph\'s bins do not sum to its candidates that are no NaN' % tag)
    if yardstick and not torch.equal(HR.counts_above(got), walk.select_totals(table, sigmoid, skip)):
        bad.append('%s: counts_above differs from the count entry\'s totals at an edge' % tag)
    first = h.parent.clone()
    walk.hist(table, sigmoid, skip, out=h)                  # onto its own result: overwritten, not added to
    if not torch.equal(h.parent, first):
        bad.append('%s: a second call gives other bytes' % tag)
    return bad, got


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('H', HS)
def test_sim_hist_equals_the_binning_of_the_dense_cosines_and_the_count_entry(H):
    """sim_case and empty_middle_case at seed 1, nan_case (graph_ptr NULL), 64 graphs of 1 to 3 nodes; tables A, B, D, (0.999,) and the
    256-edge table (the last against the dense scores only: 256 count walks per case say nothing new)."""
    dev = _dev()
    bad, pairs = [], 0
    for kind in SYM_KINDS:
        c, y, dense = _sym_case(H, kind)
        walk = Walk(dev, y, y, c['graph_ptr'], True)
        for table in SYM_TABLES:
            b, got = _exact('%s H=%d table %s' % (kind, H, table), walk, dense, table, yardstick=table != 'wide')
            bad += b
            pairs = max(pairs, int(got.sum()))
        if kind == 'sim':
            above = HR.counts_above(walk.hist('one').v.cpu())
            if int(above.sum()) != 7:
                bad.append('H=%d: %d pairs above 0.999, the case plants 7' % (H, int(above.sum())))
            d = walk.hist('D').v.cpu()
            if int(d[:, 0].sum()) or int(d[:, 3].sum()) or int(d[:, 1].sum()) < 64:
                bad.append('H=%d table D: something at or below -2 or above 1.5, or the zero rows\' cosines are not in bin 1' % H)
    print('HIST sim exact H=%d | %d cases x %d tables, up to %d pairs per case | %d findings' % (H, len(SYM_KINDS), len(SYM_TABLES), pairs, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', HS)
def test_pair_hist_equals_the_binning_of_the_dense_scores_and_the_count_entry(H):
    """select_case at seed 1 with its graphs and as one graph, and 64 graphs of 1 to 3 nodes; the sigmoid with self, raw without."""
    dev = _dev()
    bad, pairs = [], 0
    for kind in ('select', 'many'):
        c = _gen_case(H, kind)
        for sigmoid, skip in GEN_MODES:
            dense = TP._fwd(dev, c['s'], c['t'], sigmoid)[0].v.cpu()
            for gp in (c['graph_ptr'], None):
                walk = Walk(dev, c['s'], c['t'], gp, False)
                for table in GEN_TABLES:
                    tag = '%s H=%d sigmoid=%s skip_self=%s graphs=%s table %s' % (kind, H, sigmoid, skip, gp is not None, table)
                    b, got = _exact(tag, walk, dense, table, sigmoid, skip, yardstick=table != 'wide' and gp is not None)
                    bad += b
                    pairs = max(pairs, int(got.sum()))
    print('HIST pair exact H=%d | up to %d pairs per case | %d findings' % (H, pairs, len(bad)))
    assert not bad, bad[:10]


def test_one_node_and_no_node():
    dev = _dev()
    H = 32
    x = PR._rows(1, H, torch.Generator().manual_seed(3), 1.0)
    for gp in ([0, 1], None):
        w = Walk(dev, x, x, gp, True)
        assert int(w.hist('A').v.abs().sum()) == 0                          # no pair
        g = Walk(dev, x, x, gp, False)
        raw = float(TP._fwd(dev, x, x, False)[0].v[0, 0])
        h = g.hist('D', False, False).v.cpu()
        assert h.tolist() == [[0, 0, int(raw <= 1.5), int(raw > 1.5)]] and raw > 0
        assert int(g.hist('D', False, True).v.abs().sum()) == 0             # without itself: no candidate
    # N = 0: hist is zeroed (one row for G = 0), nothing is launched
    empty = torch.full((1, H), TP.NAN, device=dev)
    e = HR.edges_f32('D').to(dev)
    for gpd, G in ((None, 0), (torch.zeros(1, dtype=I32, device=dev), 0), (torch.zeros(3, dtype=I32, device=dev), 2)):
        for sym in (True, False):
            h = Hist(G, 3, dev)
            if sym:
                _call('mgv_sim_hist', H, 0, _ptr(empty), H, _ptr(gpd), G, _ptr(e), 3, _ptr(h.v))
            else:
                _call('mgv_pair_hist', H, 0, _ptr(empty), H, _ptr(empty), H, _ptr(gpd), G, 1, 0, _ptr(e), 3, _ptr(h.v))
            assert h.intact() and h.v.shape == (max(G, 1), 4) and int(h.v.abs().sum()) == 0
    from deepgate import ops
    z = torch.zeros(0, H, device=dev)
    assert ops.sim_profile(z, HR.EDGES['D'], graph_ptr=[0]).shape == (0, 4)
    assert ops.sim_profile(z, HR.EDGES['D']).tolist() == [[0, 0, 0, 0]]
    assert ops.pair_profile(z, z, HR.EDGES['D'], graph_ptr=[0, 0, 0]).tolist() == [[0, 0, 0, 0]] * 2


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize('H', HS)
def test_sim_hist_against_float64(H):
    """Seed 1 of the three builders, tables A, B and D: per edge, the band (pairs within their bound (2H + 6) 2^-24 S of the edge) holds
    at most ER.band_limit pairs — a condition — and the device's count above the edge is within that many of cos_ref's."""
    dev = _dev()
    bad, worst_band, worst_diff = [], 0, 0
    for kind in ER.CASES:
        c, r = TE._case(H, 1, kind)
        gp, N = c['graph_ptr'], c['N']
        y, _ = TE._device_rows(H, 1, kind)
        mask = ER.upper_mask(N, gp)
        walk = Walk(dev, y, y, gp, True)
        for table in ('A', 'B', 'D'):
            got = HR.counts_above(walk.hist(table).v.cpu())
            ref = HR.counts_above(HR.brute_hist(r['cos'], gp, table, True))
            for j, thr in enumerate(HR.edges_f32(table).tolist()):
                band = ER.band_count(r['cos'], r['bound'], thr, mask)
                worst_band = max(worst_band, band)
                assert band <= ER.band_limit(mask), (kind, table, thr, band)
                diff = int((got[:, j] - ref[:, j]).abs().sum())
                worst_diff = max(worst_diff, diff)
                if diff > band:
                    bad.append('%s table %s edge %.9g: the count above differs by %d, %d pairs lie inside their bound' % (kind, table, thr, diff, band))
    print('HIST float64 H=%d | counts above an edge differ by at most %d | at most %d pairs inside their bound of an edge | %d findings'
          % (H, worst_diff, worst_band, len(bad)))
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_before_anything_is_launched_or_zeroed():
    dev = _dev()
    n = 40
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    good = torch.tensor([-0.5, 0.0, 0.5], device=dev)

    def both(H, N, x, ld, gp, edges=good, B=None, base=None, hist=True):
        """(mgv_pair_hist's code, mgv_sim_hist's code, hist untouched)"""
        B = (0 if edges is None else edges.numel()) if B is None else B
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        G = 0 if gp is None else len(gp) - 1
        h = Hist(G, 300, dev)
        xp = _ptr(x) if base is None else base
        hp = _ptr(h.v) if hist else None
        a = _rc('mgv_pair_hist', H, N, xp, ld, xp, ld, _ptr(gpd), G, 0, 0, _ptr(edges), B, hp)
        b = _rc('mgv_sim_hist', H, N, xp, ld, _ptr(gpd), G, _ptr(edges), B, hp)
        return a, b, h.untouched()
    INV, UNS = (MGV_EINVAL, MGV_EINVAL, True), (MGV_EUNSUPPORTED, MGV_EUNSUPPORTED, True)
    wide = torch.linspace(-1, 1, 257, device=dev)
    assert both(16, n, y, 16, None, B=0) == INV
    assert both(16, n, y, 16, None, edges=wide) == INV                             # B = 257
    assert both(16, n, y, 16, None, edges=wide[:256]) == (0, 0, False)             # B = 256 is served
    assert both(16, n, y, 16, None, B=-1) == INV
    assert both(16, n, y, 16, None, edges=torch.tensor([0.5, 0.0, -0.5], device=dev)) == INV      # descending
    assert both(16, n, y, 16, None, edges=torch.tensor([-0.5, 0.0, 0.0], device=dev)) == INV      # equal
    assert both(16, n, y, 16, None, edges=torch.tensor([-0.0, 0.0], device=dev)) == INV           # equal as numbers
    for at in range(3):
        e = good.clone()
        e[at] = TP.NAN
        assert both(16, n, y, 16, None, edges=e) == INV                            # a NaN edge, wherever it stands
    assert both(16, n, y, 16, None, edges=torch.tensor([TP.NAN], device=dev)) == INV
    assert both(16, n, y, 16, None, edges=None, B=3) == INV                        # NULL edges
    assert both(16, n, y, 16, None, hist=False) == INV                             # NULL hist
    assert both(48, n, y48, 48, None) == UNS
    assert both(0, n, y, 16, None) == UNS
    assert both(48, n, y48, 48, None, B=0) == UNS                                  # the width comes first
    assert both(16, n, y, 12, None) == INV                                         # a stride of H - 4
    assert both(16, n, y, 18, None) == INV                                         # row stride no multiple of 4
    assert both(16, n, y, 16, None, base=TP._hip().ptr(y.view(-1)[1:])) == INV     # base not 16-byte aligned
    assert both(16, 2 ** 31, y, 16, None) == INV
    assert both(16, -1, y, 16, None) == INV
    assert both(16, n, y, 16, [0, 10, n - 1]) == INV                               # does not end at N
    assert both(16, n, y, 16, [0, 10, n + 1]) == INV
    assert both(16, n, y, 16, [1, 10, n]) == INV                                   # does not start at 0
    assert both(16, 0, y, 16, [0, 0], edges=torch.tensor([0.5, 0.0], device=dev)) == INV          # the table is checked without rows too
    assert both(16, n, y, 16, [0, 10, n]) == (0, 0, False)
    assert both(16, n, y, 16, None, edges=torch.tensor([float('-inf'), 0.0, float('inf')], device=dev)) == (0, 0, False)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.sim_profile(y, [0.5, 0.25])
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.pair_profile(y, y, [0.1, 0.2], graph_ptr=[0, 10, n - 1])
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.sim_profile(y48, [0.5])
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.pair_profile(y48, y48, [0.5])
    with pytest.raises(_hip.HipLibraryError, match='1 to 256'):
        ops.sim_profile(y, [])
    with pytest.raises(_hip.HipLibraryError, match='1 to 256'):
        ops.sim_profile(y, wide)


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize('H', HS)
def test_the_ops_report_the_entries_bins_and_the_curve_is_the_stacked_counts(H):
    dev = _dev()
    from deepgate import ops
    # the cosine: ops.sim_profile on x is the entry on the device's unit rows
    c, y, _ = _sym_case(H, 'sim')
    gp = c['graph_ptr']
    xd = c['x'].to(dev)
    prof = ops.sim_profile(xd, HR.EDGES['B'], graph_ptr=gp)
    assert prof.dtype == I64 and prof.is_cuda and prof.shape == (len(gp) - 1, 21) and not prof.requires_grad
    assert torch.equal(prof.cpu(), Walk(dev, y, y, gp, True).hist('B').v.cpu())
    assert torch.equal(ops.sim_profile(xd, torch.tensor(HR.EDGES['B'], dtype=F64), graph_ptr=torch.tensor(gp)), prof)
    assert torch.equal(ops.counts_above(prof).cpu(), HR.counts_above(prof.cpu())) and ops.counts_above(prof).shape == (len(gp) - 1, 20)
    assert ops.sim_profile(xd, (0.999,)).shape == (1, 2)
    # the decoder: ops.pair_profile, and the curve against reconstruction_counts threshold by threshold
    c = _gen_case(H, 'select')
    gp = c['graph_ptr']
    sd, td = c['s'].to(dev), c['t'].to(dev)
    for sigmoid, skip in GEN_MODES:
        prof = ops.pair_profile(sd, td, HR.EDGES['A'], graph_ptr=gp, sigmoid=sigmoid, skip_self=skip)
        assert torch.equal(prof.cpu(), Walk(dev, c['s'], c['t'], gp, False).hist('A', sigmoid, skip).v.cpu())
    ei = PR.edges_case(c, 3, 1).to(dev)
    thresholds = [float(torch.tensor(v, dtype=F32)) for v in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.999, 1.0)]
    curve = ops.reconstruction_curve(sd, td, ei, gp, thresholds)
    want = torch.stack([ops.reconstruction_counts(sd, td, ei, gp, thr) for thr in thresholds], 1)
    assert curve.dtype == I64 and curve.shape == (len(gp) - 1, len(thresholds), 4) and curve.is_cuda
    assert torch.equal(curve, want)
    assert int(curve[:, 0, 0].sum()) > int(curve[:, -2, 0].sum()) >= 0 and int(curve[:, -1, 1].sum()) == 0      # it is a curve
    assert ops.reconstruction_curve(sd[:0], td[:0], ei[:, :0], [0], thresholds).shape == (0, len(thresholds), 4)
    import deepgate
    dec = deepgate.digae_layer.DirectedInnerProductDecoder()
    assert torch.equal(dec.reconstruction_curve(sd, td, ei, gp, thresholds), curve)
    gae = deepgate.digae_model.DirectedGAE(encoder=None, decoder=dec)
    assert torch.equal(gae.reconstruction_curve(sd, td, ei, gp, thresholds), curve)
    print('HIST ops H=%d | profile = entry, curve = %d stacked reconstruction_counts | ok' % (H, len(thresholds)))


def test_the_model_methods_on_a_small_batch():
    """3 graphs of 300 nodes: similarity_profile against the binning of the dense cosines; equivalence_threshold for several budgets, each
    followed by equivalence_candidates at the threshold (exactly `pairs` pairs) and, when tight, at `lower` (refused); the curve."""
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
        hs, hf = model(batch)
    gp = batch.graph_ptr.tolist()
    assert gp == [0, 300, 600, 900]
    y = ops.row_unit(hf)
    dense = ops.pair_scores(y, y, sigmoid=False).cpu()
    above = model.similarity_profile(hf, HR.EDGES['B'], graph_ptr=batch.graph_ptr)
    assert above.shape == (3, 20) and above.dtype == I64 and above.is_cuda
    assert torch.equal(above.cpu(), HR.counts_above(HR.brute_hist(dense, gp, 'B', True)))
    allp = 3 * 300 * 299 // 2
    seen = []
    for P in (0, 10, 1000, 20000, allp):
        r = model.equivalence_threshold(hf, P, graph_ptr=batch.graph_ptr, lo=-2.0 if P == allp else 0.0)
        thr = r['threshold']
        assert isinstance(thr, float) and float(torch.tensor(thr, dtype=F32)) == thr and r['pairs'] <= P
        pi = model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=thr, max_pairs=P)[0]
        assert pi.shape[1] == r['pairs'] == int(((dense > thr) & ER.upper_mask(900, gp)).sum())
        if r['lower'] is not None:
            assert r['lower'] < thr and r['pairs_lower'] > P
            if r['tight']:
                with pytest.raises(_hip.HipLibraryError, match='max_pairs'):
                    model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=r['lower'], max_pairs=P)
        else:
            assert thr == (-2.0 if P == allp else 0.0)
        assert r['tight'] is True
        seen.append((P, thr, r['pairs']))
    assert seen[-1][2] == allp - int(torch.isnan(torch.triu(dense, 1)).sum()) and seen[0][2] == 0
    thresholds = [0.25, 0.5, 0.75]
    curve = model.reconstruction_curve(hs, batch.edge_index, batch.graph_ptr, thresholds)
    want = torch.stack([model.reconstruction_counts(hs, batch.edge_index, batch.graph_ptr, thr) for thr in thresholds], 1)
    assert curve.shape == (3, 3, 4) and torch.equal(curve, want)
    print('HIST model | (max_pairs, threshold, pairs): %s' % ', '.join('(%d, %.9g, %d)' % s for s in seen))


def test_feature_extract_profile_threshold_and_curve(tmp_path):
    """examples/feature_extract.py --similarity_profile B --equivalences_max P --recon_curve B beside the embeddings."""
    _dev()
    import importlib

    import numpy as np
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '2', '--rounds', '1', '--batch_size', '2', '--similarity_profile', '25', '--equivalences_max',
             '500', '--recon_curve', '4', '--out', str(out)])
    emb = np.load(out)
    keys = ('hs', 'hf', 'eq_pairs', 'eq_cos', 'eq_threshold', 'sim_thresholds', 'sim_counts_above', 'recon_thresholds', 'recon_curve')
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(2) for k in keys)
    total = 0
    for i in range(2):
        n = emb['graph%d/hf' % i].shape[0]
        st, sa = emb['graph%d/sim_thresholds' % i], emb['graph%d/sim_counts_above' % i]
        assert st.shape == (20,) and st.dtype == np.float32 and st[0] == 0.5 and (np.diff(st) > 0).all()       # capped at 20
        assert sa.shape == (20,) and sa.dtype == np.int64 and (np.diff(sa) <= 0).all() and 0 <= sa[-1] <= sa[0] <= n * (n - 1) // 2
        rt, rc = emb['graph%d/recon_thresholds' % i], emb['graph%d/recon_curve' % i]
        assert np.allclose(rt, [0.2, 0.4, 0.6, 0.8]) and rc.shape == (4, 4) and rc.dtype == np.int64
        assert (np.diff(rc[:, 1]) <= 0).all() and (rc[:, 0] <= rc[:, 2]).all() and (rc[:, 3] == n * n).all()
        eq, ec, thr = emb['graph%d/eq_pairs' % i], emb['graph%d/eq_cos' % i], emb['graph%d/eq_threshold' % i]
        assert thr.dtype == np.float32 and emb['graph0/eq_threshold'] == thr and (ec > thr).all() and (eq[0] < eq[1]).all()
        total += eq.shape[1]
    assert total <= 500
