"""CPU pins of tests/embed_sim_ref.py, the reference and the checkers behind tests/test_hip_embed_sim.py (mgv_row_unit,
mgv_sim_select_count, mgv_sim_select_fill of csrc/pair_scores.hip): cos_ref against torch.cosine_similarity and against the functional
loss's own distance, a float32 stand-in inside the derived bounds, the properties of the case builders the device tests rely on, the
measured band around each threshold, planted defects of a restated upper fill against the checkers the device file uses, and every
refusal the new entries and functions make on the host."""
import ctypes
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

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
SEEDS = (1, 2, 3)
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2


@functools.lru_cache(maxsize=None)
def _case(H, seed=1, kind='sim'):
    c = ER.CASES[kind](H, seed)
    return c, ER.cos_ref(c['x'])


@functools.lru_cache(maxsize=None)
def _f32(H, seed=1, kind='sim'):
    """The float32 stand-in of the case: (unit rows, norms, cosines)."""
    c, _ = _case(H, seed, kind)
    y, n = ER.unit_f32(c['x'])
    return y, n, ER.chain_f32(y)


# ------------------------------------------------------------------------------------------------ the reference
def test_cos_ref_is_torch_cosine_similarity_in_float64():
    """On listed pairs of the case (zero rows, the row below eps, the trio and the rest) and on the clamp example: the clamp is per row,
    [3e-9, 4e-9] against [0.5, 0] gives 0.3 (a clamp of the product of the norms would give 0.15)."""
    for H in HS:
        c, r = _case(H)
        N = c['N']
        g = torch.Generator().manual_seed(H)
        a, b = torch.randint(0, N, (4000,), generator=g), torch.randint(0, N, (4000,), generator=g)
        special = c['info']['zeros'] + [c['info']['tiny']] + c['info']['trio']
        a = torch.cat([a, torch.tensor(special * 2)])
        b = torch.cat([b, torch.tensor(special + special[::-1])])
        x = c['x'].to(F64)
        want = torch.cosine_similarity(x[a], x[b], dim=1, eps=ER.EPS)
        assert float((r['cos'][a, b] - want).abs().max()) <= 1e-12
    x = torch.tensor([[3e-9, 4e-9], [0.5, 0.0]], dtype=F64)
    got = ER.cos_ref(x)['cos'][0, 1]
    assert abs(float(got) - 0.3) <= 1e-12
    assert abs(float(torch.cosine_similarity(x[:1], x[1:], dim=1, eps=1e-8)) - 0.3) <= 1e-12


def test_one_minus_cos_is_the_functional_loss_distance():
    """dis of tests/losses_ref.py's restatement of the functional loss (trainer.py:158-163), on its own builder (tiny rows included)."""
    for H in (16, 64):
        fc = LR.build_func(300, H, 500, 3)
        hf = torch.as_tensor(fc['hf'])
        pr = torch.as_tensor(fc['pairs']).long().reshape(2, -1)
        dis = LR.func(hf, pr, fc['tt'])['dis']
        cos = ER.cos_ref(hf)['cos'][pr[0], pr[1]]
        assert float((1 - cos - dis).abs().max()) <= 1e-12


@pytest.mark.parametrize('H', HS)
def test_a_float32_stand_in_is_inside_the_bounds(H):
    """Sequential sum of squares and the k-ascending chain in float32, against unit_ref and cos_ref: worst error over bound < 1
    (measured: at most 0.34 for the unit rows, 0.17 for the cosines)."""
    wu = wn = wc = 0.0
    for seed in SEEDS:
        for kind in ER.CASES:
            c, r = _case(H, seed, kind)
            u = ER.unit_ref(c['x'])
            y, n, cs = _f32(H, seed, kind)
            wu = max(wu, ER.worst_ratio(y, u['y'], u['bound']))
            wn = max(wn, ER.worst_ratio(n, u['norm'], u['norm_bound']))
            wc = max(wc, ER.worst_ratio(cs, r['cos'], r['bound']))
            assert bool((torch.isnan(y) == torch.isnan(u['y'])).all())
    print('SIM stand-in H=%d | unit rows %.2g/1 | norms %.2g/1 | cosines %.2g/1' % (H, wu, wn, wc))
    assert wu < 1 and wn < 1 and wc < 1


# ------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize('H', HS)
def test_builder_properties(H):
    for seed in SEEDS:
        c, r = _case(H, seed)
        gp, N, info, x = c['graph_ptr'], c['N'], c['info'], c['x']
        assert N == 530 and [b - a for a, b in zip(gp, gp[1:])] == list(PR.TOPK_SIZES)
        um = ER.upper_mask(N, gp)
        assert int(um.sum()) == 34345 == sum(n * (n - 1) // 2 for n in PR.TOPK_SIZES)
        t0, t1, t2 = info['trio']
        assert t0 // 64 != t1 // 64 and gp[-2] <= t0 and t2 < gp[-1]              # across a 64-boundary, inside the 200-node graph
        y, n, cs = _f32(H, seed)
        assert torch.equal(y[t0].view(I32), y[t1].view(I32)) and torch.equal(y[t0].view(I32), y[t2].view(I32))
        cos, bound = r['cos'], r['bound']
        for a, b in ((t0, t1), (t0, t2), (t1, t2)):
            assert abs(float(cos[a, b]) - 1) <= 1e-12 and float(bound[a, b]) <= (2 * H + 6) * ER.U24 * (1 + 1e-12)
        assert 0.9999 < float(cos[t0, info['near']]) < 0.99999
        assert abs(float(cos[t0, info['neg']]) + 1) <= 1e-12
        # the zero rows: cosine exactly 0 with everything, also in float32; the row below eps comes out as x / eps
        z0, z1 = info['zeros']
        assert z0 == gp[4] and z1 == gp[4] + 64 == gp[5] - 1
        assert not bool(cos[[z0, z1]].any()) and not bool(cs[[z0, z1]].any()) and not bool(y[[z0, z1]].any())
        tn = info['tiny']
        assert 0 < float(x[tn].to(F64).norm()) < ER.EPS and torch.equal(r['y'][tn], x[tn].to(F64) / ER.EPS)
        # the 5-node graph, and the copy beyond its border
        lo, last = info['scaled']
        assert abs(float(cos[lo, last]) - 1) <= 1e-12 and info['border'] == (last, last + 1) and last + 1 == gp[-2]
        assert torch.equal(x[last].view(I32), x[last + 1].view(I32)) and not bool(um[last, last + 1]) and not bool(um[lo, last + 1])
        # exactly 7 pairs above 0.999, beyond doubt: 3 in the trio, 3 of the trio with the near-duplicate, 1 in the 5-node graph
        for shift in (-1, 1):
            row_ptr, col = ER.upper_select_ref(cos + shift * bound, gp, 0.999)
            rows = torch.repeat_interleave(torch.arange(N), row_ptr[1:] - row_ptr[:-1])
            want = sorted([(t0, t1), (t0, t2), (t1, t2), (t0, info['near']), (t1, info['near']), (t2, info['near']), (lo, last)])
            assert list(zip(rows.tolist(), col.tolist())) == want
        # every row's decade is its own: the norms span more than four decades
        nn = x.to(F64).norm(dim=1)
        assert float(nn[nn > 1e-6].max() / nn[nn > 1e-6].min()) > 1e4


def test_the_other_builders():
    c, r = _case(32, 1, 'empty_middle')
    assert c['graph_ptr'] == [0, 5, 5, 75, 77, 77, 143] and c['info']['scaled'] == (0, 4) and c['info']['border'] == (4, 5)
    row_ptr, col = ER.upper_select_ref(r['cos'], c['graph_ptr'], 0.999)
    assert row_ptr[-1] == 1 and col.tolist() == [4]
    c, r = _case(32, 1, 'nan')
    assert c['graph_ptr'] is None and c['N'] == 200 and bool(torch.isnan(r['cos'][77]).all()) and bool(torch.isnan(r['cos'][:, 77]).all())
    assert int(torch.isnan(r['cos']).sum()) == 2 * 200 - 1
    row_ptr, col = ER.upper_select_ref(r['cos'], None, 0.999)
    assert int(row_ptr[-1]) == 1 and int(row_ptr[61] - row_ptr[60]) == 1 and col.tolist() == [130]
    row_ptr, col = ER.upper_select_ref(r['cos'], None, -2.0)
    n = row_ptr[1:] - row_ptr[:-1]
    assert int(n[77]) == 0 and n[:77].tolist() == [200 - u - 2 for u in range(77)] and n[78:].tolist() == [200 - u - 1 for u in range(78, 200)]


def test_upper_mask_and_the_geometry_table():
    gp = [0, 3, 3, 5]
    m = ER.upper_mask(5, gp)
    assert torch.nonzero(m).tolist() == [[0, 1], [0, 2], [1, 2], [3, 4]]
    assert torch.equal(m, PR.candidate_mask(5, gp, True) & torch.ones(5, 5, dtype=torch.bool).triu(1))
    assert torch.nonzero(ER.upper_mask(3, None)).tolist() == [[0, 1], [0, 2], [1, 2]]
    for H in HS:
        rows = ER.UNIT_ROWS_PER_BLOCK[H]
        assert rows == ER.UNIT_THREADS // (H // 4)
        cap = ER.UNIT_CAP_ROWS[H]
        assert ER.unit_grid(H, cap) == ER.UNIT_GRID_CAP == ER.unit_grid(H, cap + 1) and ER.unit_grid(H, cap - rows) == ER.UNIT_GRID_CAP - 1
        assert ER.unit_grid(H, 1) == 1 and ER.unit_grid(H, rows + 1) == 2
        assert cap in ER.unit_sizes(H) and cap + 1 in ER.unit_sizes(H)


# ------------------------------------------------------------------------------------------------ the band
@pytest.mark.parametrize('H', HS)
def test_band_around_the_thresholds_is_narrow(H):
    """Pairs with 0 < |cos - thr| <= bound, from float64 alone, for every case the device check against float64 uses: at most
    max(4, 1e-3 of the candidates).  Measured at 8 x the bound: 0 pairs at 0.999, at most 2 at 0.25."""
    worst = {0.999: 0, 0.25: 0}
    wide = {0.999: 0, 0.25: 0}
    for seed in SEEDS:
        for kind in ER.CASES:
            c, r = _case(H, seed, kind)
            mask = ER.upper_mask(c['N'], c['graph_ptr'])
            for thr in (0.999, 0.25):
                n = ER.band_count(r['cos'], r['bound'], thr, mask)
                worst[thr] = max(worst[thr], n)
                wide[thr] = max(wide[thr], ER.band_count(r['cos'], 8 * r['bound'], thr, mask))
                assert n <= ER.band_limit(mask), (seed, kind, thr, n)
    print('SIM band H=%d | pairs within their bound of 0.999: %d, of 0.25: %d | within 8 x the bound: %d, %d'
          % (H, worst[0.999], worst[0.25], wide[0.999], wide[0.25]))


@pytest.mark.parametrize('H', HS)
def test_the_exact_thresholds(H):
    """0.0: a zero row's cosine is exactly 0 and is not selected (`>` is strict); -2: every upper candidate whose cosine is a number;
    1.5: nothing.  The same from the float32 stand-in, whose zero rows are zero rows."""
    c, r = _case(H)
    gp, N = c['graph_ptr'], c['N']
    _, _, cs = _f32(H)
    lo, hi = PR.row_range(gp, N)
    for sc in (r['cos'], cs):
        row_ptr, col = ER.upper_select_ref(sc, gp, 0.0)
        sel = SR.selected_matrix(row_ptr, col, N)
        for z in c['info']['zeros']:
            assert not bool(sel[z].any()) and not bool(sel[:, z].any())
        row_ptr, _ = ER.upper_select_ref(sc, gp, -2.0)
        assert torch.equal(row_ptr[1:] - row_ptr[:-1], hi - torch.arange(N) - 1) and int(row_ptr[-1]) == 34345
        assert int(ER.upper_select_ref(sc, gp, 1.5)[0][-1]) == 0


# ------------------------------------------------------------------------------------------------ planted defects
@functools.lru_cache(maxsize=None)
def _defect_scores():
    """The float32 stand-in's cosines of the H = 32 case; at 0.25 the 200-node graph's rows select across tile borders."""
    c, _ = _case(32)
    return c, _f32(32)[2]


def test_the_restated_upper_fill_without_a_defect_passes_both_checkers():
    c, cs = _defect_scores()
    _, r = _case(32)
    gp, N = c['graph_ptr'], c['N']
    for thr in (0.999, 0.25, -2.0):
        row_ptr, col, score = ER.restated_upper_fill(cs, gp, thr)
        assert ER.check_upper(row_ptr, col, score, cs, gp, thr) == [] and SR.UNWRITTEN not in col.tolist()
        assert ER.check_upper_band(row_ptr, col, r['cos'], r['bound'], gp, thr) == []
        want_ptr, want_col = ER.upper_select_ref(cs, gp, thr)
        assert torch.equal(row_ptr, want_ptr) and torch.equal(col, want_col)
    # the lists with their transposes are the general selection on (y, y) without self
    row_ptr, col, _ = ER.restated_upper_fill(cs, gp, 0.25)
    assert float((cs - cs.T).abs().max()) == 0.0
    full_ptr, full_col = SR.select_ref(cs, gp, 0.25, True)
    both = ER.both_sides(row_ptr, col, N)
    assert torch.equal(both[0], full_ptr) and torch.equal(both[1], full_col) and int((row_ptr[1:] - row_ptr[:-1]).max()) > 16


@pytest.mark.parametrize('defect', ER.DEFECTS)
def test_planted_defects_are_caught_by_the_exact_checker(defect):
    c, cs = _defect_scores()
    gp = c['graph_ptr']
    thr = 0.25
    row_ptr, col, score = ER.restated_upper_fill(cs, gp, thr, defect=defect)
    bad = ER.check_upper(row_ptr, col, score, cs, gp, thr) + SR.check_select(row_ptr, col, score, cs, gp, thr, True)
    exact = ER.check_upper(row_ptr, col, score, cs, gp, thr)
    print('SIM defect %s | %s' % (defect, exact))
    assert exact and bad


@pytest.mark.parametrize('defect', ER.DEFECTS)
def test_planted_defects_are_caught_by_the_float64_checker(defect):
    c, cs = _defect_scores()
    _, r = _case(32)
    gp = c['graph_ptr']
    row_ptr, col, _ = ER.restated_upper_fill(cs, gp, 0.25, defect=defect)
    assert ER.check_upper_band(row_ptr, col, r['cos'], r['bound'], gp, 0.25)


def test_a_selected_nan_is_caught():
    c, r = _case(32, 1, 'nan')
    _, _, cs = _f32(32, 1, 'nan')
    row_ptr, col = ER.upper_select_ref(torch.where(torch.isnan(cs), torch.ones_like(cs), cs), None, 0.999)
    assert int(row_ptr[-1]) > 1
    assert ER.check_upper(row_ptr, col, None, cs, None, 0.999) and ER.check_upper_band(row_ptr, col, r['cos'], r['bound'], None, 0.999)
    row_ptr, col = ER.upper_select_ref(cs, None, 0.999)
    assert ER.check_upper(row_ptr, col, None, cs, None, 0.999) == [] and ER.check_upper_band(row_ptr, col, r['cos'], r['bound'], None, 0.999) == []


# ------------------------------------------------------------------------------------------------ host-only paths
def test_the_entries_refuse_on_the_host_before_anything_is_launched():
    """H, N, the strides, the alignment and cap are looked at before any pointer is read or anything is launched (graph_ptr NULL: no
    read-back), so this runs without a GPU; the pointers are dummies.  The same on the device, with real buffers that must come back
    untouched: tests/test_hip_embed_sim.py."""
    from deepgate import _hip
    lib = _hip.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def unit(H=16, N=8, x=p, ldx=16, y=p, ldy=16):
        return lib.mgv_row_unit(H, N, x, ldx, 1e-8, y, ldy, None, None)

    def count(H=16, N=8, y=p, ldy=16, n_sel=p):
        return lib.mgv_sim_select_count(H, N, y, ldy, None, 0, 0.5, n_sel, None)

    def fill(H=16, N=8, y=p, ldy=16, cap=4, row_ptr=p, col=p):
        return lib.mgv_sim_select_fill(H, N, y, ldy, None, 0, 0.5, row_ptr, cap, col, None, None)

    for f in (unit, count, fill):
        for H in (0, 4, 8, 12, 48, 96, 256, -16):
            assert f(H=H) == MGV_EUNSUPPORTED, (f.__name__, H)
        assert f(H=48, N=-1) == MGV_EUNSUPPORTED                      # the width is looked at before anything else
        assert f(N=-1) == MGV_EINVAL and f(N=0) == 0
    for f in (count, fill):
        assert f(N=2 ** 31) == MGV_EINVAL
        assert f(ldy=12) == MGV_EINVAL and f(ldy=18) == MGV_EINVAL and f(y=odd) == MGV_EINVAL and f(y=None) == MGV_EINVAL
    assert count(n_sel=None) == MGV_EINVAL
    assert fill(cap=-1) == MGV_EINVAL and fill(cap=-1, N=0) == MGV_EINVAL and fill(cap=0) == 0
    assert fill(row_ptr=None) == MGV_EINVAL and fill(col=None) == MGV_EINVAL
    assert unit(ldx=12) == MGV_EINVAL and unit(ldx=18) == MGV_EINVAL and unit(ldy=12) == MGV_EINVAL and unit(ldy=22) == MGV_EINVAL
    assert unit(x=odd) == MGV_EINVAL and unit(y=odd) == MGV_EINVAL and unit(x=None) == MGV_EINVAL and unit(y=None) == MGV_EINVAL


def test_host_refusals_of_the_functions_need_no_gpu():
    from deepgate import _hip, ops, similarity
    x, x48 = torch.zeros(4, 16), torch.zeros(4, 48)
    pairs = torch.zeros((2, 3), dtype=I64)
    for call in (lambda v: ops.row_unit(v), lambda v: ops.sim_topk(v, 2), lambda v: ops.sim_pairs(v), lambda v: ops.sim_at(v, pairs)):
        with pytest.raises(_hip.HipLibraryError, match='MGV_EUNSUPPORTED'):
            call(x48)
        with pytest.raises(_hip.HipLibraryError, match='GPU'):
            call(x)                                          # no CPU implementation behind it
    with pytest.raises(_hip.HipLibraryError) as e:
        similarity._sim_room(98113, False, 50000, None)
    assert '98113' in str(e.value) and '50000' in str(e.value) and 'threshold' in str(e.value) and 'sim_topk' in str(e.value)
    with pytest.raises(_hip.HipLibraryError) as e:
        similarity._sim_room(2 ** 30, True, None, 2 ** 30)
    assert str(2 ** 30) in str(e.value) and '24.0 GiB' in str(e.value)
    similarity._sim_room(10, True, 10, 240)                  # exactly at both limits: accepted
    similarity._sim_room(10, False, None, 200)
    similarity._sim_room(0, False, 0, 0)


def test_the_header_declares_the_entries_with_their_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_row_unit']) == 9 and len(sigs['mgv_sim_select_count']) == 9 and len(sigs['mgv_sim_select_fill']) == 12
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in ('mgv_row_unit', 'mgv_sim_select_count', 'mgv_sim_select_fill'):
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'trainer.py:158-160' in comment
        assert name == 'mgv_row_unit' or 'digae_layer.py:31-33' in comment
    unit = text[:text.index('int mgv_row_unit(')]
    assert 'finite sum of squares' in unit[unit.rindex('/*'):]


def test_the_surface_says_what_a_user_will_meet():
    """Added functionality, the loss it mirrors, zero rows and the threshold 1.0: in the docstrings of the three methods and of ops."""
    from deepgate import ops
    from deepgate._model_base import FunctionalModel as M
    for f in (M.similar_gates, M.equivalence_candidates, M.functional_similarity):
        doc = ' '.join(f.__doc__.split())
        assert 'Added functionality' in doc and 'trainer.py:158-160' in doc and 'hf = 0' in doc
    for f in (M.similar_gates, M.equivalence_candidates, ops.sim_topk, ops.sim_pairs):
        assert '(2H + 6) 2^-24' in ' '.join(f.__doc__.split())
    import inspect
    for f in (M.similar_gates, M.equivalence_candidates, ops.sim_topk, ops.sim_pairs):
        assert inspect.signature(f).parameters['threshold'].default == 0.999
