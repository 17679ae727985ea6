"""Pin the float64 references of the loss / decoder / KL / Adam kernels (tests/losses_ref.py) where there is no GPU: against the
golden vectors the reference itself produced, against oracle/ref_cpu.py run in float64, against torch.optim.Adam in float64 — and
assert the properties of the input builders that the GPU tests (tests/test_hip_losses_reference.py) rely on.  CPU only."""
import numpy as np
import pytest
import torch

import losses_ref as LR
from conftest import load_golden
from oracle import ref_cpu as R

F64 = torch.float64


def _close(a, b, rtol, atol=0.0):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, np.asarray(b), rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------------ golden fixtures
@pytest.mark.parametrize('name', ['g1_aig', 'g1_mig', 'g1_xag', 'g1_xmg'])
def test_recon_matches_the_reference_models_eval_loss(name):
    z = load_golden(name)
    p = R.params_from_npz(z, requires_grad=False)
    st = R.linear(p, 'hs_decompose', torch.from_numpy(z['eval_hs']))
    r = LR.recon(st, z['in_edge_index'], z['in_neg_edge_index'])
    _close(r['loss'], z['eval_recon'], 1e-5)
    assert np.array_equal(r['pred'].numpy(), z['eval_pred_bin'])
    gt = z['eval_gt_bin']
    assert r['counts'] == LR.confusion(z['eval_pred_bin'], gt)
    assert sum(r['counts']) == gt.size


def test_func_and_decoder_match_the_operator_fixture():
    z = load_golden('g3_ops')
    f = LR.func(z['fl_hf'], z['fl_pairs'], z['fl_tt'])
    _close(f['dis'], z['fl_dis'], 1e-5, 1e-6)
    _close(f['loss'], z['fl_loss'], 1e-5)
    _close(f['grad'], z['fl_grad_hf'], 1e-4, 1e-7)
    _close(LR.edge_scores(z['dec_s'], z['dec_t'], z['dec_edge_index']), z['dec_sig'], 1e-6, 1e-7)
    _close(LR.edge_scores(z['dec_s'], z['dec_t'], z['dec_edge_index'], sigmoid=False), z['dec_raw'], 1e-6, 1e-6)


def test_reparam_and_kl_match_the_vae_fixture():
    z = load_golden('g4_vae')
    p = R.params_from_npz(z, requires_grad=False)
    for side in ('s', 't'):
        x = torch.from_numpy(z[side])
        mu, ls = R.linear(p, 'fc_%s_mu' % side, x), R.linear(p, 'fc_%s_logstd' % side, x)
        r = LR.reparam(mu, ls, z['eps_' + side])
        _close(r['z'], z['sample_' + side], 1e-5, 1e-6)
        n = mu.shape[0]
        _close(-0.5 / n * r['kl'] / n, z[side + '_kl'], 1e-5)          # trainer.py:146-147: the double 1 / N


# ------------------------------------------------------------------------------------------------ oracle/ref_cpu.py in float64
def _perm_params(H, prefix):
    """A Linear whose output is [x | x[:, perm]] exactly (identity and permutation blocks, zero bias)."""
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(H))
    W = torch.cat([torch.eye(H, dtype=F64), torch.eye(H, dtype=F64)[perm]])
    return {prefix + '.weight': W, prefix + '.bias': torch.zeros(2 * H, dtype=F64)}, perm


@pytest.mark.parametrize('H', [16, 64])
def test_recon_equals_the_oracle_in_float64(H):
    g = torch.Generator().manual_seed(H)
    N = 300
    hs32 = (0.6 * torch.randn(N, H, generator=g)).float()
    p, perm = _perm_params(H, 'hs_decompose')
    pos, neg = torch.randint(0, N, (2, 900), generator=g), torch.randint(0, N, (2, 1100), generator=g)
    hs = hs32.to(F64).requires_grad_(True)
    loss, pred, gt = R.recon_loss(p, hs, pos, neg)
    (2.5 * loss).backward()
    st32 = torch.cat([hs32, hs32[:, perm]], dim=1)
    r = LR.recon(st32, pos, neg, gscale=2.5)
    assert abs(float(r['loss']) - float(loss.detach())) <= 1e-12
    assert np.array_equal(r['pred'].numpy(), pred.numpy())
    inv = torch.argsort(perm)
    back = r['grad'][:, :H] + r['grad'][:, H:][:, inv]                 # d st -> d hs through the two blocks
    assert float((back - hs.grad).abs().max()) <= 1e-12
    _close(LR.edge_scores(st32[:, :H], st32[:, H:], pos), R.decoder(st32[:, :H].to(F64), st32[:, H:].to(F64), pos), 1e-14)
    # the analytic coefficients the row scales are built from: d loss / d raw
    pp = r['p']
    c = torch.cat([-2.5 / 900 * pp[:900] * (1 - pp[:900]) / (pp[:900] + 1e-15), 2.5 / 1100 * pp[900:] * (1 - pp[900:]) / (1 - pp[900:] + 1e-15)])
    assert float((c - r['coef']).abs().max()) <= 1e-15


def test_an_empty_half_contributes_zero():
    g = torch.Generator().manual_seed(5)
    st = torch.randn(40, 32, generator=g)
    pos = torch.randint(0, 40, (2, 70), generator=g)
    none = torch.zeros(2, 0, dtype=torch.int64)
    both = LR.recon(st, pos, pos)
    only_p, only_n = LR.recon(st, pos, none), LR.recon(st, none, pos)
    assert abs(float(only_p['loss']) + float(only_n['loss']) - float(both['loss'])) <= 1e-13
    assert float(only_p['sums'][1]) == 0.0 and float(only_n['sums'][0]) == 0.0
    assert only_p['counts'][1] == 0 and only_p['counts'][2] == 0 and only_n['counts'][0] == 0 and only_n['counts'][3] == 0
    assert float(LR.recon(st, none, none)['loss']) == 0.0


@pytest.mark.parametrize('H,P', [(16, 2), (32, 257), (64, 5000)])
def test_func_equals_the_oracle_in_float64(H, P):
    c = LR.func_case(H, P, signed=(H == 32), tiny=False)          # rows are zero or far above the clamp: see the next test for the rest
    hf = c['hf'].to(F64).requires_grad_(True)
    fl, dis = R.func_loss(hf, c['pairs'], c['tt'].to(F64))
    (1.3 * fl).backward()
    f = LR.func(c['hf'], c['pairs'], c['tt'], gscale=1.3)
    assert abs(float(f['loss']) - float(fl.detach())) <= 1e-12
    assert float((f['dis'] - dis.detach()).abs().max()) <= 1e-12
    assert LR.row_ratio(f['grad'], hf.grad, f['S']) <= 1e-12
    # the sums in the kernel's order reproduce the statistics, and imposing a run's own signs changes nothing
    s = f['sums'].tolist()
    d = dis.detach()
    assert abs(s[0] / P - float(d.mean())) <= 1e-12 and abs((s[1] - s[0] ** 2 / P) / (P - 1) - float(d.var())) <= 1e-12
    assert abs(s[4] / P - float(fl.detach())) <= 1e-12 and s[5] == float(f['sgn'].sum())
    g = LR.func(c['hf'], c['pairs'], c['tt'], gscale=1.3, signs=f['sgn'], add=torch.ones_like(c['hf']))
    assert float((g['grad'] - 1.0 - f['grad']).abs().max()) <= 1e-12 * max(1.0, float(f['grad'].abs().max()))


def test_where_torchs_cosine_autograd_leaves_the_formula():
    """F.cosine_similarity clamps the norms in place under no_grad: its VALUE is <a, b> / (max(|a|, eps) max(|b|, eps)), but its
    autograd differentiates |a| even while the clamp holds.  For |a| = 0 (the product's never-updated rows) and |a| > eps that is
    the formula's derivative; for 0 < |a| < eps it carries an extra own-row term -cos a / (eps |a|).  The kernels (and losses_ref)
    implement the formula's derivative — a clamped norm is a constant.  Shown here: values agree everywhere, gradients agree
    except on the rows inside the clamp and differ there by exactly that term."""
    c = LR.func_case(32, 257, signed=True)
    hf = c['hf'].to(F64).requires_grad_(True)
    fl, dis = R.func_loss(hf, c['pairs'], c['tt'].to(F64))
    fl.backward()
    f = LR.func(c['hf'], c['pairs'], c['tt'])
    assert abs(float(f['loss']) - float(fl.detach())) <= 1e-12 and float((f['dis'] - dis.detach()).abs().max()) <= 1e-12
    nrm = c['hf'].to(F64).norm(dim=1)
    inside = (nrm > 0) & (nrm < 1e-8)
    err = (f['grad'] - hf.grad).abs().amax(dim=1) / f['S'].clamp_min(1e-300)
    assert float(err[~inside].max()) <= 1e-12 and float(err[inside].max()) > 1e-4
    extra = torch.zeros_like(f['grad'])
    x = c['hf'].to(F64)
    cos = 1 - f['dis']
    for side in (0, 1):
        rows = c['pairs'][side]
        sel = inside[rows]
        extra.index_add_(0, rows[sel], -(f['dc'][sel] * cos[sel] / (1e-8 * nrm[rows[sel]])).unsqueeze(1) * x[rows[sel]])
    assert LR.row_ratio(f['grad'] + extra, hf.grad, f['S']) <= 1e-12


def test_func_clamped_norm_gradient_is_the_formulas():
    """The reference's gradient through clamped rows is what the kernels implement: for a ZERO row d cos / d x = y / (eps |y|) (and 0
    for the other row when both are zero), for a row with 0 < |x| < eps the same with no own-row term (the norm factor does not
    depend on x while it is clamped)."""
    hf = torch.tensor([[0.0, 0.0, 0.0, 0.0], [3.0, 4.0, 0.0, 0.0], [1.0, 2.0, 2.0, 0.0], [0.5, 0.0, 0.0, 1.0], [3e-9, 0.0, -4e-9, 0.0]])
    pairs = torch.tensor([[0, 1, 0, 2, 3, 4, 2, 4], [1, 2, 0, 3, 1, 1, 4, 0]])
    tt = torch.tensor([0.1, 0.7, 0.3, 0.9, 0.45, 0.2, 0.6, 0.8])
    f = LR.func(hf, pairs, tt)
    x = hf.to(F64)
    dc = f['dc']
    expect = torch.zeros(5, 4, dtype=F64)
    eps = 1e-8
    for q in range(8):
        a, b = int(pairs[0, q]), int(pairs[1, q])
        ra, rb = float(x[a].norm()), float(x[b].norm())
        na, nb = max(ra, eps), max(rb, eps)
        cs = float(x[a] @ x[b]) / (na * nb)
        expect[a] += dc[q] * (x[b] / (na * nb) - (cs / na ** 2 * x[a] if ra > eps else 0))
        expect[b] += dc[q] * (x[a] / (na * nb) - (cs / nb ** 2 * x[b] if rb > eps else 0))
    assert float(expect[0].abs().max()) > 1e5 * float(expect[2].abs().max())      # the zero row's gradient carries the 1 / eps
    assert LR.row_ratio(f['grad'], expect, f['S']) <= 1e-12
    assert float(f['dis'][0]) == 1.0 and float(f['dis'][2]) == 1.0


def test_reparam_equals_the_oracle_in_float64():
    g = torch.Generator().manual_seed(11)
    N, H = 50, 16
    s32, t32 = torch.randn(N, H, generator=g), (3 * torch.rand(N, H, generator=g) - 2)
    es, et = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    eye, z0 = torch.eye(H, dtype=F64), torch.zeros(H, dtype=F64)
    perm = torch.eye(H, dtype=F64)[torch.randperm(H, generator=g)]
    p = {'fc_s_mu.weight': eye, 'fc_s_mu.bias': z0, 'fc_s_logstd.weight': perm, 'fc_s_logstd.bias': z0,
         'fc_t_mu.weight': eye, 'fc_t_mu.bias': z0, 'fc_t_logstd.weight': perm, 'fc_t_logstd.bias': z0}
    zs, zt, (smu, sls, tmu, tls) = R.vae_sample(p, s32.to(F64), t32.to(F64), es.to(F64), et.to(F64))
    mu = smu.clone().requires_grad_(True)
    ls = sls.clone().requires_grad_(True)
    up = torch.randn(N, H, generator=g).to(F64)
    z = mu + torch.exp(ls) * es.to(F64)
    kl = R.kl_term(mu, ls)
    ((z * up).sum() + 0.7 * kl).backward()
    # kl_term = -0.5 / N * klsum / N: gkl * klcoef is its factor in front of the sum
    r = LR.reparam(smu.float(), sls.float(), es, gz=up, gkl=0.7, klcoef=-0.5 / N / N)
    assert float((r['z'] - zs).abs().max()) <= 1e-12 and float((r['z'] - z.detach()).abs().max()) <= 1e-12
    assert abs(float(-0.5 / N * r['kl'] / N) - float(kl.detach())) <= 1e-12
    assert float((r['dmu'] - mu.grad).abs().max()) <= 1e-12 and float((r['dls'] - ls.grad).abs().max()) <= 1e-12
    r0 = LR.reparam(smu.float(), sls.float(), es, gz=None, gkl=None)
    assert float(r0['dmu'].abs().max()) == 0.0 and float(r0['dls'].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.5, 0.9)])
def test_adam_equals_torch_optim_adam_in_float64(wd, betas):
    c = LR.build_adam(301, 50, seed=3)
    gs = 0.125
    p = torch.nn.Parameter(c['p'].to(F64).clone())
    opt = torch.optim.Adam([p], lr=1e-3, betas=betas, eps=1e-8, weight_decay=wd)
    for k in range(50):
        p.grad = c['g'][k].to(F64) * gs                   # grad_scale folded into the gradient on torch's side
        opt.step()
    r = LR.adam(c['p'], c['g'], torch.zeros(301), torch.zeros(301), 1e-3, betas, 1e-8, wd, gs)
    st = opt.state[p]
    assert float((r['p'] - p.detach()).abs().max()) <= 1e-12
    assert float(((r['m'] - st['exp_avg']).abs() - 1e-12 * r['m_scale']).max()) <= 0
    assert float(((r['v'] - st['exp_avg_sq']).abs() - 1e-12 * r['v_scale']).max()) <= 0
    if wd == 0:
        assert float(r['m_scale'][c['dead']].max()) == 0.0 and float((r['p'][c['dead']] - c['p'][c['dead']].to(F64)).abs().max()) == 0.0
    # a later start: the bias corrections follow first_step
    r2 = LR.adam(r['p'].float(), c['g'][:1], r['m'].float(), r['v'].float(), 1e-3, betas, 1e-8, wd, gs, first_step=51)
    q = torch.nn.Parameter(r['p'].float().to(F64))
    opt2 = torch.optim.Adam([q], lr=1e-3, betas=betas, eps=1e-8, weight_decay=wd)
    opt2.state[q] = {'step': torch.tensor(50.0), 'exp_avg': r['m'].float().to(F64), 'exp_avg_sq': r['v'].float().to(F64)}
    q.grad = c['g'][0].to(F64) * gs
    opt2.step()
    assert float((r2['p'] - q.detach()).abs().max()) <= 1e-12


def test_adam_builder_spans_the_magnitudes():
    c = LR.build_adam(100003, 8, seed=1)
    a = c['g'].abs().numpy()
    live = a[:, ~c['dead'] & ~c['late']]
    assert live.min() >= 0.4e-8 and live.max() <= 1.6 and np.median(live) < 1e-3 and (live > 0.1).any() and (live < 1e-7).any()
    assert c['dead'].sum() > 9000 and not a[:, c['dead']].any()
    assert c['late'].sum() > 6000 and not a[:4, c['late']].any() and a[4:, c['late']].all()


# ------------------------------------------------------------------------------------------------ the Gaussian generator
def test_hash_words_against_hand_computed_values():
    """(seed, i) -> (a, b), worked out by hand with Python integers (x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33 on seed * 0x9E3779B97F4A7C15 + 2 i (+ 1), low 32 bits)."""
    table = {(0, 0): (0x0, 0x34c2cb2c), (1, 5): (0xddc76878, 0x8d88bdc6), (0xDEADBEEFCAFEF00D, (1 << 20) + 2): (0x4a2caa3a, 0xa691c1ce)}
    for (seed, i), (wa, wb) in table.items():
        a, b = LR.gauss_words(seed, 1, start=i)
        assert (int(a[0]), int(b[0])) == (wa, wb)
        base = seed * 0x9E3779B97F4A7C15
        assert (LR.mix32_scalar(base + 2 * i), LR.mix32_scalar(base + 2 * i + 1)) == (wa, wb)
    a, b = LR.gauss_words(1, 8)
    assert (int(a[5]), int(b[5])) == table[(1, 5)]
    # word 0 of seed 0 is 0: u1 takes its smallest value 2^-24, never 0; the radius there is the largest the generator produces
    u1, u2 = LR.gauss_uniforms(0, 4)
    assert float(u1[0]) == 2.0 ** -24 and float(u2[0]) == (0x34c2cb2c >> 8) / 2.0 ** 24
    assert abs(abs(LR.gauss_from_counter(0, 1)[0]) - np.sqrt(48 * np.log(2.0)) * abs(np.cos(2 * np.pi * float(u2[0])))) < 1e-12


def test_gauss_from_counter_is_standard_normal():
    n = 1 << 20
    u1, u2 = LR.gauss_uniforms(20260101, n)
    assert u1.dtype == np.float32 and u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    e = LR.gauss_from_counter(20260101, n)
    assert np.isfinite(e).all()
    assert abs(e.mean()) < 5 / np.sqrt(n) and abs(e.var() - 1) < 5 * np.sqrt(2.0 / n)          # five standard errors
    assert abs((e ** 4).mean() - 3) < 0.05
    assert np.abs(e).max() <= np.sqrt(48 * np.log(2.0))
    assert not np.array_equal(e[:64], LR.gauss_from_counter(20260102, 64))
    assert np.array_equal(e[100:164], LR.gauss_from_counter(20260101, 64, start=100))
    assert abs(LR.GAUSS_FLOOR - 2.2e-6) < 0.05e-6


def test_confusion_counts_only_zeros_and_ones():
    pred = np.array([1, 1, 0, 0, 2, -1, 1, 0], dtype=np.int32)
    gt = np.array([1, 0, 0, 1, 1, 0, 3, 0], dtype=np.int32)
    assert LR.confusion(pred, gt) == [1, 1, 2, 1]
    assert LR.confusion(torch.from_numpy(pred), torch.from_numpy(gt)) == [1, 1, 2, 1]


# ------------------------------------------------------------------------------------------------ builders: reconstruction
def _recon_cases():
    out = []
    for H in (16, 32, 64, 128):
        for size in LR.recon_sizes(H):
            out.append((H, size, False))
        out.append((H, 'odd', True))
    return out


@pytest.mark.parametrize('H,size,wide', _recon_cases())
def test_recon_builder_properties(H, size, wide):
    c = LR.recon_case(H, size, wide=wide)
    N, B = c['N'], c['B']
    st = c['st']
    assert st.dtype == torch.float32 and st.shape == (N, 2 * H)
    s, t = st[:, :H].to(F64), st[:, H:].to(F64)
    assert float(s.norm(dim=1).max()) ** 2 <= B * (1 + 1e-6) and float(t.norm(dim=1).max()) ** 2 <= B * (1 + 1e-6)
    assert not st[c['zero_rows']].any()
    for key in ('pos', 'neg'):
        e = c[key]
        assert e.dtype == torch.int64 and e.shape[0] == 2 and e.shape[1] > 0 and int(e.min()) >= 0 and int(e.max()) < N
        raw = LR.edge_scores(s, t, e, sigmoid=False)
        assert float(raw.abs().max()) <= B * (1 + 1e-6)
        inside = (raw.abs() < LR.BAND) & (raw != 0)
        assert not bool(inside.any())                                   # the counters are compared exactly
        if N >= 129:
            assert bool((raw == 0).any())                               # zero rows are hit: p = 0.5 exactly
        if wide:
            assert int((raw.abs() > 13.9).sum()) >= 50                  # the ends are reached
        if N > 17:
            keys = e[0] * N + e[1]
            assert keys.unique().numel() < keys.numel()                 # duplicates
        assert bool((e[0] == e[1]).any())                               # self loops
    tot = LR.list_totals(c)
    if N >= LR.DESIGNED_MIN_N:
        for u, cnt in c['designed'].items():
            assert tuple(tot[u]) == cnt, (u, tuple(tot[u]), cnt)
        sums = {sum(cnt) for cnt in c['designed'].values()}
        assert sums >= set(LR.LIST_TOTALS) | {0}
        for k in LR.LIST_TOTALS:                                        # every total also all in ONE list, for each of the four lists
            for j in range(4):
                assert any(cnt[j] == k and sum(cnt) == k for cnt in c['designed'].values()), (k, j)
        assert (tot[:, 0] == LR.HEAVY_ROW).any() and (tot[:, 0] == LR.HEAVY_ROW + 1).any()
        assert (tot[:, 1] == LR.HEAVY_ROW).any() and (tot[:, 1] == LR.HEAVY_ROW + 1).any()
        for ko, ki in LR.HUBS:
            assert ((tot[:, 0] == ko) & (tot[:, 1] == ki)).any()
        assert ((tot[:, 0] > LR.HEAVY_ROW) & (tot[:, 1] <= LR.HEAVY_ROW)).any() and ((tot[:, 1] > LR.HEAVY_ROW) & (tot[:, 0] <= LR.HEAVY_ROW)).any()
        assert (tot.sum(axis=1) == 0).sum() >= 40
    else:
        assert tot[:, :2].max() <= LR.HEAVY_ROW                         # the small cases run the pull without heavy lists
    # the same call gives the same case
    again = LR.recon_case(H, size, wide=wide)
    assert torch.equal(again['st'], st) and torch.equal(again['pos'], c['pos']) and torch.equal(again['neg'], c['neg'])


def test_recon_sizes_cross_the_boundaries_they_are_named_for():
    for H in (16, 32, 64, 128):
        rpb, sz = LR.rows_per_workgroup(H), LR.recon_sizes(H)
        grid = lambda n: min(-(-n // rpb), LR.GRID_CAP)
        for name in ('xcd_short', 'xcd'):
            n = sz[name]
            assert grid(n) % 8 == 0 and grid(n) < LR.GRID_CAP
            chunk = -(-n // (8 * rpb)) * rpb
            assert 0 < n - 7 * chunk < chunk                            # the last XCD range is short, not empty
        assert grid(sz['odd']) % 8 != 0
        assert sz['cap'] > LR.GRID_CAP * rpb and min(sz['xcd'], sz['odd'], sz['cap']) >= LR.DESIGNED_MIN_N
    assert LR.recon_sizes(64)['xcd_short'] == 8 * 16 * 5 - 3


@pytest.mark.parametrize('want_pos', [True, False])
def test_recon_builder_one_sided_cases(want_pos):
    c = LR.recon_case(64, 'xcd', want_pos=want_pos, want_neg=not want_pos)
    assert (c['pos'].shape[1] > 0) == want_pos and (c['neg'].shape[1] > 0) == (not want_pos)
    tot = LR.list_totals(c)
    for k in LR.LIST_TOTALS:
        assert (tot.sum(axis=1) == k).any()


@pytest.mark.parametrize('H,wide', [(16, False), (64, False), (16, True), (64, True)])
def test_float32_route_sits_inside_the_derived_forward_bounds(H, wide):
    """The reference's own float32 arithmetic (torch on the CPU) against the bounds the GPU test asserts for the device."""
    c = LR.recon_case(H, 'odd', wide=wide)
    r64 = LR.recon(c['st'], c['pos'], c['neg'])
    r32 = LR.recon(c['st'], c['pos'], c['neg'], dtype=torch.float32)
    err = abs(float(r32['loss']) - float(r64['loss']))
    print('H=%d wide=%s: float32 loss error %.3g, bound %.3g; worst |dp| / dq %.3g' %
          (H, wide, err, r64['loss_bound'], float(((r32['p'].to(F64) - r64['p']).abs() / r64['dq']).max())))
    assert err <= r64['loss_bound']
    assert bool(((r32['p'].to(F64) - r64['p']).abs() <= r64['dq']).all())
    assert r32['counts'] == r64['counts'] and torch.equal(r32['pred'], r64['pred'])
    assert r64['loss_bound'] < (1e-2 if wide else 1e-5)


# ------------------------------------------------------------------------------------------------ builders: functional loss
@pytest.mark.parametrize('H', [16, 32, 64])
@pytest.mark.parametrize('P', LR.FUNC_P)
def test_func_builder_properties(H, P):
    signed = (P % 2 == 1)
    c = LR.func_case(H, P, signed=signed)
    hf, pairs, tt, N = c['hf'], c['pairs'], c['tt'], c['N']
    assert hf.shape == (N, H) and pairs.shape == (2, P) and tt.shape == (P,) and hf.dtype == torch.float32 and tt.dtype == torch.float32
    assert N % LR.rows_per_workgroup(H) != 0
    zero = ~hf.any(dim=1)
    assert int(zero.sum()) == len(range(3, N, 7)) and bool((hf < 0).any()) == signed
    assert float(hf[hf != 0].abs().min()) > 1e-19                     # squares far above float32's denormals
    f = LR.func(hf, pairs, tt)
    assert float(f['diff'].abs().min()) >= LR.FUNC_MARGIN
    if P > 2:
        f32 = LR.func(hf, pairs, tt, dtype=torch.float32)
        assert torch.equal(f32['sgn'].to(F64), f['sgn'])                  # the reference's own float32 route decides the same signs
    if P >= 255:
        za, zb = zero[pairs[0]], zero[pairs[1]]
        assert bool((za & ~zb).any()) and bool((~za & zb).any()) and bool((za & zb).any())
        assert bool((pairs[0] == pairs[1]).any())
        nrm = hf.to(F64).norm(dim=1)
        tiny = (nrm > 4e-9) & (nrm < 6e-9)
        assert int(tiny.sum()) >= N // 40 and bool((tiny[pairs[0]] & ~zb & ~tiny[pairs[1]]).any()) and bool((tiny[pairs[1]] & ~za & ~tiny[pairs[0]]).any())
        assert float(f['grad'][tiny].abs().max()) > 0                # clamped, and their gradient is alive
        keys = pairs[0] * N + pairs[1]
        assert keys.unique().numel() < P
        used = torch.zeros(N, dtype=torch.bool)
        used[pairs[0]] = True
        used[pairs[1]] = True
        assert int((~used).sum()) >= N // 10 and not bool(used[c['n_in']:].any())
        assert float(f['S'][~used].max()) == 0.0 and float(f['grad'][~used].abs().max()) == 0.0
    assert bool(torch.isfinite(f['grad']).all()) and (P == 2 or float(f['dis'].std()) > 0.05)          # well conditioned
