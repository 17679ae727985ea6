"""float64 restatement of the fused variational link heads, mgv_var_head_fwd_x3 / mgv_var_head_bwd_x3 (csrc/var_head_x3.hip;
digvae_model.py:134-142, trainer.py:145-148), from exactly the arguments of the C ABI, with one error scale per output entry, a
float32 stand-in in the kernel's arithmetic, planted defects, seeded builders and the launch geometry restated.

Scales.  Every output is a sum of terms; its scale is the sum of the terms' magnitudes, and where a term goes through exp(ls) the
error ls itself may carry (its own scale S_ls) is carried along with the factor's derivative:
    P = X Wp^T + bp          S_P   = |X| |Wp|^T + |bp|                                   (S_mu, S_ls: its column halves)
    z = mu + e^ls eps        S_z   = S_mu + e^ls |eps| (1 + S_ls)
    kl terms                 S_kl  = sum 1 + 2 S_ls + mu^2 + 2 |mu| S_mu + e^2ls (1 + 2 S_ls)
    dmu = gz - 2 gk mu       S_dmu = |gz| + 2 |gk| S_mu
    dls = gz eps e^ls + gk (2 - 2 e^2ls)
                             S_dls = |gz eps| e^ls (1 + S_ls) + |gk| (2 + 2 e^2ls + 4 e^2ls S_ls)
    dST = dP Wp, dWp = dP^T X, dbp = colsum(dP):  S_dP through |Wp|, |X| and the column sum.
A ratio is |got - float64| / scale; the device bound is tau = 8 max(r, 2^-17) with r the float32 stand-in's ratio (dense_ref.taus)."""
import numpy as np
import torch

import dense_ref as DR
import losses_ref as LR
from dense_ref import F32, F64, TILE, mm3

NAN = float('nan')
THREADS_FWD, THREADS_BWD = 256, 512       # var_head_x3.hip: kThreads, VarBwdGeom::NT
LDS_BYTES = 160 * 1024
WIDTHS = (32, 64)                         # mgv_launch.h X3Widths
ROW_OUT = ('Z', 'ML', 'dST')
SUM_OUT = ('kl', 'dWp_s', 'dWp_t', 'dbp_s', 'dbp_t')


# ------------------------------------------------------------------------------------------------ launch geometry, restated
def fwd_smem(H):      # VarFwdGeom::smem_bytes: two bf16 planes of H + 8, the fp32 stage of 2H + 4, one double per thread
    return 2 * TILE * (H + 8) * 2 + TILE * (2 * H + 4) * 4 + THREADS_FWD * 8


def bwd_smem(H):      # VarBwdGeom::smem_bytes: dP planes of 2H + 8, X planes of H + 8, all but one k-step of both transposed weight planes
    return 2 * TILE * (2 * H + 8) * 2 + 2 * TILE * (H + 8) * 2 + 2 * (H // 16) * (2 * H // 32 - 1) * 512 * 2


# kernel: (resident workgroups per CU, the source line restated).  Workgroups PER HALF = min(tiles, 128 per_cu); the grid is twice that
GEOMETRY = {
    'var_head_fwd': (lambda H: min(4, LDS_BYTES // fwd_smem(H)), 'var_head_x3.hip VarFwdGeom::per_cu = min(4, 160 KiB / smem_bytes); var_head_nwg'),
    'var_head_bwd': (lambda H: 1 if H == 64 else 2, 'var_head_x3.hip VarBwdGeom::per_cu = H == 64 ? 1 : 2 (216 VGPRs x 8 waves at 64); var_head_nwg'),
}


def per_cu(kernel, H):
    return GEOMETRY[kernel][0](H)


def nwg(kernel, H, N):
    """Workgroups per half (slab rows per half)."""
    return min(max((N + TILE - 1) // TILE, 1), 128 * per_cu(kernel, H))


def cap_rows(kernel, H):
    """The largest N at which every workgroup visits one tile."""
    return 128 * per_cu(kernel, H) * TILE


def large_rows(kernel, H):
    """2 cap_rows + 5 tiles + 19 rows: workgroups 0..5 of a half visit three tiles, the others two, the last tile is partial."""
    return 2 * cap_rows(kernel, H) + 5 * TILE + 19


def ws_floats(H, N, backward):
    """mgv_var_head_x3_ws_floats."""
    if backward:
        return nwg('var_head_bwd', H, N) * 2 * (2 * H * H + 2 * H)
    return nwg('var_head_fwd', H, N) * 4


# ------------------------------------------------------------------------------------------------ the generator, per the ABI
def noise(H, N, seed, same_seed=False):
    """float64 [N, 2H] = [eps_s | eps_t]: element (r, c) of half h is the generator at element r * H + c of seed + h."""
    halves = [torch.from_numpy(LR.gauss_from_counter(int(seed) + (0 if same_seed else h), N * H)).reshape(N, H) for h in (0, 1)]
    return torch.cat(halves, 1)


# ------------------------------------------------------------------------------------------------ both entries
def var_head(ST, Wp, bp, eps=None, seed=0, sample=1, gZ=None, gkl=None, H=None, dtype=F64, mm='exact', mutate=None):
    """Both entries from the ABI's arguments: ST [N, >= 2H] (the first 2H columns are read), Wp = (Wp_s, Wp_t) each [2H, H] = mu rows
    over logstd rows, bp likewise [2H], eps [N, >= 2H] or None (generated from `seed`), sample, gZ [N, >= 2H] or None, gkl two floats
    or None.  -> {'Z', 'ML', 'kl' [2], 'dST', 'dWp_s', 'dWp_t', 'dbp_s', 'dbp_t'} in float64, and 'S' for float64 without a defect.
    dtype = F32 with mm = 'x3' is the kernel's arithmetic: bf16x3 products (dense_ref / struct_stage_ref mm3), float32 exp and
    terms, the KL terms widened to float64 at their sum.
    Defects (mutate): ('seed_t',) half t drawn from `seed`; ('swap_rows',) mu and logstd rows of the pack swapped; ('no_2ls',) the
    2 ls term of the KL sum lost; ('dls_no_eps',); ('sample0_noise',) sample = 0 still adds the noise; ('drop_last_tile_kl',) the
    last partial tile's KL terms dropped; ('dwp_tile_lost', g) tile g (the first a workgroup visits second at g workgroups per half)
    missing from dWp and dbp."""
    assert mm == 'exact' or dtype == F32
    kind = mutate[0] if mutate else None
    H = Wp[0].shape[1] if H is None else H
    N = ST.shape[0]
    cv = lambda t: t.to(dtype)       # noqa: E731
    if eps is None:
        E = noise(H, N, seed, same_seed=kind == 'seed_t')
    else:
        E = eps[:, :2 * H]
    E = cv(E.to(F64) if dtype == F64 else E.to(F64).to(F32))
    G = cv(gZ[:, :2 * H]) if gZ is not None else torch.zeros(N, 2 * H, dtype=dtype)
    gk = [0.0, 0.0] if gkl is None else [float(np.float32(g)) for g in gkl]
    noisy = bool(sample) or kind == 'sample0_noise'
    mul = (lambda a, b: mm3(a, b)) if mm == 'x3' else (lambda a, b: a @ b)
    out = {'Z': [], 'ML': [], 'kl': [], 'dST': []}
    S = {'Z': [], 'ML': [], 'kl': [], 'dST': []}
    keep_kl = torch.ones(N, 1, dtype=F64)
    if kind == 'drop_last_tile_kl' and N % TILE:
        keep_kl[N - N % TILE:] = 0
    keep_w = torch.ones(N, 1, dtype=dtype)
    if kind == 'dwp_tile_lost':
        keep_w[mutate[1] * TILE:(mutate[1] + 1) * TILE] = 0
    for h, tag in ((0, 's'), (1, 't')):
        X = cv(ST[:, h * H:(h + 1) * H])
        W, b = cv(Wp[h]), cv(bp[h])
        if kind == 'swap_rows':
            W, b = torch.cat([W[H:], W[:H]]), torch.cat([b[H:], b[:H]])
        P = mul(X, W.t()) + b
        mu, ls = P[:, :H], P[:, H:]
        e, g = E[:, h * H:(h + 1) * H], G[:, h * H:(h + 1) * H]
        sd = torch.exp(ls)
        z = mu + sd * e if noisy else mu.clone()
        two_ls = 0 if kind == 'no_2ls' else 2 * ls
        terms = 1 + two_ls - mu * mu - sd * sd
        kl = (terms.to(F64) * keep_kl).sum()
        dmu = g + gk[h] * (-2 * mu)
        dls = (g * (1 if kind == 'dls_no_eps' else e) * sd if sample else torch.zeros_like(g)) + gk[h] * (2 - 2 * sd * sd)
        dP = torch.cat([dmu, dls], 1)
        out['Z'].append(z); out['ML'].append(P); out['kl'].append(kl)
        out['dST'].append(mul(dP, W))
        out['dWp_' + tag] = mul((dP * keep_w).t().contiguous(), X)
        out['dbp_' + tag] = (dP * keep_w).sum(0)
        if dtype == F64 and mutate is None:
            aX, aW = X.abs(), W.abs()
            SP = aX @ aW.t() + b.abs()
            Smu, Sls = SP[:, :H], SP[:, H:]
            sd2 = sd * sd
            S['ML'].append(SP)
            S['Z'].append(Smu + (sd * e.abs() * (1 + Sls) if noisy else 0))
            S['kl'].append((1 + 2 * Sls + mu * mu + 2 * mu.abs() * Smu + sd2 * (1 + 2 * Sls)).sum())
            Sdmu = g.abs() + 2 * abs(gk[h]) * Smu
            Sdls = ((g * e).abs() * sd * (1 + Sls) if sample else 0) + abs(gk[h]) * (2 + 2 * sd2 + 4 * sd2 * Sls)
            SdP = torch.cat([Sdmu, Sdls], 1)
            S['dST'].append(SdP @ aW)
            S['dWp_' + tag] = SdP.t() @ aX
            S['dbp_' + tag] = SdP.sum(0)
    res = {k: (torch.cat(v, 1) if k != 'kl' else torch.stack(v)).to(F64) for k, v in out.items() if isinstance(v, list)}
    res.update({k: v.to(F64) for k, v in out.items() if not isinstance(v, list)})
    if dtype == F64 and mutate is None:
        res['S'] = {k: (torch.cat(v, 1) if k != 'kl' else torch.stack(v)) if isinstance(v, list) else v for k, v in S.items()}
    return res


def stand_in(c, mutate=None, **kw):
    """The float32 stand-in in the kernel's arithmetic on a case of `case`."""
    return var_head(*args_of(c, **kw), dtype=F32, mm='x3', mutate=mutate, **opts_of(c, **kw))


def exact(c, mutate=None, **kw):
    return var_head(*args_of(c, **kw), mutate=mutate, **opts_of(c, **kw))


def args_of(c, **kw):
    return c['ST'], c['Wp'], c['bp']


def opts_of(c, eps='given', sample=1, gZ=True, gkl=True):
    return dict(eps=c['eps'] if eps == 'given' else None, seed=c['seed'], sample=sample, gZ=c['gZ'] if gZ else None,
                gkl=c['gkl'] if gkl else None, H=c['H'])


def taus(r64, rk):
    """Per output: tau = 8 max(r, 2^-17), r the stand-in's worst ratio against float64 — never a device figure."""
    return {k: 8 * max(DR.ratio(rk[k], r64[k], S), DR.FLOOR['x3']) for k, S in r64['S'].items()}


def ratios(got, r64):
    return {k: DR.ratio(got[k], r64[k], r64['S'][k]) for k in got if k in r64['S']}


# ------------------------------------------------------------------------------------------------ seeded builders
LS_LO, LS_HI = -6.0, 3.0


def heads(H, seed):
    """The eight head parameters of a case as (Wp_s, Wp_t), (bp_s, bp_t): mu rows uniform in +-1/sqrt(H); logstd rows small but for
    column 0, weight 4.5 with bias -1.5, so that logstd follows column 0 of the half's rows over [-6, 3]."""
    g = torch.Generator().manual_seed(1000 + seed)
    Wp, bp = [], []
    for _ in range(2):
        Wm = (torch.rand(H, H, generator=g) * 2 - 1) / H ** 0.5
        Wl = (torch.rand(H, H, generator=g) * 2 - 1) * 0.02 / H ** 0.5
        Wl[:, 0] = (LS_HI - LS_LO) / 2
        bm = (torch.rand(H, generator=g) * 2 - 1) * 0.1
        bl = torch.full((H,), (LS_HI + LS_LO) / 2) + (torch.rand(H, generator=g) * 2 - 1) * 0.01
        Wp.append(torch.cat([Wm, Wl]).to(F32)); bp.append(torch.cat([bm, bl]).to(F32))
    return Wp, bp


def case(H, N, seed=0, wide=False):
    """One designed case.  ST [N, ldst]: rows uniform in +-1, column 0 of each half a ramp over [-1, 1] (in a seeded row order), so
    logstd spans [-6, 3] inside every case of two rows or more.  wide: ldst = 2H + 8, ldz = 2H + 4, ldg = 2H + 12 with NaN in the
    foreign columns (eps keeps 2H + 4 likewise)."""
    g = torch.Generator().manual_seed(77 * H + 13 * seed + N % 9973)
    pad = (8, 4, 12, 4) if wide else (0, 0, 0, 0)
    def rows(extra, scale=1.0):
        t = torch.full((N, 2 * H + extra), NAN, dtype=F32)
        t[:, :2 * H] = (torch.rand(N, 2 * H, generator=g) * 2 - 1) * scale
        return t
    ST = rows(pad[0])
    ramp = torch.linspace(-1, 1, N) if N > 1 else torch.zeros(1)
    ST[:, 0] = ramp[torch.randperm(N, generator=g)]
    ST[:, H] = ramp[torch.randperm(N, generator=g)]
    eps = rows(pad[3])
    eps[:, :2 * H] = torch.randn(N, 2 * H, generator=g)
    Wp, bp = heads(H, seed)
    return {'H': H, 'N': N, 'ST': ST, 'Wp': Wp, 'bp': bp, 'eps': eps, 'gZ': rows(pad[2]), 'gkl': (0.3, -0.2), 'seed': 12345 + seed,
            'ldz': 2 * H + pad[1], 'wide': wide}


def fixture_case(z):
    """g4_vae.npz as a case: the reference's own heads, inputs, noise, upstream gradients and kl_weight (N = 70, H = 64)."""
    H, N = z['s'].shape[1], z['s'].shape[0]
    t = lambda k: torch.from_numpy(np.asarray(z[k]))       # noqa: E731
    Wp = [torch.cat([t('param_fc_%s_mu.weight' % h), t('param_fc_%s_logstd.weight' % h)]) for h in 'st']
    bp = [torch.cat([t('param_fc_%s_mu.bias' % h), t('param_fc_%s_logstd.bias' % h)]) for h in 'st']
    c = -0.5 / N / N                                   # trainer.py:146-147: s_kl = c * klsum_s
    gk = float(z['kl_weight']) * c
    return {'H': H, 'N': N, 'ST': torch.cat([t('s'), t('t')], 1), 'Wp': Wp, 'bp': bp, 'eps': torch.cat([t('eps_s'), t('eps_t')], 1),
            'gZ': torch.cat([t('up_s'), t('up_t')], 1), 'gkl': (gk, gk), 'seed': 0, 'ldz': 2 * H, 'wide': False, 'klcoef': c}


def fixture_expected(z):
    """What the fixture records, in the restatement's names."""
    H = z['s'].shape[1]
    t = lambda k: torch.from_numpy(np.asarray(z[k])).to(F64)       # noqa: E731
    out = {'Z': torch.cat([t('sample_s'), t('sample_t')], 1), 'dST': torch.cat([t('grad_s'), t('grad_t')], 1)}
    for h in 'st':
        out['dWp_' + h] = torch.cat([t('grad_fc_%s_mu.weight' % h), t('grad_fc_%s_logstd.weight' % h)])
        out['dbp_' + h] = torch.cat([t('grad_fc_%s_mu.bias' % h), t('grad_fc_%s_logstd.bias' % h)])
    out['kl_loss'] = torch.stack([t('s_kl'), t('t_kl')])
    assert out['dWp_s'].shape == (2 * H, H)
    return out
