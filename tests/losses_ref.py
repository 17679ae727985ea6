"""Float64 restatements of what csrc/losses.hip and csrc/optim.hip compute, in the words of their specification (plain torch /
numpy on the CPU; the product package is never imported here), and the deterministic input builders the loss tests share.

Every reference takes the float32 data the device sees, lifts it to float64 EXACTLY and computes there; gradients come from
torch autograd of the plain formula.  Beside each gradient the reference returns a per-row (per-element) SCALE: the sum of the
magnitudes of the terms that make up that row.  A kernel's rounding error is a few 2^-24 of that sum; a lost, doubled or stale
list entry is of order one of it — so rows are judged one by one against their own scale and a wrong low-degree row cannot hide
behind a hub (a global max-norm would let it).

    recon      -mean log(sigma(<s_u, t_v>) + 1e-15) over positives - mean log(1 - sigma + 1e-15) over negatives; a half
               without edges contributes 0 (the product's convention, ops.ReconLossFn: sums / max(E, 1))
    func       L1 mean of z(1 - cos(hf[a], hf[b])) - z(tt), z = (x - mean) / unbiased std, cos with each norm clamped at 1e-8
    reparam    z = mu + exp(logstd) * eps, klsum = sum(1 + 2 logstd - mu^2 - exp(logstd)^2)
    adam       torch.optim.Adam's update written out (L2 weight decay enters the gradient in front of the moments)
"""
import numpy as np
import torch

EPS = 1e-15              # dg_ae_model_aig.py:21
F64 = torch.float64
U24 = 2.0 ** -24         # unit roundoff of float32


def _t64(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().cpu().to(F64)


def _idx(x):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().cpu().to(torch.int64)


# ------------------------------------------------------------------------------------------------ decoder / recon
def edge_scores(s, t, edge_index, sigmoid=True, dtype=F64):
    """<s[u], t[v]> (or its sigmoid) per edge (u, v)."""
    s, t, ei = _t64(s).to(dtype), _t64(t).to(dtype), _idx(edge_index)
    v = (s.index_select(0, ei[0]) * t.index_select(0, ei[1])).sum(dim=1)
    return torch.sigmoid(v) if sigmoid else v


def recon(st, pos, neg, gscale=1.0, dtype=F64):
    """Reconstruction loss on st = [s | t] ([N, 2H]) with positives `pos` and negatives `neg` ([2, E] each, either may be empty).
    `dtype=torch.float32` runs the same formula in float32 (the reference's float32 self, for measured tolerances).
    -> dict: loss, sums [2] (the two un-normalised halves), raw / p per edge (positives first), pred [Ep + En] (p > 0.5),
       counts [TP, FP, TN, FN], grad = d(gscale * loss) / d st, coef = d(gscale * loss) / d raw per edge,
       S [N, 2]: per node, the scale of its ds row (sum over its out-edges of |coef| * max|t[partner]|) and of its dt row
       (sum over its in-edges of |coef| * max|s[partner]|),
       dq per edge: the derived bound of |p_float32 - p|, absdot = sum_i |s_i t_i| per edge, sum_bounds [2] / loss_bound: the derived
       bounds of the two sums' and the loss's float32 error (sum resp. mean of dq / q over each half, q = p or 1 - p)."""
    st = _t64(st).to(dtype).requires_grad_(True)
    pos, neg = _idx(pos).reshape(2, -1), _idx(neg).reshape(2, -1)
    N, H = st.shape[0], st.shape[1] // 2
    s, t = st[:, :H], st[:, H:]
    Ep, En = pos.shape[1], neg.shape[1]
    ei = torch.cat([pos, neg], dim=1)
    xs, xt = s.index_select(0, ei[0]), t.index_select(0, ei[1])
    raw = (xs * xt).sum(dim=1)
    raw.retain_grad()
    p = torch.sigmoid(raw)
    sp = -torch.log(p[:Ep] + EPS).sum()
    sn = -torch.log(1 - p[Ep:] + EPS).sum()
    loss = sp / max(Ep, 1) + sn / max(En, 1)
    if Ep + En > 0:
        (loss * gscale).backward()
        grad, coef = st.grad.detach(), raw.grad.detach()
    else:
        grad, coef = torch.zeros_like(st.detach()), torch.zeros(0, dtype=dtype)
    with torch.no_grad():
        S = torch.zeros(N, 2, dtype=dtype)
        S[:, 0].index_add_(0, ei[0], coef.abs() * t.index_select(0, ei[1]).abs().amax(dim=1))
        S[:, 1].index_add_(0, ei[1], coef.abs() * s.index_select(0, ei[0]).abs().amax(dim=1))
        pd = p.detach()
        # |p32 - p|: one rounding each for exp, add and reciprocal and one to spare (4 * 2^-24, p <= 1), plus the dot product's
        # rounding (H * 2^-24 * sum |s_i t_i|, the classical bound of a length-H sum in any order) carried through the slope p (1 - p)
        absdot = (xs * xt).detach().abs().sum(dim=1)
        dq = 4 * U24 + pd * (1 - pd) * H * U24 * absdot
        q = torch.cat([pd[:Ep], 1 - pd[Ep:]])
        rel = dq / q                                        # |d log q| to first order
        bound = (rel[:Ep].mean() if Ep else 0.0) + (rel[Ep:].mean() if En else 0.0)
        pred = (pd > 0.5).to(torch.int32)
        gt = torch.cat([torch.ones(Ep, dtype=torch.int32), torch.zeros(En, dtype=torch.int32)])
    return {'loss': loss.detach(), 'sums': torch.stack([sp, sn]).detach(), 'raw': raw.detach(), 'p': pd, 'pred': pred,
            'counts': confusion(pred, gt), 'grad': grad, 'coef': coef, 'S': S, 'dq': dq, 'absdot': absdot, 'loss_bound': float(bound),
            'sum_bounds': [float(rel[:Ep].sum()), float(rel[Ep:].sum())]}


def row_ratio(got, ref, scale, tiny=1e-30):
    """max over rows of max|got[row] - ref[row]| / scale[row]: the row-wise measure of the gradient tests.  Rows whose scale is 0
    (no terms at all) must hold exactly what the reference holds there; they return inf otherwise."""
    err = (_t64(got) - _t64(ref)).abs()
    err = err.reshape(err.shape[0], -1).amax(dim=1) if err.dim() > 1 else err
    scale = _t64(scale).reshape(-1)
    dead = scale <= tiny
    r = torch.where(dead, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))), err / scale.clamp_min(tiny))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ functional loss
def func(hf, pairs, tt, signs=None, gscale=1.0, add=None, dtype=F64, eps=1e-8):
    """Functional-similarity loss.  `signs` (optional, [P] of -1 / 0 / +1): the L1 branches imposed instead of decided here (the
    device's, as ref_cpu.readout_prob(decisions=) does for the readout); `add` [N, H]: gradient of a second consumer of hf, added
    to the result (the pass-through).
    -> dict: dis [P], sums [7] in the kernel's order (sum d, sum d^2, sum t, sum t^2, sum |zd - zt|, sum sgn, sum sgn * zd),
       sums_abs [7] (the same sums over the terms' magnitudes), diff = zd - zt, sgn (this run's own decisions), loss,
       grad = d(gscale * loss) / d hf (+ add), dc = d(gscale * loss) / d cos per pair,
       S [N]: per row sum over its pairs of |dc|_terms * max|other row| / (n_a n_b) (clamped norms; |dc|_terms: the magnitudes of
       the three terms of dc, see below), bound_dis [P]."""
    hf = _t64(hf).to(dtype).requires_grad_(True)
    pr = _idx(pairs).reshape(2, -1)
    tt = _t64(tt).to(dtype)
    P = pr.shape[1]
    a, b = hf.index_select(0, pr[0]), hf.index_select(0, pr[1])
    # cosine_similarity(eps) written out: <a, b> / (max(|a|, eps) max(|b|, eps)).  Its value is torch's; its derivative is the
    # formula's own — a clamped norm is a constant.  torch.nn.functional.cosine_similarity clamps in place under no_grad, so its
    # autograd differentiates |a| even while the clamp holds: for 0 < |a| < eps it adds an own-row term -cos * a / (eps |a|) that the
    # formula does not have (tests/test_losses_spec.py shows both; for |a| = 0 and |a| > eps the two agree to the last bit).
    cos = (a * b).sum(dim=1) / (a.norm(dim=1).clamp_min(eps) * b.norm(dim=1).clamp_min(eps))
    cos.retain_grad()
    dis = 1 - cos
    zd = (dis - dis.mean()) / dis.std()
    zt = (tt - tt.mean()) / tt.std()
    diff = zd - zt
    own = torch.sign(diff.detach())
    sg = own if signs is None else _t64(signs).to(dtype)
    loss = (sg * diff).sum() / P                   # = F.l1_loss(zd, zt) on this run's own signs
    (loss * gscale).backward()
    grad = hf.grad.detach()
    if add is not None:
        grad = grad + _t64(add).to(dtype)
    with torch.no_grad():
        dc = cos.grad.detach()
        na, nb = a.norm(dim=1).clamp_min(eps), b.norm(dim=1).clamp_min(eps)
        # d loss / d cos = -k (sgn - mean(sgn) - zd * sum(sgn * zd) / (P - 1)), k = gscale / (P * std): a difference of O(1) terms that
        # cancels to nothing for some pairs (for all of them at P = 2, where zd is the constant +-1 / sqrt(2)); the scale takes the terms'
        # magnitudes, which is >= |dc| and within a small factor of it wherever nothing cancels
        k = abs(float(gscale)) / (P * dis.detach().std())
        dc_abs = k * (sg.abs() + sg.mean().abs() + (zd.detach() * (sg * zd.detach()).sum() / (P - 1)).abs())
        w = dc_abs / (na * nb)
        # a row's terms are dc * (other / (n_a n_b) - cos * own / n_own^2); the second is at most sqrt(H) times the first's size
        # (|cos| <= 1, max|x| / |x| in [1 / sqrt(H), 1]) and vanishes with it, so the first term's magnitude serves as the scale
        S = torch.zeros(hf.shape[0], dtype=dtype)
        S.index_add_(0, pr[0], w * b.abs().amax(dim=1))
        S.index_add_(0, pr[1], w * a.abs().amax(dim=1))
        d_, z_ = dis.detach(), zd.detach()
        sums = torch.stack([d_.sum(), (d_ * d_).sum(), tt.sum(), (tt * tt).sum(), diff.detach().abs().sum(), sg.sum(), (sg * z_).sum()])
        sums_abs = torch.stack([d_.abs().sum(), (d_ * d_).sum(), tt.abs().sum(), (tt * tt).sum(), diff.detach().abs().sum(),
                                sg.abs().sum(), z_.abs().sum()])
        # three length-H float32 sums (any order) and a handful of roundings around the division
        bound_dis = 4 * U24 + hf.shape[1] * U24 * (a * b).detach().abs().sum(dim=1) / (na * nb)
    return {'dis': d_, 'sums': sums, 'sums_abs': sums_abs, 'diff': diff.detach(), 'sgn': own, 'loss': loss.detach(), 'grad': grad,
            'dc': dc, 'S': S, 'bound_dis': bound_dis, 'zd': z_}


# ------------------------------------------------------------------------------------------------ sampler + KL
def reparam(mu, logstd, eps, gz=None, gkl=None, klcoef=1.0):
    """-> dict: z, kl (the sum), kl_abs (sum of the terms' magnitudes), z_abs = |mu| + e^l |eps|, dmu, dls and their term
    magnitudes dmu_abs, dls_abs for the upstream gradients gz (per element or None) and gkl (scalar or None)."""
    mu, ls, eps = _t64(mu), _t64(logstd), _t64(eps)
    sd = torch.exp(ls)
    z = mu + sd * eps
    kl = (1 + 2 * ls - mu * mu - sd * sd).sum()
    kl_abs = (1 + 2 * ls.abs() + mu * mu + sd * sd).sum()
    g = _t64(gz) if gz is not None else torch.zeros_like(mu)
    gk = float(gkl) * float(klcoef) if gkl is not None else 0.0
    dmu = g + gk * (-2 * mu)
    dls = g * eps * sd + gk * (2 - 2 * sd * sd)
    return {'z': z, 'kl': kl, 'kl_abs': kl_abs, 'z_abs': mu.abs() + sd * eps.abs(), 'dmu': dmu, 'dls': dls,
            'dmu_abs': g.abs() + abs(gk) * 2 * mu.abs(), 'dls_abs': (g * eps).abs() * sd + abs(gk) * (2 + 2 * sd * sd)}


_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def mix32_scalar(x):
    """The low 32 bits of the 64-bit finaliser of losses.hip (`mix32`) for ONE value, in plain Python integers mod 2^64."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x & 0xFFFFFFFF


def gauss_words(seed, n, start=0):
    """(a, b): the two 32-bit hash words of elements start .. start + n - 1, `mix32(seed * GOLD + 2 i)` and `... + 2 i + 1`, as
    numpy uint64 arrays (uint64 ARRAY arithmetic wraps mod 2^64, as the kernel's does)."""
    base = np.uint64((int(seed) * _GOLD) & _M64)
    i2 = np.arange(start, start + n, dtype=np.uint64) * np.uint64(2)
    out = []
    for off in (0, 1):
        x = i2 + np.uint64(off)
        x += base
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
        out.append(x & np.uint64(0xFFFFFFFF))
    return out[0], out[1]


def gauss_uniforms(seed, n, start=0):
    """(u1, u2) in float32 exactly as the kernel forms them: u1 = ((a >> 8) + 1) / 2^24 in (0, 1], u2 = (b >> 8) / 2^24 in [0, 1)."""
    a, b = gauss_words(seed, n, start)
    u1 = ((a >> np.uint64(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    u2 = (b >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u1, u2


def gauss_from_counter(seed, n, start=0):
    """The built-in Gaussian generator of mgv_reparam_fwd restated: Box-Muller sqrt(-2 ln u1) cos(2 pi u2) in float64 on the
    kernel's own float32 uniforms.  -> numpy float64 [n]"""
    u1, u2 = gauss_uniforms(seed, n, start)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


# |device - gauss_from_counter| floor: the kernel scales u2 by 2 pi in float32 (an argument error up to 2 pi * 2^-24) and the radius is
# at most sqrt(2 * 24 * ln 2) = 5.77
GAUSS_FLOOR = 2 * np.pi * U24 * np.sqrt(2 * 24 * np.log(2.0))      # 2.2e-6


# ------------------------------------------------------------------------------------------------ Adam
def adam(p, g_seq, m, v, lr, betas, eps, wd, grad_scale, first_step=1):
    """torch.optim.Adam (amsgrad off, maximize off) over the gradient sequence g_seq [K, n], the k-th applied as step
    first_step + k:   g = grad_scale * g_k (+ wd * p);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
                      p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    -> dict p, m, v (float64) and m_scale, v_scale: per element sum_k (1 - b1) b1^(K-1-k) |g| (+ b1^K |m_0|) and its square analogue."""
    p, m, v = _t64(p).clone(), _t64(m).clone(), _t64(v).clone()
    g_seq = _t64(g_seq)
    b1, b2 = float(betas[0]), float(betas[1])
    ms, vs = m.abs(), v.abs()
    for k in range(g_seq.shape[0]):
        t = first_step + k
        g = g_seq[k] * float(grad_scale)
        if wd != 0:
            g = g + float(wd) * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        ms = b1 * ms + (1 - b1) * g.abs()
        vs = b2 * vs + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        p = p - (float(lr) / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + float(eps)))
    return {'p': p, 'm': m, 'v': v, 'm_scale': ms, 'v_scale': vs}


def f32(x):
    """A Python float rounded to float32 (what a C `float` argument of the ABI receives), as a Python float again."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ confusion
def confusion(pred, gt):
    """[TP, FP, TN, FN] as Python ints; entries of pred / gt other than 0 / 1 are counted nowhere."""
    p = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred).astype(np.int64).ravel()
    g = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt).astype(np.int64).ravel()
    return [int(np.count_nonzero((p == 1) & (g == 1))), int(np.count_nonzero((p == 1) & (g == 0))),
            int(np.count_nonzero((p == 0) & (g == 0))), int(np.count_nonzero((p == 0) & (g == 1)))]


# ================================================================================================ input builders
HEAVY_ROW, HEAVY_SEG = 64, 512                  # GraphPlan.HEAVY_ROW / HEAVY_SEG (asserted equal in the GPU tests)
LIST_TOTALS = (1, 3, 4, 5, 8, 9, 63, 64, 65)    # per-node totals over the four lists that the chunked walk must get right (0: the idle nodes)
HUBS = ((512, 512), (513, 513), (3000, 2100), (700, 0))      # (positive out, positive in) list lengths; the last is heavy on the out side only
BAND = 1e-3                                     # no recon score inside (-BAND, BAND) other than exact zeros
DESIGNED_MIN_N = 4096                           # from here on build_recon lays out the designed nodes; below: random lists only


def _rows(rng, n, H, lo, hi):
    """n rows of random direction whose 2-norm is uniform in [lo, hi]."""
    x = rng.standard_normal((n, H))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x * rng.uniform(lo, hi, size=(n, 1))


def build_recon(N, H, seed, wide=False, want_pos=True, want_neg=True, hubs=True):
    """Deterministic decoder / reconstruction-loss case.  -> dict st [N, 2H] float32 tensor, pos / neg [2, E] int64 tensors, meta.
    Rows have 2-norm <= sqrt(B), B = 6 ('moderate') or 14 ('wide': a few hundred aligned / anti-aligned pairs reach the ends), so
    |score| <= B; one row in 53 is all zero (score exactly 0, p = 0.5: "not a hit" on both sides).
    N >= DESIGNED_MIN_N: nodes [0, n_designed) are laid out by hand, the rest is a pool with random lists —
      * for every total k in LIST_TOTALS five nodes whose four lists (positive out / in, negative out / in) hold k entries in all:
        all in one list (one node per list) and spread over the four;
      * the HUBS; idle nodes in no list at all; duplicates of positive and of negative pairs; self loops.
    A designed node's partners come from the pool, and an edge whose score falls inside (-BAND, BAND) without being an exact zero
    has its pool end redrawn, so the designed list lengths hold.  Below DESIGNED_MIN_N: random pairs (duplicates and self loops
    included), offending pairs dropped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = 14.0 if wide else 6.0
    r = np.sqrt(B)
    st = np.concatenate([_rows(rng, N, H, 0.3 * r, r), _rows(rng, N, H, 0.3 * r, r)], axis=1)
    zero_rows = np.arange(7, N, 53)
    st[zero_rows] = 0.0
    pos, neg = [], []
    designed = {}
    n_designed = 0
    if N >= DESIGNED_MIN_N:
        nid = 0
        pool_lo = 1024
        def pool(k):
            return rng.integers(pool_lo, N, size=k)
        for k in LIST_TOTALS:
            for pat in range(5):
                cnt = [0, 0, 0, 0]
                if pat < 4:
                    cnt[pat] = k
                else:
                    for j in range(k):
                        cnt[j % 4] += 1
                    cnt = cnt[1:] + cnt[:1] if k % 2 else cnt          # vary which list takes the remainder
                if (not want_pos and (cnt[0] or cnt[1])) or (not want_neg and (cnt[2] or cnt[3])):
                    continue
                u = nid; nid += 1
                designed[u] = tuple(cnt)
                pos += [(u, int(v)) for v in pool(cnt[0])] + [(int(v), u) for v in pool(cnt[1])]
                neg += [(u, int(v)) for v in pool(cnt[2])] + [(int(v), u) for v in pool(cnt[3])]
        if hubs and want_pos:
            for (ko, ki) in HUBS:
                u = nid; nid += 1
                designed[u] = (ko, ki, 0, 0)
                pos += [(u, int(v)) for v in pool(ko)] + [(int(v), u) for v in pool(ki)]
        idle = list(range(nid, nid + 40))            # more than two workgroups' rows at H = 64: whole workgroups without work
        nid += 40
        for u in idle:
            designed[u] = (0, 0, 0, 0)
        n_designed = nid
        assert n_designed <= pool_lo
        # nodes [n_designed, pool_lo) stay idle as well; the pool gets random lists, duplicates and self loops
        npool = N - pool_lo
        if want_pos:
            e = rng.integers(pool_lo, N, size=(2 * npool, 2))
            pos += [tuple(x) for x in e.tolist()]
            pos += pos[-50:]                                        # duplicates of positive pairs
            pos += [(int(v), int(v)) for v in pool(30)]             # self loops
        if want_neg:
            e = rng.integers(pool_lo, N, size=(2 * npool + 17, 2))
            neg += [tuple(x) for x in e.tolist()]
            neg += neg[-40:]
            neg += [(int(v), int(v)) for v in pool(10)]
        if wide:
            # aligned / anti-aligned pairs at the full norm: scores at +-B
            for lst, on in ((pos, want_pos), (neg, want_neg)):
                if not on:
                    continue
                for j in range(150):
                    u, v = int(pool(1)[0]), int(pool(1)[0])
                    if u == v or u % 53 == 7 or v % 53 == 7:           # (not the zero rows)
                        continue
                    d = st[u, :H] / np.linalg.norm(st[u, :H])
                    st[u, :H] = d * r
                    st[v, H:] = d * r * (1 if j % 2 else -1)
                    lst.append((u, v))
    else:
        for lst, on, mult in ((pos, want_pos, 3), (neg, want_neg, 4)):
            if on:
                e = rng.integers(0, N, size=(mult * N + 2, 2))
                lst += [tuple(x) for x in e.tolist()]
                lst += lst[:3]
                lst.append((N - 1, N - 1))
    st32 = st.astype(np.float32)
    s64, t64 = st32[:, :H].astype(np.float64), st32[:, H:].astype(np.float64)

    def fix(lst):
        e = np.asarray(lst, dtype=np.int64).reshape(-1, 2)
        for _ in range(50):
            if e.shape[0] == 0:
                break
            sc = (s64[e[:, 0]] * t64[e[:, 1]]).sum(axis=1)
            bad = (np.abs(sc) < BAND) & (sc != 0.0)
            if not bad.any():
                break
            if N >= DESIGNED_MIN_N:
                for i in np.flatnonzero(bad):
                    end = 1 if e[i, 0] < n_designed else 0          # redraw the pool end (either end of a pool-pool pair)
                    e[i, end] = rng.integers(1024, N)
            else:
                e = e[~bad]
        return torch.from_numpy(np.ascontiguousarray(e.T))
    out = {'st': torch.from_numpy(st32), 'pos': fix(pos), 'neg': fix(neg), 'H': H, 'N': N, 'B': B, 'designed': designed,
           'zero_rows': zero_rows}
    return out


def list_totals(case):
    """Per node (positive out, positive in, negative out, negative in) list lengths of a build_recon case, int64 [N, 4]."""
    N = case['N']
    return np.stack([np.bincount(case['pos'][0].numpy(), minlength=N), np.bincount(case['pos'][1].numpy(), minlength=N),
                     np.bincount(case['neg'][0].numpy(), minlength=N), np.bincount(case['neg'][1].numpy(), minlength=N)], axis=1)


FUNC_MARGIN = 1e-4       # every |zd - zt| of a build_func case is at least this in float64: L1 signs are compared exactly


def build_func(N, H, P, seed, signed=False, tiny=True):
    """Deterministic functional-loss case.  -> dict hf [N, H] float32, pairs [2, P] int64, tt [P] float32.
    hf >= 0 unless `signed`; one row in seven is exactly zero (never-updated nodes: the clamped-norm branch) and, with `tiny`, one
    in 29 has norm 5e-9 (clamped WITHOUT being zero: there the gradient's own-row term must be absent, not merely multiplied by a
    zero dot product); pairs hit such rows on either and on both sides, include a == b and repeated pairs; the last tenth of the nodes
    is in no pair (N >= 10).  tt is drawn
    uniformly and then moved, pair by pair, wherever |zd - zt| < 2 * FUNC_MARGIN, until none is left."""
    rng = np.random.Generator(np.random.PCG64(seed))
    hf = rng.uniform(-1.0, 1.0, size=(N, H))
    if not signed:
        hf = np.abs(hf)
    if tiny:
        hf[5::29] *= 5e-9 / np.linalg.norm(hf[5::29], axis=1, keepdims=True)      # |row| = eps / 2: clamped without being zero
    hf[3::7] = 0.0
    hf32 = hf.astype(np.float32)
    n_in = N - N // 10 if N >= 10 else N
    pa, pb = rng.integers(0, n_in, size=P), rng.integers(0, n_in, size=P)
    if P >= 16:
        pb[5] = pa[5]                                   # a == b
        pa[7], pb[7] = pa[6], pb[6]                     # a repeated pair
        if n_in > 10:
            pa[8], pb[8] = 3, 10                        # zero rows on both sides
            pa[9] = 3                                   # ... on the first side
            pb[10] = 10                                 # ... on the second side
            pa[11], pb[12] = 5, 34                      # clamped non-zero rows on either side
    tt = rng.uniform(0.0, 1.0, size=P).astype(np.float32)
    if P == 2:
        pa, pb = np.array([0, min(1, N - 1)]), np.array([min(2, N - 1), min(4, N - 1)])
    x = hf32.astype(np.float64)
    a, b = x[pa], x[pb]
    na, nb = np.maximum(np.linalg.norm(a, axis=1), 1e-8), np.maximum(np.linalg.norm(b, axis=1), 1e-8)
    dis = 1.0 - (a * b).sum(axis=1) / (na * nb)
    zd = (dis - dis.mean()) / dis.std(ddof=1)
    if P == 2:
        # two values normalise to -+1 / sqrt(2) whatever they are: zd - zt is 0 or +-sqrt(2); the targets take the opposite order
        tt = np.array([0.75, 0.25] if dis[0] < dis[1] else [0.25, 0.75], dtype=np.float32)
    if P > 2:
        for _ in range(100):
            t64 = tt.astype(np.float64)
            diff = zd - (t64 - t64.mean()) / t64.std(ddof=1)
            bad = np.flatnonzero(np.abs(diff) < 2 * FUNC_MARGIN)
            if bad.size == 0:
                break
            tt[bad] = (tt[bad] + rng.uniform(0.02, 0.2, size=bad.size).astype(np.float32)) % np.float32(1.0)
        else:
            raise AssertionError('build_func: could not clear the sign margin')
    return {'hf': torch.from_numpy(hf32), 'pairs': torch.from_numpy(np.stack([pa, pb]).astype(np.int64)), 'tt': torch.from_numpy(tt),
            'N': N, 'H': H, 'P': P, 'n_in': n_in}


def build_adam(n, K, seed, first_nonzero_at=None):
    """Gradient sequence [K, n] float32 whose per-element magnitudes span 1e-8 .. 1 (logspace over the elements, random sign and a
    factor in [0.5, 1.5] per step); every 11th element has gradient exactly zero throughout, every 13th is zero for the first
    K // 2 steps and live afterwards.  Parameters start in [-1, 1]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mag = np.logspace(-8, 0, n) if n > 1 else np.array([1e-3])
    mag = mag[rng.permutation(n)]
    g = mag[None, :] * rng.uniform(0.5, 1.5, size=(K, n)) * rng.choice([-1.0, 1.0], size=(K, n), p=[0.3, 0.7])
    dead = np.arange(n) % 11 == 4
    late = np.arange(n) % 13 == 6
    g[:, dead] = 0.0
    g[:K // 2, late & ~dead] = 0.0
    p = rng.uniform(-1.0, 1.0, size=n)
    return {'g': torch.from_numpy(g.astype(np.float32)), 'p': torch.from_numpy(p.astype(np.float32)), 'dead': dead, 'late': late & ~dead}


# ------------------------------------------------------------------------------------------------ the cases both test files run
def rows_per_workgroup(H):
    """Rows a 256-thread workgroup of the float4 routes takes per trip (H / 4 lanes per row)."""
    return 1024 // H


GRID_CAP = 2048          # mgv_common.h grid_for(tiles, 8): 256 * 8 workgroups


def recon_sizes(H):
    """{name: N}: the small sizes, a size whose grid is a multiple of 8 with a short last XCD range, one whose grid is not a
    multiple of 8, and one past the grid cap (a second grid-stride trip).  The last three are >= DESIGNED_MIN_N."""
    rpb = rows_per_workgroup(H)
    k = max(40, -(-(DESIGNED_MIN_N + 8) // (8 * rpb)))
    out = {'n%d' % n: n for n in (1, 15, 16, 17, 127, 129)}
    out['xcd_short'] = 8 * rpb * 5 - 3                      # small lists, grid = 40
    out['xcd'] = 8 * rpb * k - 3                            # grid = 8 k, the last range three rows short
    out['odd'] = 8 * rpb * k + 3 * rpb + 1                  # grid = 8 k + 4
    out['cap'] = GRID_CAP * rpb + 17
    return out


def recon_case(H, size, wide=False, want_pos=True, want_neg=True):
    N = recon_sizes(H)[size]
    seed = 1000 * H + sorted(recon_sizes(H)).index(size) + (500 if wide else 0)
    return build_recon(N, H, seed, wide=wide, want_pos=want_pos, want_neg=want_neg)


FUNC_P = (2, 3, 255, 257, 65539, GRID_CAP * 256 + 13)       # the last: past k_func_l1's grid cap


def func_case(H, P, signed=False, tiny=True):
    N = 1001 if P < 60000 else 30011                         # neither a multiple of 16, 32 or 64
    return build_func(N, H, P, seed=7 * H + P % 1000 + (1 if signed else 0), signed=signed, tiny=tiny)
