"""Float64 restatement of the reconstruction loss's one-walk route (csrc/losses.hip: k_recon_bwd_pull2<H, true> and
k_recon_heavy_seg<H, true>, entries mgv_recon_step_csr / mgv_recon_step_heavy_lists), in the words of the walk, and the small
designed cases its tests run.  Plain numpy / torch on the CPU; the product package is never imported here.

The walk visits every node's OUT lists — positive, then negative — and each entry (u, v) there is one pair of the loss, seen exactly
once: p = sigma(<s_u, t_v>), a positive adds -log(p + 1e-15) to sums[0], a negative -log(1 - p + 1e-15) to sums[1], `p > 0.5` is a
hit (TP / FP) and anything else a miss (FN / TN).  The in lists carry no loss term.

Bound of the two sums.  tests/losses_ref.py derives, for mgv_recon_loss_fwd, |p32 - p| <= dq = 4 * 2^-24 + p (1 - p) H 2^-24 sum_i
|s_i t_i| per pair and |term32 - term| <= dq / q (q = p or 1 - p), and adds 1e-12 relative for the accumulation in double.  That
derivation is per TERM; how the terms are grouped enters only through the accumulation.  The walk forms each term by the same float
expressions and adds them in double from the first addition on (per thread, per workgroup, slab rows in index order), so the
same bound holds for it whatever the lists look like; it is computed here from the lists, not taken from losses_ref."""
import numpy as np
import torch

EPS = 1e-15
U24 = 2.0 ** -24
HEAVY_ROW = 64           # GraphPlan.HEAVY_ROW (asserted equal in the GPU tests)


def by_source(pairs, N):
    """(ptr [N + 1], dst [E]) of the pairs [2, E] grouped by source, each list in pair order (what a by-source CSR holds)."""
    e = np.asarray(pairs, dtype=np.int64).reshape(2, -1)
    order = np.argsort(e[0], kind='stable')
    ptr = np.concatenate([[0], np.cumsum(np.bincount(e[0], minlength=N))]).astype(np.int64)
    return ptr, e[1][order]


def walk(st, pos, neg):
    """-> dict sums [2], bounds [2] (see the module docstring), counts [TP, FP, TN, FN] as decided in float64, near: the number of
    pairs whose float64 score is within 1e-3 of 0 without being 0 (their hit decision may differ in float32)."""
    st = np.asarray(st.detach().cpu().numpy() if torch.is_tensor(st) else st).astype(np.float64)
    N, H = st.shape[0], st.shape[1] // 2
    s, t = st[:, :H], st[:, H:]
    sums, bounds, counts, near = [0.0, 0.0], [0.0, 0.0], [0, 0, 0, 0], 0
    for half, pairs in enumerate((pos, neg)):
        ptr, dst = by_source(pairs.cpu().numpy() if torch.is_tensor(pairs) else pairs, N)
        for u in range(N):
            for v in dst[ptr[u]:ptr[u + 1]]:
                prod = s[u] * t[v]
                raw = prod.sum()
                p = 1.0 / (1.0 + np.exp(-raw))
                q = p if half == 0 else 1.0 - p
                sums[half] += -np.log(q + EPS)
                bounds[half] += (4 * U24 + p * (1 - p) * H * U24 * np.abs(prod).sum()) / q
                hit = p > 0.5
                counts[(0 if hit else 3) if half == 0 else (1 if hit else 2)] += 1
                near += int(abs(raw) < 1e-3 and raw != 0.0)
    bounds = [bounds[k] + 1e-12 * abs(sums[k]) for k in range(2)]
    return {'sums': sums, 'bounds': bounds, 'counts': counts, 'near': near}


def rows_per_workgroup(H):
    return 1024 // H


def sizes(H):
    """{name: N}: about 300 nodes — 'odd' leaves a partial last workgroup on a grid that is no multiple of 8 (the plain
    grid-stride ranges), 'xcd' a grid that is one (the XCD-contiguous ranges, the last one three rows short) — and N = 1."""
    rpb = rows_per_workgroup(H)
    k = -(-300 // (8 * rpb))
    out = {'one': 1, 'odd': 301, 'xcd': 8 * rpb * k - 3}
    assert (-(-out['odd'] // rpb)) % 8 != 0 and out['odd'] % rpb != 0 and (-(-out['xcd'] // rpb)) % 8 == 0
    return out


LIST_LENGTHS = (1, 3, 4, 5, 9)      # on both sides of the walk's four-entry chunks


def build(H, size, seed=0, want_pos=True, want_neg=True, heavy=True):
    """-> dict st [N, 2H] float32, pos / neg [2, E] int64, N, H, designed {node: (positive out, positive in, negative out, negative
    in) list lengths}.  Node 0 is in no list; for every k in LIST_LENGTHS four nodes hold k entries in one of their four lists and a
    fifth spreads k over the four; one positive and one negative self pair; with `heavy`, node 30 has a positive out-list of
    HEAVY_ROW + 6 entries; a pool of random pairs (duplicates included) over nodes [40, N); one row in 53 is all zero (score exactly
    0, p = 0.5: a miss on both sides).  N = 1: the self pairs only."""
    N = sizes(H)[size]
    rng = np.random.Generator(np.random.PCG64(1000 * H + 7 * seed + N))
    r = np.sqrt(6.0)
    st = rng.standard_normal((N, 2 * H))
    for half in (slice(0, H), slice(H, 2 * H)):
        st[:, half] *= rng.uniform(0.3 * r, r, size=(N, 1)) / np.linalg.norm(st[:, half], axis=1, keepdims=True)
    st[7::53] = 0.0
    pos, neg, designed = [], [], {}
    if N == 1:
        pos, neg = [(0, 0)], [(0, 0), (0, 0)]
    else:
        def pool(k):
            return [int(v) for v in rng.integers(40, N, size=k)]
        designed[0] = (0, 0, 0, 0)
        u = 1
        for k in LIST_LENGTHS:
            for pat in range(5):
                cnt = [0, 0, 0, 0]
                if pat < 4:
                    cnt[pat] = k
                else:
                    for j in range(k):
                        cnt[(j + k) % 4] += 1
                designed[u] = tuple(cnt)
                pos += [(u, v) for v in pool(cnt[0])] + [(v, u) for v in pool(cnt[1])]
                neg += [(u, v) for v in pool(cnt[2])] + [(v, u) for v in pool(cnt[3])]
                u += 1
        assert u <= 30
        if heavy:
            designed[30] = (HEAVY_ROW + 6, 0, 0, 0)
            pos += [(30, v) for v in pool(HEAVY_ROW + 6)]
        pos += [(50, 50)]
        neg += [(51, 51)]
        e = rng.integers(40, N, size=(2 * N, 2)).tolist()
        pos += [tuple(x) for x in e] + [tuple(x) for x in e[:5]]
        e = rng.integers(40, N, size=(2 * N + 3, 2)).tolist()
        neg += [tuple(x) for x in e] + [tuple(x) for x in e[:4]]
    if not want_pos:
        pos = []
    if not want_neg:
        neg = []

    def as_pairs(lst):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(lst, dtype=np.int64).reshape(-1, 2).T))
    return {'st': torch.from_numpy(st.astype(np.float32)), 'pos': as_pairs(pos), 'neg': as_pairs(neg), 'N': N, 'H': H, 'designed': designed}


def build_marginal(H, N=300, seed=0):
    """A case whose every score is rounding noise around 0: pair k joins s[k] with a t row made orthogonal to it in float64 and only
    then rounded to float32 (positives (k, N/2 + k), negatives (N/2 + k, k)), rows of norm sqrt(14).  The float32 score then is
    whatever the order and the fusing of the dot product's roundings leave, a few 2^-24 * sum |s_i t_i| of either sign, while
    the sigmoid leaves 0.5 only beyond |score| = 6e-8: `p > 0.5` is decided by the last bits.  Two kernels agree on all the
    hits only if they form the score by the same float operations.  -> dict as `build`, plus margin [E]: |score| / (2^-24 sum
    |s_i t_i|) per pair in float64 (asserted small by the test)."""
    rng = np.random.Generator(np.random.PCG64(77 * H + seed))
    half = N // 2
    st = rng.standard_normal((N, 2 * H))
    r = np.sqrt(14.0)
    pos = [(k, half + k) for k in range(half)]
    neg = [(half + k, k) for k in range(half)]
    for u, v in pos + neg:
        a, b = st[u, :H], st[v, H:]
        b -= a * (a @ b) / (a @ a)
    for sl in (slice(0, H), slice(H, 2 * H)):
        st[:, sl] *= r / np.linalg.norm(st[:, sl], axis=1, keepdims=True)
    st32 = st.astype(np.float32)
    x = st32.astype(np.float64)
    e = np.asarray(pos + neg, dtype=np.int64)
    prod = x[e[:, 0], :H] * x[e[:, 1], H:]
    margin = np.abs(prod.sum(axis=1)) / (U24 * np.abs(prod).sum(axis=1))

    def as_pairs(lst):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(lst, dtype=np.int64).reshape(-1, 2).T))
    return {'st': torch.from_numpy(st32), 'pos': as_pairs(pos), 'neg': as_pairs(neg), 'N': N, 'H': H, 'designed': {}, 'margin': margin}


def list_lengths(case):
    """int64 [N, 4]: per node the (positive out, positive in, negative out, negative in) list lengths of a case."""
    N = case['N']
    return np.stack([np.bincount(case['pos'][0].numpy(), minlength=N), np.bincount(case['pos'][1].numpy(), minlength=N),
                     np.bincount(case['neg'][0].numpy(), minlength=N), np.bincount(case['neg'][1].numpy(), minlength=N)], axis=1)
