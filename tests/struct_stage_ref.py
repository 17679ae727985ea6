"""Plain restatement of ONE structural-encoder half round (AggConv -> GRU -> LayerNorm, digae_layer.py:267-275) and its backward
under torch autograd, working from exactly what the C ABI of the struct-stage kernels takes (include/mgvae_hip.h), plus the
builders of the cases tests/test_hip_struct_stage_reference.py runs on the device.  CPU only; pinned to the reference project's
fixture and to oracle/ref_cpu.py by tests/test_struct_stage_spec.py, which also asserts the properties of the builders.

half_round(case, dtype, mm):
  agg[n] = sum_e h_in[nbr_row(e)],  gi = agg Wc^T + deg bc + xtab[xcls]  (or + xrow[n], the general-feature form),
  gh = h_own Whh^T + bhh,  h_own[n] = h_in[own_idx[n]] (own_idx None: row n),  torch's GRU gate order r, z, n,
  LayerNorm with eps 1e-5 (ln_w None: none).  nbr_row(e) is the entry itself; in tagged mode it is the entry's top byte and
  gy_agg is indexed by the low 24 bits.  Incoming gradient dY[n] = gy_direct[n] + sum_e gy_agg[node(e)].
  mm = 'x3' (float32 only): every matrix product (forward, dgrad, wgrad) is hi.hi + hi.lo + lo.hi of the operands' bf16 planes,
  hi = bf16(x), lo = bf16(x - hi), accumulated in float32: the CPU stand-in for the bf16x3 kernels' arithmetic.
  mm = 'exact' with dtype float32 is the stand-in for the fp32 kernels.

Scales S (float64 only): the sums of the magnitudes of the terms behind each output entry, so that an error is judged against what
the entry was summed from and not against the tensor's largest entry:
  g_agg row n   max_j sum_i |Wc[i,j]| |dGi[n,i]|          g_direct row n  max_j (sum_i |Whh[i,j]| |dGh[n,i]| + |dpre[n,j]| z[n,j])
  dWc[i,j]      sum_n |dGi[n,i]| |agg[n,j]|               dWhh[i,j]       sum_n |dGh[n,i]| |h_own[n,j]|
  dbc[i]        sum_n deg[n] |dGi[n,i]|                   dxtab[c,i]      sum_{cls=c} |dGi[n,i]|     dxrow row n: max_i |dGi[n,i]|
  dbhh[i]       sum_n |dGh[n,i]|        dln_w[j] sum_n |dY xhat|        dln_b[j] sum_n |dY|
  h_out row n   max(1, max|row|)        mean[n]  max(1, max|pre row|)    rstd[n]  rstd[n] (relative)
"""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
LN_EPS = 1e-5
TILE = 64                   # rows per workgroup tile (csrc/mgv_common.h kTileRows)
IDX_CAP = 512               # kIdxCap: index entries of a tile staged in LDS
CHUNK_CUT = IDX_CAP - 8     # a full tile whose list total exceeds this takes the generic row path (tile_dmax)
HEAVY_ROW = 64              # kHeavyRow: rows with MORE entries are listed for the pre-pass
GRID_CAP = 256              # grid_for: workgroups per launch and co-resident workgroup per CU

ROW_OUT = ('h_out', 'mean', 'rstd', 'g_direct', 'g_agg', 'dxrow')
PARAM_OUT = ('dWc', 'dbc', 'dWhh', 'dbhh', 'dxtab', 'dln_w', 'dln_b')


# ------------------------------------------------------------------------------------------------ arithmetic
def _split(x):
    hi = x.to(torch.bfloat16).to(F32)
    lo = (x - hi).to(torch.bfloat16).to(F32)
    return hi, lo


def mm3(a, b):
    """a @ b on bf16 planes: hi.hi + hi.lo + lo.hi (products of bf16 values are exact in float32; float32 accumulation)."""
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bh + (ah @ bl + al @ bh)


class _Lin3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return mm3(x, W.t())

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        return mm3(g, W), mm3(g.t(), x)


def _entries(c):
    """(row of each entry, h_in row it names, gradient row it names) as int64."""
    ptr = c['ptr'].long()
    E = int(ptr[-1])
    deg = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(c['N']), deg)
    ent = c['idx'][:E].long() & 0xffffffff
    if c['tagged']:
        return rows, ent >> 24, ent & 0xffffff
    return rows, ent, ent


def half_round(c, dtype=F64, mm='exact', mutate=None):
    """See the module docstring.  `mutate` = (kind, ...) plants ONE defect in the restatement (tests/test_struct_stage_spec.py shows
    that each of them is far outside the bound the device tests assert); scales are returned for float64 without a defect only."""
    assert mm == 'exact' or dtype == F32
    H, N = c['H'], c['N']
    kind = mutate[0] if mutate else None
    cv = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    h_in = cv(c['h_in'])
    rows, hrow, grow = _entries(c)
    ptr = c['ptr'].long()
    deg = (ptr[1:] - ptr[:-1]).to(dtype)
    ew = torch.ones(rows.numel(), dtype=dtype)
    if kind == 'drop_entry':                                # (node, position in its list; -1 = the last)
        node, pos = mutate[1], mutate[2]
        ew[int(ptr[node + 1]) - 1 if pos < 0 else int(ptr[node]) + pos] = 0
    if kind == 'tag_for_node':
        grow = hrow
    own = c['own_idx'].long() if c['own_idx'] is not None else torch.arange(N)
    if kind == 'own_identity':
        own = torch.arange(N).clamp(max=h_in.shape[0] - 1)
    if kind == 'no_deg_bc':
        deg = torch.zeros_like(deg)
    agg = torch.zeros(N, H, dtype=dtype).index_add_(0, rows, h_in[hrow] * ew[:, None]).requires_grad_(True)
    h_own = h_in[own].clone().requires_grad_(True)
    P = {k: cv(c[k]).clone().requires_grad_(True) for k in ('Wc', 'bc', 'Whh', 'bhh')}
    has_ln = c['ln_w'] is not None
    if has_ln:
        P['ln_w'], P['ln_b'] = (cv(c[k]).clone().requires_grad_(True) for k in ('ln_w', 'ln_b'))
    if c.get('xrow') is not None:
        P['xrow'] = cv(c['xrow']).clone().requires_grad_(True)
        xterm = P['xrow']
    else:
        P['xtab'] = cv(c['xtab']).clone().requires_grad_(True)
        xterm = P['xtab'][c['xcls'].long()]
    lin = _Lin3.apply if mm == 'x3' else (lambda x, W: x @ W.t())
    gi = lin(agg, P['Wc']) + deg[:, None] * P['bc'] + xterm
    gh = lin(h_own, P['Whh']) + P['bhh']
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    pre = (1 - z) * n + z * h_own
    mean = pre.mean(1)
    rstd = (pre.var(1, unbiased=False) + LN_EPS).rsqrt()
    m_used, r_used = mean, rstd
    if kind == 'stale_stats':                               # (row, the row whose statistics it reuses)
        sel = torch.arange(N)
        sel[mutate[1]] = mutate[2]
        m_used, r_used = mean[sel], rstd[sel]
    xhat = (pre - m_used[:, None]) * r_used[:, None]
    out = xhat * P['ln_w'] + P['ln_b'] if has_ln else pre
    dY = cv(c['gy_direct']).clone()
    if c['gy_agg'] is not None:
        dY.index_add_(0, rows, cv(c['gy_agg'])[grow] * ew[:, None])
    for t in (gi, gh, pre):
        t.retain_grad()
    out.backward(dY)
    res = {'h_out': out, 'mean': mean, 'rstd': rstd, 'g_direct': h_own.grad, 'g_agg': agg.grad, 'dWc': P['Wc'].grad, 'dbc': P['bc'].grad,
           'dWhh': P['Whh'].grad, 'dbhh': P['bhh'].grad}
    if 'xrow' in P:
        res['dxrow'] = P['xrow'].grad
    else:
        res['dxtab'] = P['xtab'].grad
    if has_ln:
        res['dln_w'], res['dln_b'] = P['ln_w'].grad, P['ln_b'].grad
    if kind == 'skip_tile_dbhh':                            # (tile): its rows' share never reaches the accumulator
        t0 = mutate[1] * TILE
        res['dbhh'] = res['dbhh'] - gh.grad[t0:t0 + TILE].sum(0)
    res = {k: v.detach().to(F64) for k, v in res.items()}
    if dtype == F64 and mutate is None:
        dGi, dGh, dpre = gi.grad.abs(), gh.grad.abs(), pre.grad.abs()
        aW, aWhh = P['Wc'].detach().abs(), P['Whh'].detach().abs()
        S = {'h_out': out.detach().abs().amax(1).clamp(min=1.0), 'mean': pre.detach().abs().amax(1).clamp(min=1.0), 'rstd': rstd.detach().clone(),
             'g_agg': (dGi @ aW).amax(1), 'g_direct': (dGh @ aWhh + dpre * z.detach()).amax(1),
             'dWc': dGi.t() @ agg.detach().abs(), 'dWhh': dGh.t() @ h_own.detach().abs(), 'dbc': (deg[:, None] * dGi).sum(0), 'dbhh': dGh.sum(0)}
        if 'xrow' in P:
            S['dxrow'] = dGi.amax(1)
        else:
            S['dxtab'] = torch.zeros(c['xtab'].shape, dtype=F64).index_add_(0, c['xcls'].long(), dGi)
        if has_ln:
            S['dln_w'], S['dln_b'] = (dY * xhat.detach()).abs().sum(0), dY.abs().sum(0)
        res['S'] = S
    return res


def ratio(got, ref, S):
    """max |got - ref| / S over a tensor: S per row ([N] against [N, *]) or per entry.  Where S is 0 the entry must be exactly the
    reference's (0): any difference there gives inf."""
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - ref).abs()
    if err.dim() == S.dim() + 1:
        err = err.amax(1)
    if err.numel() == 0:
        return 0.0
    q = torch.where(S > 0, err / S.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(q.max())


def ratios(got, ref):
    """{output: ratio} for every output of `got` (a dict of tensors) that the float64 result `ref` (with its scales) has."""
    return {k: ratio(v, ref[k], ref['S'][k]) for k, v in got.items() if k in ref['S']}


# ------------------------------------------------------------------------------------------------ launch geometry, restated
def grid_for(ntiles, per_cu=1):
    return min(max(ntiles, 1), GRID_CAP * per_cu)


def tile_seq(ntiles, grid, b):
    """Tiles workgroup b of `grid` visits (struct_stage_x3_common.h tile_seq with the XCD order on): contiguous eighths when the grid
    is a multiple of 8, round-robin otherwise."""
    if grid % 8 == 0:
        x, per, chunk = b & 7, grid >> 3, (ntiles + 7) >> 3
        first, end = x * chunk + (b >> 3), min((x + 1) * chunk, ntiles)
        return list(range(first, end, per)) if first < end else []
    return list(range(b, ntiles, grid))


def paths(c):
    """Which row path every tile of a case takes in the bf16x3 kernels, and why: {'total', 'full', 'chunked', 'reason'} per tile
    (reason: '' chunked, 'partial' last tile, 'cap' list total above CHUNK_CUT), the heavy rows (more than HEAVY_ROW entries) and
    the tiles they sit in."""
    N = c['N']
    ptr = c['ptr'].long().numpy()
    nt = (N + TILE - 1) // TILE
    out = []
    for t in range(nt):
        lo, hi = t * TILE, min(N, (t + 1) * TILE)
        total = int(ptr[hi] - ptr[lo])
        full = hi - lo == TILE
        reason = '' if full and total <= CHUNK_CUT else ('partial' if not full else 'cap')
        d = ptr[lo + 1:hi + 1] - ptr[lo:hi]
        out.append({'total': total, 'full': full, 'chunked': reason == '', 'reason': reason, 'dmax': int(d.max()), 'degs': d})
    deg = ptr[1:] - ptr[:-1]
    heavy = np.nonzero(deg > HEAVY_ROW)[0]
    return {'tiles': out, 'heavy': heavy, 'heavy_chunked': [int(n) for n in heavy if out[n // TILE]['chunked']],
            'heavy_generic': [int(n) for n in heavy if not out[n // TILE]['chunked']]}


# ------------------------------------------------------------------------------------------------ cases
def _tiles(k):
    return TILE * (k - 1) + 5         # k tiles: k - 1 full ones and a last tile of 5 rows


SIZES = {'n1': 1, 'n2': 2, 'n63': 63, 'n64': 64, 'n65': 65, 'n127': 127, 'n129': 129,
         't7': _tiles(7), 't8': _tiles(8), 't9': _tiles(9), 't16': _tiles(16), 't17': _tiles(17), 't20': _tiles(20),
         't256': _tiles(256), 't257': _tiles(257), 't300': _tiles(300), 't513': _tiles(513),
         'm260': TILE * 260}          # a multiple of 64 above the grid cap: no partial tile
HUB = 600                             # largest list of the float64 comparisons: a lost entry is >= 1/600 of its row's scale
LAST_ROW = 84                         # list of node N - 1 (heavy, inside the partial last tile where there is one)
ON_CHUNKED = 130                      # the listed heavy row inside a 504-entry (chunked) tile
LADDER = (64, 65, 127, 128, 129)      # heavy threshold; the pre-pass's 64-entry unroll and its tail


def degrees(N, lists):
    """List length per node, placed by tile.  'empty': none.  'small': 0..7 in every tile (the chunk widths D = 2, 3 and their
    multiples), tile 1 all zero.  'designed': on top of that, where the size has six full tiles: node 0 a HUB (tile 0 beyond the
    index-list capacity), tile 2 exactly 504 entries, tile 3 505, tile 4 504 with one ON_CHUNKED row, tile 5 the LADDER; smaller
    sizes put the hub and the ladder at the head.  Node N - 1 has LAST_ROW entries."""
    n = np.arange(N)
    if lists == 'empty':
        return np.zeros(N, dtype=np.int64)
    deg = (n * 5 + n // TILE) % 8
    full = N // TILE
    if full >= 2:
        deg[TILE:2 * TILE] = 0
    if lists == 'small':
        return deg
    assert lists == 'designed'
    if N == 1:
        deg[0] = 70
        return deg
    deg[0] = HUB
    if full >= 6:
        deg[2 * TILE:3 * TILE] = 7
        deg[2 * TILE:2 * TILE + 56] = 8                     # 448 + 56 = 504
        deg[3 * TILE:4 * TILE] = deg[2 * TILE:3 * TILE]
        deg[4 * TILE - 1] = 8                               # 505
        deg[4 * TILE:5 * TILE] = 5
        deg[4 * TILE:4 * TILE + 60] = 6                     # rows 0..59 without row 10: 59 rows at 6, 4 at 5, one of 130 = 504
        deg[4 * TILE + 10] = ON_CHUNKED
        deg[5 * TILE + 3:5 * TILE + 3 + len(LADDER)] = LADDER
    elif N >= 8:
        deg[1:1 + len(LADDER)] = LADDER
    deg[N - 1] = LAST_ROW
    return deg


def case(H, size, lists='designed', mode='plain', C=6, seed=0, ln=True, agg=True, rows=False):
    """Inputs of one half round as the C ABI takes them (float32 / int32 / uint8 CPU tensors) plus the builder's bookkeeping.
    mode: 'plain'; 'tagged' (h_in a 256-row table, entries node | row << 24, own rows through own_idx); 'own_few' / 'own_more'
    (untagged entries and own_idx into an h_in of fewer / more rows than N, as the quotient stages call it); 'n_rows' (h_in longer
    than the stage, no own index: the fp32 form).  rows=True: the general-feature form, xrow [N, 3H] instead of xcls / xtab.
    Values: standard normal rows (odd rows of h_in at 0.05: the long lists draw from those, so a 600-entry row's gates stay
    unsaturated and its outputs move with every entry), weights 0.15, bhh and xtab 0.1 / 0.3, bc 0.1 / 64 (it is multiplied by the
    list length), ln_w = 1 + 0.2 g; gy_direct = 1.7 (g + a per-column offset of +-0.6), gy_agg = 0.8 g."""
    N = SIZES[size] if isinstance(size, str) else int(size)
    g = np.random.Generator(np.random.PCG64([seed, H, N, {'empty': 0, 'small': 1, 'designed': 2}[lists]]))
    R = {'plain': N, 'tagged': 256, 'own_few': max(1, N // 3), 'own_more': N + 37, 'n_rows': N + 41}[mode]
    tagged = mode == 'tagged'
    deg = degrees(N, lists)
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=ptr[1:])
    E = int(ptr[-1])
    row = np.repeat(np.arange(N), deg)
    long_list = deg[row] > 16
    quiet = 2 * g.integers(0, max(R // 2, 1), E) + (1 if R >= 2 else 0)
    hrow = np.where(long_list, quiet, g.integers(0, R, E))
    first = ptr[:-1]
    rep = np.nonzero((deg >= 2) & (np.arange(N) % 7 == 3))[0]
    if tagged:
        node = g.integers(0, N, E)
        self_rows = np.nonzero((deg >= 1) & (np.arange(N) % 5 == 2))[0]
        node[first[self_rows]] = self_rows                  # self entries
        node[first[rep] + 1], hrow[first[rep] + 1] = node[first[rep]], hrow[first[rep]]     # repeated entries
        idx = (node | (hrow << 24)).astype(np.uint32).view(np.int32)
    else:
        self_rows = np.nonzero((deg >= 1) & (np.arange(N) % 5 == 2) & (np.arange(N) < R))[0]
        hrow[first[self_rows]] = self_rows
        hrow[first[rep] + 1] = hrow[first[rep]]
        idx = hrow.astype(np.int32)
    if E == 0:
        idx = np.zeros(1, dtype=np.int32)                   # a one-element dummy: the kernels get a valid pointer
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    h_in = f(R, H)
    h_in[(1 if R >= 2 else 0)::2] *= 0.05 * min(1.0, (max(R // 2, 1) / HUB) ** 0.5)      # (few quiet rows: a long list repeats them, its sum is coherent)
    absent = C - 2 if C > 1 else -1
    cls = g.integers(0, C, N)
    cls[cls == absent] = C - 1
    own_idx = None
    if mode in ('tagged', 'own_few', 'own_more'):
        own_idx = torch.from_numpy(g.integers(0, R, N).astype(np.int32))
    col = torch.from_numpy(np.where(g.integers(0, 2, H) > 0, 0.6, -0.6).astype(np.float32))
    c = {'H': H, 'N': N, 'R': R, 'C': C, 'size': size, 'lists': lists, 'mode': mode, 'tagged': tagged, 'absent': absent,
         'h_in': h_in, 'ptr': torch.from_numpy(ptr.astype(np.int32)), 'idx': torch.from_numpy(idx), 'E': E,
         'xcls': torch.from_numpy(cls.astype(np.uint8)), 'xtab': 0.1 * f(C, 3 * H) + 0.3 * f(C, 3 * H), 'Wc': 0.15 * f(3 * H, H), 'bc': 0.1 / 64 * f(3 * H),
         'Whh': 0.15 * f(3 * H, H), 'bhh': 0.1 * f(3 * H), 'ln_w': 1 + 0.2 * f(H), 'ln_b': 0.1 * f(H), 'own_idx': own_idx,
         'gy_direct': 1.7 * (f(N, H) + col), 'gy_agg': 0.8 * f(N if tagged else R, H), 'xrow': 0.3 * f(N, 3 * H) if rows else None}
    if not ln:
        c['ln_w'] = c['ln_b'] = None
    if not agg:
        c['gy_agg'] = None
    heavy = np.nonzero(deg > HEAVY_ROW)[0].astype(np.int32)
    c['heavy'] = (int(heavy.size), torch.from_numpy(heavy))
    return c


def csr(rows, cols, N):
    """CSR lists: node i's list holds cols[e] of every pair with rows[e] == i, in pair order (int32 ptr, idx)."""
    order = torch.argsort(rows, stable=True)
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    idx = cols[order].to(torch.int32)
    return ptr.to(torch.int32), idx if idx.numel() else torch.zeros(1, dtype=torch.int32)


def plain_case(h_in, ptr, idx, xcls, xtab, Wc, bc, Whh, bhh, ln_w, ln_b, gy_direct, gy_agg):
    """A case in plain mode from tensors of any float type (the pinning tests feed float64)."""
    N, H = h_in.shape
    return {'H': H, 'N': N, 'tagged': False, 'own_idx': None, 'xrow': None, 'h_in': h_in, 'ptr': ptr, 'idx': idx, 'xcls': xcls, 'xtab': xtab,
            'Wc': Wc, 'bc': bc, 'Whh': Whh, 'bhh': bhh, 'ln_w': ln_w, 'ln_b': ln_b, 'gy_direct': gy_direct, 'gy_agg': gy_agg}
