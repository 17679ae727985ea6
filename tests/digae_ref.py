"""Plain-torch restatement of the DiGAE baseline (DirectedGCNConv and the encoders built from it, DirectedGAE.recon_loss), test
infrastructure only: what the HIP path is held to, in whatever dtype the inputs have (the tests feed float64).  Written from the
layer's definition — a per-edge weight din(col)^-alpha * dout(row)^-beta on (W x_row + b), summed into col, one appended self loop
per node — and pinned to arrays recorded from the reference's own modules (tests/golden/g9_digae.npz, test_digae_spec.py)."""
import torch

EPS = 1e-15


def with_loops(ei, n, self_loops):
    if not self_loops:
        return ei
    loop = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei, torch.stack([loop, loop])], dim=1)


def _inv_pow(deg, a):
    out = torch.zeros_like(deg)
    nz = deg > 0
    out[nz] = deg[nz] ** (-a)
    return out


def scales(ei, n, alpha, beta, self_loops, dtype=torch.float64):
    """r[i] = din(i)^-alpha over col, c[j] = dout(j)^-beta over row (0 where the degree is 0)."""
    row, col = with_loops(ei, n, self_loops)
    din = torch.zeros(n, dtype=dtype).index_add_(0, col, torch.ones(col.shape[0], dtype=dtype))
    dout = torch.zeros(n, dtype=dtype).index_add_(0, row, torch.ones(row.shape[0], dtype=dtype))
    return _inv_pow(din, alpha), _inv_pow(dout, beta)


def propagate(y, ei, alpha, beta, self_loops, rc=None):
    """out[col] += r[col] c[row] y[row] per edge.  rc = (r, c) replaces the scales (somebody else's, widened: the per-entry tests
    price the sum apart from the scales' own rounding)."""
    n = y.shape[0]
    r, c = scales(ei, n, alpha, beta, self_loops, y.dtype) if rc is None else (rc[0].to(y.dtype), rc[1].to(y.dtype))
    row, col = with_loops(ei, n, self_loops)
    return torch.zeros_like(y).index_add_(0, col, (r[col] * c[row]).unsqueeze(1) * y[row])


def conv(x, W, b, ei, alpha=1.0, beta=0.0, self_loops=True):
    """The per-edge form: the Linear first, as the layer is written."""
    return propagate(x @ W.t() + b, ei, alpha, beta, self_loops)


def conv_factored(x, W, b, ei, alpha=1.0, beta=0.0, self_loops=True):
    """agg_i = r_i sum c_j x_j, rho_i = r_i sum c_j, out_i = W agg_i + rho_i b."""
    agg = propagate(x, ei, alpha, beta, self_loops)
    rho = propagate(torch.ones(x.shape[0], 1, dtype=x.dtype), ei, alpha, beta, self_loops)
    return agg @ W.t() + rho * b


def flip(ei):
    return torch.flip(ei, [0])


def encoder(p, pre, x_s, x_t, ei, alpha=1.0, beta=0.0, self_loops=True, relu_mask=None):
    """DirectedGCNConvEncoder: s = conv2(relu(conv1(x, ei)), flip(ei)), t = conv2(relu(conv1(x, flip(ei))), ei) with four Linear
    layers p[pre + 'source_conv.conv1.lin.weight'] ...  Returns (s, t, hidden_s, hidden_t).  relu_mask = (mask_s, mask_t) replaces
    the ReLU decisions (comparisons on somebody else's mask)."""
    def act(v, k):
        return torch.relu(v) if relu_mask is None else v * relu_mask[k].to(v.dtype)
    g = lambda half, layer: (p['%s%s_conv.%s.lin.weight' % (pre, half, layer)], p['%s%s_conv.%s.lin.bias' % (pre, half, layer)])
    a = (alpha, beta, self_loops)
    hs = act(conv(x_s, *g('source', 'conv1'), ei, *a), 0)
    s = conv(hs, *g('source', 'conv2'), flip(ei), *a)
    ht = act(conv(x_t, *g('target', 'conv1'), flip(ei), *a), 1)
    t = conv(ht, *g('target', 'conv2'), ei, *a)
    return s, t, hs, ht


def single_layer_encoder(p, pre, s0, t0, ei, alpha=1.0, beta=0.0, self_loops=True):
    """SingleLayerDirectedGCNConvEncoder with its cross wiring: s_1 = source_conv(t_0) over flip(ei), t_1 = target_conv(s_0) over ei."""
    a = (alpha, beta, self_loops)
    s1 = conv(t0, p[pre + 'source_conv.conv.lin.weight'], p[pre + 'source_conv.conv.lin.bias'], flip(ei), *a)
    t1 = conv(s0, p[pre + 'target_conv.conv.lin.weight'], p[pre + 'target_conv.conv.lin.bias'], ei, *a)
    return s1, t1


def recon_loss(s, t, pos, neg):
    """(loss, pred_bin) of DirectedGAE.recon_loss with the negatives given."""
    pp = torch.sigmoid((s[pos[0]] * t[pos[1]]).sum(1))
    pn = torch.sigmoid((s[neg[0]] * t[neg[1]]).sum(1))
    loss = -torch.log(pp + EPS).mean() - torch.log(1 - pn + EPS).mean()
    return loss, (torch.cat([pp, pn]) > 0.5).int()


# ------------------------------------------------------------------------------------------------
# The entries of csrc/digcn_conv.hip one output entry at a time: designed lists and operands, float64 references from exactly the
# ABI's arguments with a bound per entry derived from float32 rounding, the same sums in float32 in another order, and restatements
# that each make one mistake (tests/test_digae_spec.py pins all of it without a GPU; tests/test_hip_digae_entries.py runs the device).
# ------------------------------------------------------------------------------------------------
import numpy as np  # noqa: E402

U24 = 2.0 ** -24                 # u: half an ulp of float32, the relative error of one rounding
HEAVY = 64                       # lists longer than this take one workgroup each (kDigcnHeavy, GraphPlan.HEAVY_ROW)
CLASSES = 8                      # rows of the class table (kDigcnClasses)
SUBNORMAL = 2.0 ** -140          # a positive float32 subnormal: counts as > 0
LAST_IN, LAST_OUT = 7, 65        # list lengths of node n - 1 (the last row of the last workgroup): one trip and a tail; heavy
SETTINGS = [(1.0, 0.0, True), (0.5, 0.5, True), (0.0, 1.0, True), (1.0, 0.0, False), (1.0, 1.0, False)]       # (alpha, beta, self loops)


def lane_groups(H):
    """G: the lane groups of k_digcn_gather_heavy (256 threads, H/4 lanes per row)."""
    return 256 // (H // 4)


def pass_rows(H, entry):
    """Rows one grid pass covers: 256 / (H/4) rows per workgroup, at most 256 * 16 workgroups (gather, class_fwd) or 256 * 4 (class_bwd)."""
    return lane_groups(H) * 256 * (4 if entry == 'class_bwd' else 16)


def planted_lengths(H):
    """An empty list, the tail alone, one and two unrolled trips with and without a tail, both sides of the heavy boundary, heavy lists
    of fewer entries than lane groups beyond the boundary, an exact multiple and a remainder, and long ones."""
    G = lane_groups(H)
    return [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 66, 64 + G - 1, 64 + G, 64 + G + 1, 64 + 2 * G + 1, 129, 200, 300]


def planted(H, n=400, first=0, out_first=None, lengths=None):
    """({node: in-list length}, {node: out-list length}) that designed_lists plants: the lengths on `first`.. in the in-CSR, the same
    lengths in reverse order on `out_first`.. (by default the nodes behind the first set) in the out-CSR, and node n - 1 in both."""
    L = planted_lengths(H) if lengths is None else list(lengths)
    out_first = first + len(L) + 1 if out_first is None else out_first
    a = {first + k: v for k, v in enumerate(L)}
    b = {out_first + k: v for k, v in enumerate(reversed(L))}
    assert n % 64 != 0 and max(a) < n - 1 and max(b) < n - 1
    a[n - 1], b[n - 1] = LAST_IN, LAST_OUT
    return a, b


def designed_lists(H, n=400, first=0, out_first=None, lengths=None, seed=0):
    """edge_index [2, E] of a directed multigraph (duplicates and self edges allowed) whose in-lists and out-lists have the lengths
    `planted` names; every other in-list has 0 to 3 entries, every other out-list whatever is left over (far below HEAVY).  The two
    degree sequences are paired stub by stub at random, and the edges are shuffled."""
    rng = np.random.default_rng([seed, H, n, first])
    a, b = planted(H, n, first, out_first, lengths)
    din = rng.integers(0, 4, n)
    din[list(a)] = list(a.values())
    dout = np.zeros(n, dtype=np.int64)
    dout[list(b)] = list(b.values())
    left = int(din.sum() - dout.sum())
    assert left >= 0
    free = np.setdiff1d(np.arange(n), np.array(list(b)))
    dout += np.bincount(rng.choice(free, left), minlength=n)
    src, dst = np.repeat(np.arange(n), dout), np.repeat(np.arange(n), din)
    rng.shuffle(src)
    p, q = int(np.nonzero(dst == n - 1)[0][0]), int(np.nonzero(src == n - 1)[0][0])
    src[p], src[q] = src[q], src[p]              # one self edge for certain, on node n - 1 (degrees unchanged)
    order = rng.permutation(src.shape[0])
    return torch.from_numpy(np.stack([src[order], dst[order]]).astype(np.int64))


def many_heavy_lists(n=4100, seed=0):
    """Every in-list has 65 to 70 entries: more heavy nodes than the heavy kernel has workgroups (4,096)."""
    rng = np.random.default_rng([seed, n])
    dst = np.repeat(np.arange(n), rng.integers(65, 71, n))
    src = rng.integers(0, n, dst.shape[0])
    order = rng.permutation(dst.shape[0])
    return torch.from_numpy(np.stack([src[order], dst[order]]).astype(np.int64))


def csr_of(ei, n, reverse):
    """(ptr, idx) int64 of the lists a node sums over, as GraphPlan.csr(reverse) holds them (stable order)."""
    src, dst = (ei[1], ei[0]) if reverse else (ei[0], ei[1])
    perm = torch.sort(dst, stable=True).indices
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return ptr, src[perm].contiguous()


def signed(rng, *shape):
    """float32, magnitudes in [0.5, 2], random signs: no term is small beside its neighbours, so a lost one shows."""
    return torch.from_numpy((rng.uniform(0.5, 2.0, shape) * (rng.integers(0, 2, shape) * 2 - 1)).astype(np.float32))


def positive(rng, n):
    """float32 in [0.25, 4]: scales that are not the degrees' own."""
    return torch.from_numpy(rng.uniform(0.25, 4.0, n).astype(np.float32))


def designed_mask(rng, n, H, special_rows):
    """float32 [n, H] of negative values, +0.0, -0.0 and positive normals at random, and in every column one positive subnormal, on
    a row out of `special_rows` (nodes that sit in many lists).  The decision expected of it is float64 > 0."""
    kind = rng.integers(0, 4, (n, H))
    val = rng.uniform(0.5, 2.0, (n, H)).astype(np.float32)
    m = np.where(kind == 0, -val, np.where(kind == 1, np.float32(0.0), np.where(kind == 2, np.float32(-0.0), val))).astype(np.float32)
    rows = np.asarray(list(special_rows))
    for k in range(H):
        m[rows[k % len(rows)], k] = SUBNORMAL
    return torch.from_numpy(m)


def special_rows(H, n=400, first=0, out_first=None, lengths=None):
    """Nodes with planted lists of at least 8 entries, the two sets alternating: each sits in many lists of the opposite CSR."""
    a, b = planted(H, n, first, out_first, lengths)
    a, b = [v for v, l in a.items() if l >= 8], [v for v, l in b.items() if l >= 8]
    return [v for pair in zip(b, a) for v in pair]


def designed_classes(rng, n, C):
    """uint8 [n] class ids: every id below C occurs, except C - 2 when 2 <= C < 8 (a table row no term reaches)."""
    ids = np.array([k for k in range(C) if not (2 <= C < CLASSES and k == C - 2)])
    cls = ids[rng.integers(0, len(ids), n)]
    cls[rng.permutation(n)[:len(ids)]] = ids
    return torch.from_numpy(cls.astype(np.uint8))


def _list_sum(P, ptr, idx, wt=None, selfw=None):
    """row i: sum over the slots e of list i of wt[e] P[idx[e]], plus selfw[i] P[i]."""
    n, W = P.shape
    rows = torch.repeat_interleave(torch.arange(n), ptr[1:] - ptr[:-1])
    cols = []
    for k0 in range(0, W, 32):
        t = P[:, k0:k0 + 32][idx]
        if wt is not None:
            t = t * wt[:, None]
        cols.append(torch.zeros(n, t.shape[1], dtype=P.dtype).index_add_(0, rows, t))
    out = torch.cat(cols, 1)
    return out if selfw is None else out + selfw[:, None].to(P.dtype) * P


def _class_rows(a, mut, wt, selfw):
    """W[i][k] = sum of inner[j] over the entries of list i (and i itself) whose class is k."""
    n = a['ptr'].shape[0] - 1
    one = torch.zeros(n, CLASSES, dtype=torch.float64)
    one[torch.arange(n), a['cls'].long()] = a['inner'].double()
    true = _list_sum(one, a['ptr'], a['idx'], None, torch.ones(n) if a['loops'] else None)
    if mut.get('skip_class') is not None:
        one[:, mut['skip_class']] = 0
    return _list_sum(one, a['ptr'], a['idx'], wt, selfw), true


def reference(entry, a, **mut):
    """float64 restatement of mgv_digcn_gather / _class_fwd / _class_bwd from the ABI's arguments (CPU tensors; `ptr`, `idx` int64; float32
    operands widened) -> {'ref', 'S', 'bound'} per output entry, u = 2^-24, terms = list length (+ 1 with self loops):
      gather     S = |outer_i| sum |inner_j| [mask_jk > 0] |y_jk|        bound (terms + 4) u S         (a rounding per product, terms - 1
                 inexact additions in any order, one for the outer scale, two to spare; the ReLU is exact)
      class_fwd  S = |outer_i| sum_j |inner_j| |T[cls_j, k]|             bound (terms + 8 + 4) u S     (the class sums, then eight multiply-adds)
      class_bwd  S[c,k] = sum_i w_i[c] |outer_i| [z_ik > 0] |dz_ik|      bound (nz + Lmax + 8) u S + 2 u |a0|    (nz: nodes with a nonzero
                 term for the entry — adding a zero partial is exact, whatever the tree; Lmax: the longest list; a0: dT before the call)
    `mut` plants one mistake (defects()); S and bound are always the correct run's."""
    ptr, idx = a['ptr'], a['idx']
    n = ptr.shape[0] - 1
    lens = ptr[1:] - ptr[:-1]
    loops = bool(a['loops'])
    outer, inner = a['outer'].double(), a['inner'].double()
    if mut.get('swap'):
        outer, inner = inner, outer
    wt = mut['wt'](a, lens) if 'wt' in mut else None
    ones = torch.ones(n, dtype=torch.float64)
    selfw = (mut['selfw'](a, lens).double() if 'selfw' in mut else ones) if loops else None
    terms = (lens + int(loops)).double()[:, None]
    if entry == 'class_bwd':
        W, Wtrue = _class_rows(a, mut, wt, selfw)
        C = a['C']
        z = None if a['z'] is None else (a['z'].double() > 0).double()
        d = a['dz'].double() * a['outer'].double()[:, None]
        dtrue = d if z is None else d * z
        if mut.get('no_outer'):
            d = a['dz'].double()
        if z is not None and not mut.get('no_z'):
            d = d * z
        if 'skip_rows' in mut:
            W = W.clone()
            W[mut['skip_rows'](a):] = 0
        a0 = a['a0'].double()
        ref = W[:, :C].t() @ d + (0 if mut.get('overwrite') else a0)
        S = Wtrue[:, :C].t() @ dtrue.abs()
        nz = (Wtrue[:, :C] != 0).double().t() @ (dtrue != 0).double()
        bound = (nz + float(lens.max()) + 8) * U24 * S + 2 * U24 * a0.abs()
        return {'ref': ref, 'S': S, 'bound': bound}
    if entry == 'class_fwd':
        W, Wtrue = _class_rows(a, mut, wt, selfw)
        T = torch.zeros(CLASSES, a['T'].shape[1], dtype=torch.float64)
        T[:a['C']] = a['T'].double()
        s, Sabs, spare = W @ T, Wtrue @ T.abs(), 12
    else:
        P = inner[:, None] * a['y'].double()
        Ptrue = a['inner'].double()[:, None] * a['y'].double()
        m = None
        if a['mask'] is not None:
            mk = a['mask'].double()
            m = ((mk >= 0) if mut.get('mask_ge') else (mk > 0)).double()
            Ptrue = Ptrue * (mk > 0).double()
            if not mut.get('mask_row_i'):
                P = P * m
        s = _list_sum(P, ptr, idx, wt, selfw)
        if m is not None and mut.get('mask_row_i'):
            s = s * m
        Sabs, spare = _list_sum(Ptrue.abs(), ptr, idx, None, ones if loops else None), 4
    ref = outer[:, None] * s
    S = a['outer'].double().abs()[:, None] * Sabs
    if a['relu']:
        ref = ref.clamp_min(0)
    if 'unwritten' in mut:
        ref[mut['unwritten'](a, lens)] = float('nan')
    if 'skip_rows' in mut:
        ref[mut['skip_rows'](a):] = float('nan')
    return {'ref': ref, 'S': S, 'bound': (terms + spare) * U24 * S}


def share(got, r):
    """max |got - ref| / bound over the entries; inf for a NaN, or where a zero bound is missed (such an entry must equal its reference: 0
    for the row outputs, a0 bit for bit for dT)."""
    e = (got.double() - r['ref']).abs()
    e = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)
    q = torch.where(r['bound'] > 0, e / r['bound'].clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float('inf')), torch.zeros_like(e)))
    return float(q.max()) if q.numel() else 0.0


def _list_sum32(P, ptr, idx, loops, G, heavy):
    """The list sums in float32 in ANOTHER order than the kernels': a list from its last entry to its first and the node's own term
    last (the kernels start from it); with `heavy`, a list above HEAVY as G strided partials that meet from the last group to the first."""
    n = P.shape[0]
    lens = ptr[1:] - ptr[:-1]
    acc = torch.zeros_like(P)
    hv = (lens > HEAVY) if heavy else torch.zeros(n, dtype=torch.bool)
    for p in range(int(lens[~hv].max()) if bool((~hv).any()) else 0):
        sel = torch.nonzero(~hv & (lens > p)).reshape(-1)
        acc[sel] = acc[sel] + P[idx[ptr[sel] + lens[sel] - 1 - p]]
    hn = torch.nonzero(hv).reshape(-1)
    if hn.numel():
        parts = torch.zeros(hn.numel(), G, P.shape[1], dtype=P.dtype)
        for p in range(int(lens[hn].max())):
            s = torch.nonzero(lens[hn] > p).reshape(-1)
            parts[s, p % G] = parts[s, p % G] + P[idx[ptr[hn[s]] + p]]
        tot = torch.zeros(hn.numel(), P.shape[1], dtype=P.dtype)
        for g in reversed(range(G)):
            tot = tot + parts[:, g]
        acc[hn] = tot
    return acc + P if loops else acc


def restate32(entry, a, heavy=True):
    """The three entries in float32 arithmetic, summed in another order than the device's (see _list_sum32; the class sums from class 7
    down, dT over the nodes from the last to the first): what any correct float32 evaluation must keep inside `reference`'s bounds."""
    f32 = torch.float32
    ptr, idx, loops, G = a['ptr'], a['idx'], bool(a['loops']), lane_groups(a['H'])
    n = ptr.shape[0] - 1
    if entry == 'gather':
        P = a['inner'][:, None] * a['y']
        if a['mask'] is not None:
            P = torch.where(a['mask'] > 0, P, torch.zeros_like(P))
        out = a['outer'][:, None] * _list_sum32(P, ptr, idx, loops, G, heavy)
        return out.clamp_min(0) if a['relu'] else out
    one = torch.zeros(n, CLASSES, dtype=f32)
    one[torch.arange(n), a['cls'].long()] = a['inner']
    W = _list_sum32(one, ptr, idx, loops, G, False)
    C = a['C']
    if entry == 'class_fwd':
        acc = torch.zeros(n, a['T'].shape[1], dtype=f32)
        for k in reversed(range(C)):
            acc = acc + W[:, k:k + 1] * a['T'][k][None, :]
        out = a['outer'][:, None] * acc
        return out.clamp_min(0) if a['relu'] else out
    d = a['outer'][:, None] * a['dz']
    if a['z'] is not None:
        d = torch.where(a['z'] > 0, d, torch.zeros_like(d))
    part = torch.zeros(C, d.shape[1], dtype=f32)
    for i in reversed(torch.nonzero((d != 0).any(1)).reshape(-1).tolist()):
        part = part + W[i, :C, None] * d[i][None, :]
    return a['a0'] + part


def _slot_pos(a, lens):
    rows = torch.repeat_interleave(torch.arange(lens.shape[0]), lens)
    return rows, torch.arange(rows.shape[0]) - a['ptr'][rows]


def defects():
    """name -> f(entry, a) with `reference`'s signature and result, making one mistake; f.entries: the entries it concerns, f.applies(entry, a):
    whether the case can show it (self loops on for the self-term mistakes, a mask given, C = 8, a second grid pass, ...)."""
    def light(a, lens, keep_not):
        rows, pos = _slot_pos(a, lens)
        return (~((lens[rows] <= HEAVY) & keep_not(lens[rows], pos))).double()

    def group(a, lens, g):
        rows, pos = _slot_pos(a, lens)
        G = lane_groups(a['H'])
        return (~((lens[rows] > HEAVY) & (pos % G == (g if g >= 0 else G + g)))).double()

    every = lambda entry, a: True
    looped = lambda entry, a: bool(a['loops'])
    looped_heavy = lambda entry, a: bool(a['loops']) and int((a['ptr'][1:] - a['ptr'][:-1]).max()) > HEAVY
    masked = lambda entry, a: a['mask'] is not None
    table = {
        'the tail entry dropped when length % 4 != 0': (('gather',), every, dict(wt=lambda a, l: light(a, l, lambda n, p: (n % 4 != 0) & (p == n - 1)))),
        'the fourth entry of an unrolled trip dropped': (('gather',), every, dict(wt=lambda a, l: light(a, l, lambda n, p: (p % 4 == 3) & (p < 4 * (n // 4))))),
        'the self term omitted': (('gather', 'class_fwd', 'class_bwd'), looped, dict(selfw=lambda a, l: torch.zeros(l.shape[0]))),
        'the self term doubled': (('gather', 'class_fwd', 'class_bwd'), looped, dict(selfw=lambda a, l: torch.full((l.shape[0],), 2.0))),
        'heavy: the partial of lane group 0 dropped': (('gather',), every, dict(wt=lambda a, l: group(a, l, 0))),
        'heavy: the partial of lane group G-1 dropped': (('gather',), every, dict(wt=lambda a, l: group(a, l, -1))),
        'heavy: the self term added once per group': (('gather',), looped_heavy, dict(selfw=lambda a, l: torch.where(l > HEAVY, float(lane_groups(a['H'])), 1.0))),
        'a list of 65 left unwritten': (('gather',), lambda entry, a: bool(((a['ptr'][1:] - a['ptr'][:-1]) == 65).any()), dict(unwritten=lambda a, l: l == 65)),
        'mask read at row i instead of j': (('gather',), masked, dict(mask_row_i=True)),
        'mask with >=': (('gather',), masked, dict(mask_ge=True)),
        'outer and inner exchanged': (('gather',), every, dict(swap=True)),
        'class id 7 ignored': (('class_fwd', 'class_bwd'), lambda entry, a: a['C'] == CLASSES, dict(skip_class=7)),
        'class_bwd overwriting instead of adding': (('class_bwd',), every, dict(overwrite=True)),
        'class_bwd ignoring z': (('class_bwd',), lambda entry, a: a['z'] is not None, dict(no_z=True)),
        'class_bwd without outer': (('class_bwd',), lambda entry, a: bool((a['outer'] != 1).any()), dict(no_outer=True)),      # (alpha = 0: outer is 1)
        'the rows of a second grid pass skipped': (('gather', 'class_fwd', 'class_bwd'), lambda entry, a: a['ptr'].shape[0] - 1 > pass_rows(a['H'], entry),
                                                   dict(skip_rows=lambda a: pass_rows(a['H'], a['entry']))),
    }
    out = {}
    for name, (entries, applies, mut) in table.items():
        def f(entry, a, mut=mut):
            return reference(entry, dict(a, entry=entry), **mut)
        f.entries, f.applies = entries, applies
        out[name] = f
    return out


def gather_case(H, ei, n, reverse, loops, relu, masked, form, seed, rc=None, special=None):
    """The ABI's arguments of one gather case on the lists of `ei` (CPU tensors): form 'random' takes independent scales in [0.25, 4];
    any other form takes rc = (outer, inner) as given (the float32 scales of the graph: the device's own, or scales() rounded)."""
    rng = np.random.default_rng([seed, H, n, int(reverse)])
    ptr, idx = csr_of(ei, n, reverse)
    y, o, i = signed(rng, n, H), positive(rng, n), positive(rng, n)
    mask = designed_mask(rng, n, H, special if special is not None else special_rows(H, n))
    outer, inner = (o, i) if form == 'random' else (rc[0].float().cpu(), rc[1].float().cpu())
    return dict(H=H, ptr=ptr, idx=idx, y=y, outer=outer, inner=inner, mask=mask if masked else None, loops=loops, relu=relu)


def class_case(H, ei, n, reverse, loops, relu, masked, C, seed, rc=None, special=None, dz_rows=None):
    """The arguments of mgv_digcn_class_fwd and _bwd on the lists of `ei`: T and dz of magnitudes in [0.5, 2], z the designed mask
    (or None), dz zero outside `dz_rows` where those are given, a0 random (below)."""
    rng = np.random.default_rng([seed, H, n, int(reverse), C])
    ptr, idx = csr_of(ei, n, reverse)
    cls, T, dz, a0 = designed_classes(rng, n, C), signed(rng, C, H), signed(rng, n, H), signed(rng, C, H)
    o, i = positive(rng, n), positive(rng, n)
    z = designed_mask(rng, n, H, special if special is not None else special_rows(H, n))
    if dz_rows is not None:
        keep = torch.zeros(n, dtype=torch.bool)
        keep[torch.as_tensor(dz_rows)] = True
        dz = dz * keep[:, None]
    outer, inner = (o, i) if rc is None else (rc[0].float().cpu(), rc[1].float().cpu())
    a = dict(H=H, ptr=ptr, idx=idx, cls=cls, T=T, C=C, outer=outer, inner=inner, loops=loops, relu=relu, z=z if masked else None, dz=dz, a0=a0)
    # a0 of each entry's own magnitude (S times a uniform in [-1, 1]): S runs from 1e-2 to 1e4 with the setting, and an a0 of order 1
    # beside a small S would make the final += the thing measured; where nothing contributes (S = 0) a0 keeps a magnitude in [0.5, 2]
    S = reference('class_bwd', a)['S']
    a['a0'] = torch.where(S > 0, S * torch.from_numpy(rng.uniform(-1.0, 1.0, (C, H))), a0.double()).float()
    return a
