"""A numpy restatement of mgv_fanin_decode and mgv_fanin_recovery from exactly the ABI's arguments, and the seeded case builders of
tests/test_fanin_decode_spec.py (CPU, which pins all of this) and tests/test_hip_fanin_decode.py (the device against it).

Decode.  `scores` is the dense matrix with the TARGETS as rows: scores[v][u] = <s_u, t_v> (on the device: mgv_pair_scores_fwd with the
operands swapped, sigmoid = 0).  Row v keeps kk = min(max(want[v], 0), K) fan-ins.  A candidate of v is a column u of v's graph with
key[u] < key[v] whose score is not NaN; a row with kk = 0 has none.  The kept ones are the first kk candidates in the order (score
descending, id ascending); idx is -1 and score -inf past the end; n_cand counts the candidates regardless of score.

Recovery.  Plain Python sets: the decoded set of a row is the set of its idx entries other than -1, the true set the set of the sources
of the edges that end in it.  Over the rows with a non-empty true set, per graph: {gates, exact, hits, true_total, decoded_total}."""
import numpy as np
import torch

K_MAX = 8
SIZES = (1, 5, 58, 64, 1, 71)          # borders inside a row tile (1, 6, 129) and on a tile edge (64, 128); N = 200
DEFECTS = ('le', 'tie', 'want', 'graph', 'self')
NEG_INF = np.float32(-np.inf)


def graph_of(N, graph_ptr):
    """int64 [N]: the graph of every node (0 everywhere without a table)."""
    if graph_ptr is None:
        return np.zeros(N, dtype=np.int64)
    gp = np.asarray(graph_ptr, dtype=np.int64)
    return np.searchsorted(gp[1:], np.arange(N), side='right')


def kept(want, K):
    return np.clip(np.asarray(want, dtype=np.int64), 0, K)


def candidate_mask(scores, key, want, K, graph_ptr=None, defect=None):
    """bool [N, N], [v][u]: u is a candidate of target v."""
    N = scores.shape[0]
    key = np.asarray(key, dtype=np.int64)
    g = graph_of(N, graph_ptr)
    below = key[None, :] <= key[:, None] if defect == 'le' else key[None, :] < key[:, None]
    if defect == 'self':
        below = below | np.eye(N, dtype=bool)
    same = np.ones((N, N), dtype=bool) if defect == 'graph' else g[None, :] == g[:, None]
    kk = np.full(N, K) if defect == 'want' else kept(want, K)
    return below & same & ~np.isnan(scores) & (kk > 0)[:, None]


def decode_ref(scores, key, want, K, graph_ptr=None, defect=None):
    """(idx int32 [N, K], score float32 [N, K], n_cand int32 [N]); defect: one of DEFECTS planted, for the spec file."""
    scores = np.asarray(scores, dtype=np.float32)
    N = scores.shape[0]
    mask = candidate_mask(scores, key, want, K, graph_ptr, defect)
    kk = np.full(N, K) if defect == 'want' else kept(want, K)
    ids = np.broadcast_to(np.arange(N), (N, N))
    with np.errstate(invalid='ignore'):
        neg = np.where(mask, -scores, np.float32(0))
    order = np.lexsort((-ids if defect == 'tie' else ids, neg, ~mask), axis=-1)       # candidates first, by (score desc, id asc)
    n_cand = mask.sum(1).astype(np.int32)
    idx = np.full((N, K), -1, dtype=np.int32)
    out = np.full((N, K), NEG_INF, dtype=np.float32)
    for j in range(K):
        if j >= N:
            break
        take = j < np.minimum(kk, n_cand)
        col = order[:, j]
        idx[take, j] = col[take]
        out[take, j] = scores[np.arange(N), col][take]
    return idx, out, n_cand


def decode_loops(scores, key, want, K, graph_ptr=None):
    """The same by brute force: one Python loop per pair."""
    N = len(key)
    g = graph_of(N, graph_ptr)
    idx = np.full((N, K), -1, dtype=np.int32)
    out = np.full((N, K), NEG_INF, dtype=np.float32)
    n_cand = np.zeros(N, dtype=np.int32)
    for v in range(N):
        kk = min(max(int(want[v]), 0), K)
        if kk == 0:
            continue
        cand = []
        for u in range(N):
            x = scores[v][u]
            if g[u] == g[v] and int(key[u]) < int(key[v]) and x == x:
                cand.append((-float(x), u))
        cand.sort()
        n_cand[v] = len(cand)
        for j, (negx, u) in enumerate(cand[:kk]):
            idx[v, j] = u
            out[v, j] = scores[v][u]
    return idx, out, n_cand


def same_decode(a, b):
    """idx and n_cand as integers, score bit for bit."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            and np.array_equal(np.asarray(a[1], dtype=np.float32).view(np.int32), np.asarray(b[1], dtype=np.float32).view(np.int32)))


# ------------------------------------------------------------------------------------------------ keys, wants, cases
KEY_MODES = ('asc', 'desc', 'levels', 'equal')


def make_key(mode, N, graph_ptr, rng):
    g = graph_of(N, graph_ptr)
    first = np.zeros(N, dtype=np.int64) if graph_ptr is None else np.asarray(graph_ptr, dtype=np.int64)[g]
    local = np.arange(N) - first
    if mode == 'asc':
        return local.astype(np.int32)
    if mode == 'desc':
        return (-local).astype(np.int32)
    if mode == 'levels':
        return rng.integers(0, 6, size=N).astype(np.int32)         # levels 0 .. 5: many equal keys
    if mode == 'equal':
        return np.full(N, 3, dtype=np.int32)
    raise ValueError(mode)


def decode_case(H, N=None, sizes=None, keys='asc', K=3, seed=1):
    """One seeded case: s, t float32 [N, H] (torch), key, want int32 [N] (numpy), graph_ptr (list or None), K, and `info`, the rows the
    builder planted (where the case is large enough to hold them: N >= 64):
      twin      (u, u2): column rows s[u] == s[u2], so every target scores them equally: ties that go by id;
      nan_col   a column row of NaNs: never a candidate;
      nan_row   a target row of NaNs: an empty list, n_cand = 0, although it wants something;
      neg, big  rows whose want is negative / above K: clamped to 0 / K;
    `want` is otherwise mixed over 0 .. K, so rows early in the key order want more than they have candidates."""
    rng = np.random.Generator(np.random.PCG64(1000 * seed + 17 * H + (N or 0) + 3 * K))
    gp = None
    if sizes is not None:
        gp = [0]
        for n in sizes:
            gp.append(gp[-1] + n)
        N = gp[-1]
    s = rng.standard_normal((N, H)).astype(np.float32)
    t = rng.standard_normal((N, H)).astype(np.float32)
    key = make_key(keys, N, gp, rng)
    want = rng.integers(0, K + 1, size=N).astype(np.int32)
    info = {}
    if N >= 64:
        base = 0 if gp is None else gp[-2]               # inside the last graph (71 nodes of SIZES) or the single graph
        span = N - base
        u, u2 = base + 2, base + 9
        s[u2] = s[u]
        info['twin'] = (u, u2)
        info['nan_col'] = base + 5
        s[base + 5] = np.nan
        info['nan_row'] = base + span - 4
        t[base + span - 4] = np.nan
        want[base + span - 4] = K
        info['neg'], info['big'] = base + span - 2, base + span - 1
        want[base + span - 2] = -3
        want[base + span - 1] = K + 5
        # targets behind the twins score them equally whatever their own row holds; make them want at least one where K allows
        want[base + span - 6] = K
    return dict(H=H, N=N, K=K, s=torch.from_numpy(s), t=torch.from_numpy(t), key=key, want=want, graph_ptr=gp, info=info, keys=keys)


def long_case(H):
    """64 * 40 + 3 nodes in one graph, keys ascending with the id, the rows of tile 7 want nothing: with tile_min most column tiles are
    skipped, the prefetch loop runs over many tiles, and one row tile walks nothing."""
    c = decode_case(H=H, N=64 * 40 + 3, keys='asc', K=3, seed=2)
    c['want'][7 * 64:8 * 64] = 0
    return c


def dense_f32(case):
    """scores[v][u] in float32 on the CPU (any arithmetic serves the spec file: both sides read the same matrix)."""
    return (case['t'] @ case['s'].T).numpy()


# the designed cases of both test files: (name, kwargs of decode_case)
def designed_cases(H):
    out = []
    for N in (1, 2, 63, 64, 65, 129, 200):
        out.append(('N=%d one graph asc K=3' % N, dict(H=H, N=N, keys='asc', K=3)))
    for keys in KEY_MODES:
        for K in (1, 2, 3, 8):
            if keys in ('desc', 'equal') and K in (2, 8):
                continue
            out.append(('graphs %s K=%d' % (keys, K), dict(H=H, sizes=SIZES, keys=keys, K=K)))
            out.append(('N=200 one graph %s K=%d' % (keys, K), dict(H=H, N=200, keys=keys, K=K)))
    return out


# ------------------------------------------------------------------------------------------------ the orthonormal design
def ortho_case(H, seed=1):
    """A batch of graphs of H nodes each.  The column rows of a graph are an orthonormal basis (QR in float64, stored as float32); row v
    of t is the sum of the basis rows of v's true fan-ins.  A true fan-in then scores 1 and every other node of the graph 0 to within
    float32 rounding (|error| <= (H + 3) 2^-24 (1 + deg) by the usual dot-product bound: far below 1/2).  The graphs are levelised: H // 4
    inputs at level 0, the rest in levels of H // 8 + 1 nodes; a gate has 1 .. 3 distinct fan-ins, the first from the level below, the others
    from any lower level.  key = level, want = true in-degree."""
    rng = np.random.Generator(np.random.PCG64(77 * seed + H))
    graphs = max(3, 160 // H + 1)
    N = graphs * H
    s = np.zeros((N, H), dtype=np.float32)
    t = np.zeros((N, H), dtype=np.float32)
    level = np.zeros(N, dtype=np.int32)
    src, dst = [], []
    P, per = H // 4, H // 8 + 1
    for g in range(graphs):
        base = g * H
        q, _ = np.linalg.qr(rng.standard_normal((H, H)))
        s[base:base + H] = q.astype(np.float32)
        lv = np.zeros(H, dtype=np.int64)
        for i in range(P, H):
            lv[i] = 1 + (i - P) // per
        level[base:base + H] = lv
        for i in range(P, H):
            prev = np.nonzero(lv == lv[i] - 1)[0]
            lower = np.nonzero(lv < lv[i])[0]
            fins = {int(rng.choice(prev))}
            deg = int(rng.integers(1, 4))
            while len(fins) < min(deg, len(lower)):
                fins.add(int(rng.choice(lower)))
            t[base + i] = q[sorted(fins)].sum(0).astype(np.float32)
            for u in sorted(fins):
                src.append(base + u)
                dst.append(base + i)
    edge_index = np.array([src, dst], dtype=np.int64)
    want = np.bincount(edge_index[1], minlength=N).astype(np.int32)
    return dict(H=H, N=N, K=3, s=torch.from_numpy(s), t=torch.from_numpy(t), key=level, want=want,
                graph_ptr=[g * H for g in range(graphs + 1)], edge_index=edge_index)


# ------------------------------------------------------------------------------------------------ recovery
RECORD = ('gates', 'exact', 'hits', 'true_total', 'decoded_total')


def recovery_ref(idx, edge_index, graph_ptr=None):
    """(n_hit int32 [N], rec int64 [max(G, 1), 5]) with Python sets; a row behind the last graph of a table counts nowhere."""
    idx = np.asarray(idx)
    N = idx.shape[0]
    true = [set() for _ in range(N)]
    for u, v in zip(np.asarray(edge_index[0]).tolist(), np.asarray(edge_index[1]).tolist()):
        true[v].add(u)
    G = 1 if graph_ptr is None else max(len(graph_ptr) - 1, 1)
    g = graph_of(N, graph_ptr)
    n_hit = np.zeros(N, dtype=np.int32)
    rec = np.zeros((G, 5), dtype=np.int64)
    for v in range(N):
        dec = {int(x) for x in idx[v] if int(x) != -1}
        hits = len(dec & true[v])
        n_hit[v] = hits
        if true[v] and g[v] < G:
            rec[g[v]] += (1, int(dec == true[v]), hits, len(true[v]), len(dec))
    return n_hit, rec


def recovery_case(seed=1):
    """Designed lists, K = 3, N = 700 (three workgroups of 256 rows).  Graphs of (3, 70, 0, 200, 130, 297) nodes: borders inside a
    wave, an empty graph, a graph across a workgroup border; graph 0 (3 nodes) and graph 4 (130 nodes) have NO gate (no edge ends in
    them).  The true edges are listed with repeats.  The decoded lists start as the true sets (in a shuffled order) and are then
    damaged: a -1 in place of a fan-in, an id out of range (N + 5, -7, 2^31 - 1), a wrong id, a repeated id, and decoded fan-ins on rows
    whose true list is empty (counted nowhere but in n_hit = 0)."""
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    sizes = (3, 70, 0, 200, 130, 297)
    gp = [0]
    for n in sizes:
        gp.append(gp[-1] + n)
    N, K = gp[-1], 3
    src, dst = [], []
    for g in (1, 3, 5):
        lo, hi = gp[g], gp[g + 1]
        for v in range(lo + 4, hi):
            if rng.random() < 0.2:
                continue                                   # a node of a gate graph with an empty true list
            for u in rng.choice(np.arange(lo, v), size=int(rng.integers(1, 4)), replace=False):
                src.append(int(u))
                dst.append(v)
    E = len(src)
    rep = rng.integers(0, E, size=E // 5)                  # repeated true edges
    edge_index = np.array([src + [src[i] for i in rep], dst + [dst[i] for i in rep]], dtype=np.int64)
    perm = rng.permutation(edge_index.shape[1])
    edge_index = edge_index[:, perm]
    idx = np.full((N, K), -1, dtype=np.int32)
    true = [[] for _ in range(N)]
    for u, v in zip(src, dst):
        true[v].append(u)
    kinds = {}
    for v in range(N):
        row = list(rng.permutation(true[v]))
        kind = int(rng.integers(0, 8)) if row else (8 if rng.random() < 0.3 else 9)
        if kind == 1:
            row[0] = -1
        elif kind == 2:
            row[0] = (N + 5, -7, 2 ** 31 - 1)[v % 3]
        elif kind == 3:
            row[0] = (row[0] + 1) % N
        elif kind == 4 and len(row) < K:
            row.append(row[0])                             # a repeated id: still the same set
        elif kind == 5 and len(row) < K:
            row.append(int(rng.integers(0, N)))            # one more than the true set (or a repeat, rarely)
        elif kind == 8:
            row = [int(rng.integers(0, N)), N + 1]         # decoded fan-ins where nothing is true
        kinds[kind] = kinds.get(kind, 0) + 1
        idx[v, :len(row)] = row
    return dict(N=N, K=K, idx=idx, edge_index=edge_index, graph_ptr=gp, kinds=kinds)
