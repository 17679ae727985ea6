"""The negative sampler (csrc/neg_sample.hip + the two mgv_sort_lists_i32 calls of sampling.negative_sampling_device) restated in numpy.

The device's draw is no random variable from a test's point of view: slot i of a call is a pure function of (seed, i, N, the positive
out-lists), and after the per-list sort so is every array of NegativeEdges.  This file restates that function from the header's
contract (include/mgvae_hip.h) and the kernel's comments, on uint64 arrays (which wrap silently, as the device's words do), so that
the GPU tests can ask for integer equality at any shape.  tests/test_neg_sample_spec.py holds it on the CPU: the mixer against its
published outputs, the distribution against a chi-square, and planted defects against the comparison helpers below.

    slot i:      ctr = seed ^ (i * 0xD1342543DE82EF95)
    attempt a:   r = splitmix64(ctr + a),  s = (hi32(r) * N) >> 32,  d = (lo32(r) * N) >> 32        a = 0 .. 64
    accepted when s != d and (s, d) is no positive edge; the pair of attempt 64 is kept whatever it is."""
import functools

import numpy as np

M64 = (1 << 64) - 1
SLOT_MUL = 0xD1342543DE82EF95
CAP = 64                            # the last attempt's number: 65 draws at the most
GRID_SLOTS = 4096 * 256             # k_neg_sample's grid is capped at 256 CUs x 16 workgroups of 256 threads
SHORT_LIST, HEAVY_LDS, HEAVY_BLOCKS = 32, 4096, 256          # csrc/plan_build.hip: register sort up to 32, bitonic up to 4,096, 256 blocks

# the planted defects of the spec file: each names what the restatement does wrong when asked to
DRAW_DEFECTS = ('skip_last', 'swap_halves', 'cap_63', 'add_not_xor', 'seed_63_bits')
BUCKET_DEFECTS = ('arrival_order', 'in_counts_from_src')


def seed_of(base, call):
    """The 64-bit seed of call number `call` under torch seed `base`, as sampling.negative_sampling_device derives it."""
    return (int(base) * 0x9E3779B97F4A7C15 + int(call) * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & M64


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def splitmix64(x):
    """Vigna's splitmix64 output function of the state x + golden gamma (uint64 in, uint64 out)."""
    with np.errstate(over='ignore'):
        x = _u64(x) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def slot_counters(E, seed, defect=None):
    with np.errstate(over='ignore'):
        step = np.arange(int(E), dtype=np.uint64) * np.uint64(SLOT_MUL)
        return np.uint64(seed) + step if defect == 'add_not_xor' else np.uint64(seed) ^ step


def raw_pairs(ctr, attempt, N, defect=None):
    """(s, d) int64 that the counters `ctr` draw at `attempt`, before any test."""
    with np.errstate(over='ignore'):
        r = splitmix64(_u64(ctr) + np.uint64(attempt))
    hi, lo = r >> np.uint64(32), r & np.uint64(0xFFFFFFFF)
    if defect == 'swap_halves':
        hi, lo = lo, hi
    n = np.uint64(N)                                     # N < 2^31: the products stay below 2^63
    return ((hi * n) >> np.uint64(32)).astype(np.int64), ((lo * n) >> np.uint64(32)).astype(np.int64)


def edge_keys(pos_edge_index, N, defect=None):
    """Sorted distinct s*N+d keys that the edge test rejects.  'skip_last': the walk stops one entry short of every out-list (lists keep
    the original edge order, so the entry lost is each source's last edge)."""
    pos = np.asarray(pos_edge_index, dtype=np.int64).reshape(2, -1)
    if defect == 'skip_last' and pos.shape[1]:
        order = np.argsort(pos[0], kind='stable')
        s = pos[0][order]
        last = np.r_[s[1:] != s[:-1], True]
        pos = pos[:, order[~last]]
    return np.unique(pos[0] * int(N) + pos[1])


def draw(N, E, seed, pos_edge_index, defect=None):
    """-> (src[E], dst[E], attempts[E]) int64: every slot's kept pair and the number of the attempt that gave it."""
    N, E, seed = int(N), int(E), int(seed) & M64
    assert 2 <= N < 2 ** 31 and E >= 0 and (defect is None or defect in DRAW_DEFECTS)
    keys = edge_keys(pos_edge_index, N, defect)
    if defect == 'seed_63_bits':
        seed &= (1 << 63) - 1
    cap = 63 if defect == 'cap_63' else CAP
    ctr = slot_counters(E, seed, defect)
    src, dst, attempts = (np.zeros(E, dtype=np.int64) for _ in range(3))
    todo = np.arange(E)
    for a in range(cap + 1):
        if todo.size == 0:
            break
        s, d = raw_pairs(ctr[todo], a, N, defect)
        src[todo], dst[todo], attempts[todo] = s, d, a
        todo = todo[(s == d) | np.isin(s * N + d, keys)]
    return src, dst, attempts


def _ptr(idx, N):
    p = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=N), out=p[1:])
    return p.astype(np.int32)


def buckets(src, dst, N, defect=None):
    """The five arrays of NegativeEdges: edge_index [2, E] int64 sorted by (src, dst), out_ptr [N+1], out_dst [E], in_ptr [N+1],
    in_src [E] (int32; the sources of each destination ascending)."""
    assert defect is None or defect in BUCKET_DEFECTS
    src, dst, N = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), int(N)
    if defect == 'arrival_order':                        # lists left as an in-order fill leaves them
        by_src, by_dst = np.argsort(src, kind='stable'), np.argsort(dst, kind='stable')
    else:
        by_src, by_dst = np.lexsort((dst, src)), np.lexsort((src, dst))
    out_ptr = _ptr(src, N)
    in_ptr = out_ptr.copy() if defect == 'in_counts_from_src' else _ptr(dst, N)
    return (np.stack([src[by_src], dst[by_src]]), out_ptr, dst[by_src].astype(np.int32), in_ptr, src[by_dst].astype(np.int32))


def ranks(idx, N, how, rng=None):
    """A valid rank assignment of the bucket pass: rank[i] = slot i's place inside the bucket of idx[i], every bucket's ranks a
    permutation of 0..count-1.  'ascending' = slot order (one thread after the other), 'reversed', 'random' (inside each bucket)."""
    idx = np.asarray(idx, dtype=np.int64)
    tie = np.arange(idx.size) if how != 'random' else rng.permutation(idx.size)
    order = np.lexsort((tie, idx))
    rank = np.empty(idx.size, dtype=np.int64)
    rank[order] = np.arange(idx.size) - _ptr(idx, N)[:-1].astype(np.int64)[idx[order]]
    if how == 'reversed':
        rank = np.bincount(idx, minlength=N)[idx] - 1 - rank
    return rank.astype(np.int32)


def fill(src, dst, N, rank_out, rank_in):
    """k_neg_bucket on the host: the five arrays before the per-list sorts."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    out_ptr, in_ptr = _ptr(src, N), _ptr(dst, N)
    p, q = out_ptr[src].astype(np.int64) + rank_out, in_ptr[dst].astype(np.int64) + rank_in
    ei = np.empty((2, src.size), dtype=np.int64)
    out_dst, in_src = np.empty(src.size, dtype=np.int32), np.empty(src.size, dtype=np.int32)
    ei[0, p], ei[1, p], out_dst[p], in_src[q] = src, dst, dst, src
    return ei, out_ptr, out_dst, in_ptr, in_src


def sort_lists(ptr, vals):
    """Every list vals[ptr[n] : ptr[n+1]] ascending (np.sort per list)."""
    vals = np.array(vals)
    for n in range(len(ptr) - 1):
        vals[ptr[n]:ptr[n + 1]] = np.sort(vals[ptr[n]:ptr[n + 1]])
    return vals


def sort_paths(ptr):
    """How many lists of a CSR each path of mgv_sort_lists_i32 takes: {'none' (<= 1 entry), 'register' (<= 32), 'bitonic' (<= 4,096),
    'rank'}, plus 'heavy_rounds' = trips of k_sort_heavy's block loop."""
    d = np.diff(np.asarray(ptr, dtype=np.int64))
    heavy = int((d > SHORT_LIST).sum())
    return {'none': int((d <= 1).sum()), 'register': int(((d > 1) & (d <= SHORT_LIST)).sum()),
            'bitonic': int(((d > SHORT_LIST) & (d <= HEAVY_LDS)).sum()), 'rank': int((d > HEAVY_LDS).sum()),
            'heavy_rounds': -(-heavy // HEAVY_BLOCKS)}


def grid_passes(E):
    return -(-int(E) // GRID_SLOTS)


def _first_diff(a, b):
    return int(np.flatnonzero(np.asarray(a) != np.asarray(b))[0])


def assert_same_draw(got, ref):
    """got, ref: (src, dst[, ...]).  Exact equality, slot by slot."""
    for k, name in enumerate(('src', 'dst')):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, 'neg_%s holds %s slots, the restatement %s' % (name, g.shape, r.shape)
    bad = (np.asarray(got[0]) != np.asarray(ref[0])) | (np.asarray(got[1]) != np.asarray(ref[1]))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError('slot %d of %d: drew (%d, %d), the restatement (%d, %d)%s; %d slots differ'
                             % (i, bad.size, got[0][i], got[1][i], ref[0][i], ref[1][i],
                                ' at attempt %d' % ref[2][i] if len(ref) > 2 else '', int(bad.sum())))


def assert_same_buckets(got, ref):
    """got, ref: (edge_index, out_ptr, out_dst, in_ptr, in_src); payload arrays may be longer than E (the device pads E = 0 to 1)."""
    E = ref[0].shape[1]
    g_ei = np.asarray(got[0])
    assert g_ei.shape == (2, E), 'edge_index is %s, the restatement (2, %d)' % (g_ei.shape, E)
    for k, name in ((1, 'out_ptr'), (3, 'in_ptr')):
        g, r = np.asarray(got[k]), ref[k]
        assert g.shape == r.shape, '%s has %s entries, the restatement %s' % (name, g.shape, r.shape)
        if (g != r).any():
            n = _first_diff(g, r)
            raise AssertionError('%s[%d] = %d, the restatement %d (list %d)' % (name, n, g[n], r[n], max(n - 1, 0)))
    for g, r, ptr, name in ((g_ei[0], ref[0][0], ref[1], 'edge_index[0]'), (g_ei[1], ref[0][1], ref[1], 'edge_index[1]'),
                            (np.asarray(got[2])[:E], ref[2], ref[1], 'out_dst'), (np.asarray(got[4])[:E], ref[4], ref[3], 'in_src')):
        assert g.shape == r.shape, '%s has %s entries, the restatement %s' % (name, g.shape, r.shape)
        if (g != r).any():
            p = _first_diff(g, r)
            n = int(np.searchsorted(ptr, p, side='right') - 1)
            raise AssertionError('%s: list %d (%d entries) differs at its entry %d: %d, the restatement %d'
                                 % (name, n, ptr[n + 1] - ptr[n], p - ptr[n], g[p], r[p]))


# ---- the cases the spec file and the GPU file share ----

def tiny_graph(N, P):
    """P positive edges over N nodes from np.random.default_rng(0), duplicates and self loops left in."""
    return np.random.default_rng(0).integers(0, N, size=(2, P)).astype(np.int64)


TINY = ((8, 20, 200000), (5, 8, 100000), (64, 600, 1000000))        # N, positive edges, draws
SEEDS = (seed_of(0, 0), seed_of(2 ** 63 + 5, 3))                   # of every C-ABI case
COMPLETE2 = np.array([[0, 1], [1, 0]], dtype=np.int64)
ONE_FREE_OF_3 = np.array([[0, 0, 1, 1, 2], [1, 2, 0, 2, 0]], dtype=np.int64)        # (2, 1) is the one free pair
LONG_NODE, LONG_LEN = 7, 3500


def long_list_case(seed):
    """N = 3,000, node 7 with a 3,500-entry out-list (duplicates, as 3,000 nodes force) whose LAST entry t occurs nowhere else in the
    list and is drawn, per the restatement, by slot `slot` at attempt 0: an edge walk that stops one entry short accepts it."""
    N, E = 3000, 30000
    s0, d0 = raw_pairs(slot_counters(E, seed), 0, N)
    slot = int(np.flatnonzero((s0 == LONG_NODE) & (d0 != LONG_NODE))[0])
    t = int(d0[slot])
    rng = np.random.default_rng(7)
    lst = rng.integers(0, N, size=LONG_LEN - 1)
    lst[lst == t] = (t + 1) % N
    other = rng.integers(0, N, size=(2, 2000))
    other[0][other[0] == LONG_NODE] = LONG_NODE + 1
    mine = np.stack([np.full(LONG_LEN, LONG_NODE), np.r_[lst, t]])
    pos = np.concatenate([other[:, :1000], mine, other[:, 1000:]], axis=1).astype(np.int64)
    return dict(N=N, E=E, pos=pos, slot=slot, t=t)


def three_pass_case():
    N = 1 << 20
    return dict(N=N, E=3 * N + 5, pos=np.random.default_rng(11).integers(0, N, size=(2, 2 * N)).astype(np.int64))


def abi_cases(seed):
    """name -> dict(N, E, pos) of every mgv_neg_sample case that runs at both seeds."""
    none = np.zeros((2, 0), dtype=np.int64)
    cases = {'2 nodes, no edges, E=%d' % E: dict(N=2, E=E, pos=none) for E in (1, 255, 256, 257)}
    cases['2 nodes complete (the cap)'] = dict(N=2, E=1000, pos=COMPLETE2)
    cases['3 nodes, one free pair'] = dict(N=3, E=5000, pos=ONE_FREE_OF_3)
    for N, P, E in (TINY[0], TINY[2]):
        cases['tiny %d/%d' % (N, P)] = dict(N=N, E=E, pos=tiny_graph(N, P))
    cases['long out-list'] = long_list_case(seed)
    cases['E=0'] = dict(N=8, E=0, pos=tiny_graph(8, 20))
    return cases


@functools.lru_cache(maxsize=None)
def case_draw(name, seed):
    """The restatement's draw of an ABI case, computed once and shared (callers leave the arrays unchanged)."""
    c = three_pass_case() if name == 'three passes' else abi_cases(seed)[name]
    out = draw(c['N'], c['E'], seed, c['pos'])
    for a in out:
        a.setflags(write=False)
    return c, out


# the seed whose top bit is set (both SEEDS lie below 2^63): 'tiny 8/20' runs at it as well, and the Python-surface cases use it
HIGH_SEED = seed_of(1234, 0)


def surface_cases():
    """name -> dict(N, pos, num (None: the count E - loops + N), base (torch seed), call (number of the call)) of the cases that go
    through sampling.negative_sampling_device; `path` names what the reference's list lengths must reach (checked by sort_paths)."""
    none = np.zeros((2, 0), dtype=np.int64)
    sparse = np.random.default_rng(5).integers(0, 300, size=(2, 400)).astype(np.int64)
    return {
        'count with loops and duplicates': dict(N=64, pos=tiny_graph(64, 600), num=None, base=1234, call=0, path=None),
        'num_neg_samples given': dict(N=64, pos=tiny_graph(64, 600), num=1000, base=1234, call=5, path=None),
        'rank path': dict(N=2, pos=none, num=10000, base=1234, call=0, path='rank'),
        'bitonic path': dict(N=3, pos=none, num=10000, base=1234, call=0, path='bitonic'),
        'lists of 32 and 33': dict(N=300, pos=sparse, num=10000, base=1234, call=0, path='32/33'),
        'all lists heavy': dict(N=300, pos=sparse, num=30000, base=1234, call=0, path='heavy loop'),
    }


def count_of(N, pos):
    """E - self loops + N: what the sampler draws when no count is given."""
    return int(pos.shape[1] - (pos[0] == pos[1]).sum()) + int(N)


@functools.lru_cache(maxsize=None)
def surface_ref(name):
    """(case, draw, buckets) of a surface case from the restatement, computed once."""
    c = surface_cases()[name]
    E = count_of(c['N'], c['pos']) if c['num'] is None else c['num']
    d = draw(c['N'], E, seed_of(c['base'], c['call']), c['pos'])
    return c, d, buckets(d[0], d[1], c['N'])


# ---- mgv_sort_lists_i32 on its own ----

SORT_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 9001)


def sort_case_lengths():
    """(ptr [17] int32, E): one CSR with a list on either side of every length at which the sort changes its path."""
    ptr = np.r_[0, np.cumsum(SORT_LENGTHS)].astype(np.int32)
    return ptr, int(ptr[-1])


def many_heavy_ptr():
    """600 lists of 40 entries: more heavy lists than k_sort_heavy has blocks."""
    return (np.arange(601) * 40).astype(np.int32)
