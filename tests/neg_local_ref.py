"""The local draw of the negative sampler (csrc/mgv_neg_draw.h: neg_draw_slot_local; entries mgv_neg_draw_local and
mgv_neg_partition_local) restated in numpy on uint64, next to tests/neg_sample_ref.py, whose mixer, counters, edge keys, buckets and
assert helpers it uses unchanged.

    slot i:      ctr = seed ^ (i * 0xD1342543DE82EF95)
    attempt a:   r = splitmix64(ctr + a),  hi = r >> 32,  lo = r & 0xFFFFFFFF                         a = 0 .. 64
      i <  R:    e = (hi * Epos) >> 32,  s = in_dst[e],  d = in_src[e]                                (the reversal of a listed edge)
      i >= R:    s = (hi * N) >> 32,  g = the largest g < G with graph_ptr[g] <= s,
                 d = graph_ptr[g] + ((lo * (graph_ptr[g + 1] - graph_ptr[g])) >> 32)                 (uniform over s's own graph)
    accepted when s != d and (s, d) is no positive edge; the pair of attempt 64 is kept whatever it is.

(in_src[e], in_dst[e]) is the positive edge list in the order GraphPlan holds it: grouped by destination, edge order kept inside a
group (plan_in_lists).  With graph_ptr = [0, N] and R = 0 this is neg_sample_ref.draw."""
import functools

import numpy as np

from neg_sample_ref import (CAP, M64, SEEDS, assert_same_buckets, assert_same_draw, buckets, count_of, edge_keys,  # noqa: F401
                            seed_of, slot_counters, splitmix64)

GRAPH_LDS = 4096                    # csrc/mgv_neg_draw.h: kNegGraphLds, the graphs whose table the drawing kernels keep in LDS
NP_CAP = 16384                      # csrc/neg_partition.hip: kNpCap

# the planted defects of the spec file: each names what the restatement does wrong when asked to
DEFECTS = ('d_global', 'graph_from_d', 'next_ptr', 'lower_bound', 'not_reversed', 'e_from_lo', 'rev_le_R')


def plan_in_lists(pos):
    """(in_src, in_dst) as GraphPlan holds the positive edges: a stable sort by destination."""
    pos = np.asarray(pos, dtype=np.int64).reshape(2, -1)
    order = np.argsort(pos[1], kind='stable')
    return pos[0][order], pos[1][order]


def check_graph_ptr(graph_ptr, N):
    gp = np.asarray(graph_ptr, dtype=np.int64)
    assert gp.ndim == 1 and gp.size >= 2 and gp[0] == 0 and gp[-1] == int(N) and bool((np.diff(gp) >= 0).all()), 'not a graph table'
    return gp


def reverse_count(reverse, E):
    """R = floor(reverse * E + 0.5), as sampling.negative_sampling_device derives it."""
    return int(np.floor(float(reverse) * int(E) + 0.5))


def graph_of(gp, ids, side='right'):
    """The largest g < G with gp[g] <= id (an upper bound minus one; 'left': the planted lower bound)."""
    return np.clip(np.searchsorted(gp, ids, side=side) - 1, 0, gp.size - 2)


def draw_local(N, E, seed, pos_edge_index, graph_ptr, R=0, in_lists=None, defect=None):
    """-> (src[E], dst[E], attempts[E]) int64: every slot's kept pair and the number of the attempt that gave it."""
    N, E, R, seed = int(N), int(E), int(R), int(seed) & M64
    gp = check_graph_ptr(graph_ptr, N)
    in_src, in_dst = (np.asarray(a, dtype=np.int64) for a in (in_lists if in_lists is not None else plan_in_lists(pos_edge_index)))
    Epos = int(in_src.size)
    assert 2 <= N < 2 ** 31 and E >= 0 and 0 <= R <= E and (R == 0 or Epos > 0) and (defect is None or defect in DEFECTS)
    keys = edge_keys(pos_edge_index, N)
    ctr = slot_counters(E, seed)
    src, dst, attempts = (np.zeros(E, dtype=np.int64) for _ in range(3))
    todo = np.arange(E)
    u = np.uint64
    for a in range(CAP + 1):
        if todo.size == 0:
            break
        with np.errstate(over='ignore'):
            r = splitmix64(ctr[todo] + u(a))
        hi, lo = r >> u(32), r & u(0xFFFFFFFF)
        s = ((hi * u(N)) >> u(32)).astype(np.int64)
        if defect == 'graph_from_d':                         # the graph looked up from a batch-wide destination, the source inside it
            d = ((lo * u(N)) >> u(32)).astype(np.int64)
            g = graph_of(gp, d)
            s = gp[g] + ((hi * (gp[g + 1] - gp[g]).astype(u)) >> u(32)).astype(np.int64)
        else:
            g = graph_of(gp, s, 'left' if defect == 'lower_bound' else 'right')
            base = gp[g + 1] if defect == 'next_ptr' else gp[g]
            d = base + ((lo * (gp[g + 1] - gp[g]).astype(u)) >> u(32)).astype(np.int64)
            if defect == 'd_global':
                d = ((lo * u(N)) >> u(32)).astype(np.int64)
            d = np.minimum(d, N - 1)                        # (only a planted defect can reach past the last node)
        rev = todo <= R if defect == 'rev_le_R' and Epos > 0 else todo < R
        if rev.any():
            e = (((lo if defect == 'e_from_lo' else hi)[rev] * u(Epos)) >> u(32)).astype(np.int64)
            s[rev], d[rev] = (in_src[e], in_dst[e]) if defect == 'not_reversed' else (in_dst[e], in_src[e])
        src[todo], dst[todo], attempts[todo] = s, d, a
        todo = todo[(s == d) | np.isin(s * N + d, keys)]
    return src, dst, attempts


# ---- the cases the spec file and the GPU file share ----

DESIGNED_SIZES = (1, 2, 3, 63, 64, 65, 700, 4096, 4097)


def table_of(sizes):
    return np.r_[0, np.cumsum(np.asarray(sizes, dtype=np.int64))].astype(np.int64)


def edges_inside(gp, per_node, rng):
    """per_node x n random positives inside every graph of n >= 3 nodes (duplicates and self loops left in), both edges of a 2-node
    graph (complete), the self loop of a 1-node graph."""
    parts = []
    for a, b in zip(gp[:-1], gp[1:]):
        n = int(b - a)
        if n == 1:
            parts.append(np.array([[a], [a]]))
        elif n == 2:
            parts.append(np.array([[a, a + 1], [a + 1, a]]))
        elif n > 2:
            parts.append(a + rng.integers(0, n, size=(2, per_node * n)))
    pos = np.concatenate(parts, axis=1).astype(np.int64) if parts else np.zeros((2, 0), dtype=np.int64)
    return pos[:, rng.permutation(pos.shape[1])]


@functools.lru_cache(maxsize=None)
def batches():
    """name -> dict(N, gp, pos): the designed batches."""
    out = {}
    gp = table_of(DESIGNED_SIZES)
    out['nine graphs'] = dict(N=int(gp[-1]), gp=gp, pos=edges_inside(gp, 3, np.random.default_rng(31)))
    out['two 1-node graphs'] = dict(N=2, gp=table_of((1, 1)), pos=np.zeros((2, 0), dtype=np.int64))
    gp = table_of((2,) * 40)
    out['complete 2-node graphs'] = dict(N=80, gp=gp, pos=edges_inside(gp, 0, np.random.default_rng(32)))
    gp = np.array([0, 0, 5, 5, 9], dtype=np.int64)
    out['empty graphs in the table'] = dict(N=9, gp=gp, pos=edges_inside(gp, 1, np.random.default_rng(33)))
    for G in (GRAPH_LDS, GRAPH_LDS + 1):                     # on both sides of the LDS table cap: graphs of 1 to 3 nodes
        gp = table_of(1 + np.arange(G) % 3)
        out['%d small graphs' % G] = dict(N=int(gp[-1]), gp=gp, pos=edges_inside(gp, 1, np.random.default_rng(34)))
    for c in out.values():
        for a in (c['gp'], c['pos']):
            a.setflags(write=False)
    return out


def slot_counts(c):
    """The E values a designed batch runs at: nothing, one slot, a whole chunk, a chunk and a slot, the count rule's."""
    return (0, 1, 16384, 16385, count_of(c['N'], c['pos']))


HUB, HUB_OUT = 5, 20000


@functools.lru_cache(maxsize=None)
def hub_case():
    """Two graphs (25,000 + 1,000 nodes); node 5 points at 20,000 distinct nodes of its graph, 10,000 random edges beside them;
    R = E = 40,000: about two thirds of the slots are (v, 5), so node 5's negative in-list passes a finishing trip's capacity."""
    rng = np.random.default_rng(35)
    gp = table_of((25000, 1000))
    hub = np.stack([np.full(HUB_OUT, HUB), 100 + rng.permutation(24000)[:HUB_OUT]])
    other = np.stack([rng.integers(6, 26000, size=10000), rng.integers(6, 26000, size=10000)])
    pos = np.concatenate([hub, other], axis=1)[:, rng.permutation(HUB_OUT + 10000)].astype(np.int64)
    return dict(N=26000, gp=gp, pos=pos, E=40000, R=40000)


@functools.lru_cache(maxsize=None)
def ref(name, E, R, seed):
    """(draw, buckets) of a designed batch (or 'hub') from the restatement, computed once and left unchanged."""
    c = hub_case() if name == 'hub' else batches()[name]
    d = draw_local(c['N'], E, seed, c['pos'], c['gp'], R)
    b = buckets(d[0], d[1], c['N'])
    for a in d + b:
        a.setflags(write=False)
    return d, b
