"""The decoder on ALL node pairs (digae_layer.py:31-33) at any size: dense scores under autograd, and the streamed consumers of one
tile walk — top-k links, thresholded link lists, score histograms — with the reconstruction counts and curves made from them.
Added functionality beside the train step: it reads none of ops' switches, uses none of its workspaces and depends on _hip only
(ops re-binds the public names; similarity and metrics build on this module).
"""
import torch

from . import _hip
from ._hip import F32, I32, HipLibraryError, check, edge_rows, ptr


def _pair_rows(x, name):
    """(tensor, row stride) as the pair-score launchers take an operand: fp32 rows with unit column stride, a row stride that is a
    multiple of 4 and a 16-byte aligned base — a column half of st = hs_decompose(hs) goes in as it is, anything else is copied."""
    x = x.detach()
    if x.dim() != 2:
        raise HipLibraryError('%s must be a matrix [rows, H] (got shape %s)' % (name, tuple(x.shape)))
    if not x.is_cuda:
        raise HipLibraryError('%s must live on the GPU (got %s); the hot path has no CPU implementation' % (name, x.device))
    if x.dtype != F32:
        raise HipLibraryError('%s must be %s (got %s)' % (name, F32, x.dtype))
    rows_ok = x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
    if x.shape[0] <= 1 or not rows_ok:
        x = x.contiguous()
    return x, _pair_ld(x)


def _pair_ld(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def _pair_operands(s, t):
    sd, lds = _pair_rows(s, 's')
    td, ldt = _pair_rows(t, 't')
    if sd.shape[1] != td.shape[1]:
        raise HipLibraryError('s and t must have the same width (got %d and %d)' % (sd.shape[1], td.shape[1]))
    return sd, lds, td, ldt, sd.shape[1]


def _same_rows(sd, td, opening):
    """N of a walk over the nodes of one batch; `opening` names the caller and what it does with them."""
    N = sd.shape[0]
    if td.shape[0] != N:
        raise HipLibraryError('%s: s and t need the same number of rows (got %d and %d)' % (opening, N, td.shape[0]))
    return N


_PAIR_WIDTHS = (16, 32, 64, 128)          # csrc/mgv_launch.h AllWidths


def _pair_width(x, name):
    if x.dim() == 2 and x.shape[1] not in _PAIR_WIDTHS:
        raise HipLibraryError('%s: MGV_EUNSUPPORTED (unsupported size): the pair kernels serve H in %s, got %d'
                              % (name, list(_PAIR_WIDTHS), x.shape[1]))


def _pair_graphs(graph_ptr, dev):
    """(gp int32 [G + 1] on the device, G) as the walk entries take a batch's graphs; None: (None, 0), one graph."""
    if graph_ptr is None:
        return None, 0
    gp = torch.as_tensor(graph_ptr).to(device=dev, dtype=I32).contiguous()
    if gp.numel() < 1:
        raise HipLibraryError('graph_ptr needs at least one entry')
    return gp, gp.numel() - 1


def _graph_ptr64(graph_ptr, dev):
    """graph_ptr as int64 [G + 1] on `dev`, for the torch side of a per-graph sum."""
    return torch.as_tensor(graph_ptr).to(device=dev, dtype=torch.int64)


def _graph_of(rows, gp, G):
    """The graph of each node id in `rows` (gp int64 [G + 1], G >= 1); an id past the last graph counts for the last."""
    return torch.bucketize(rows, gp[1:].contiguous(), right=True).clamp_(max=G - 1)


def _list_rows(row_ptr, total):
    """int64 [total]: the row of every entry of the lists row_ptr [N + 1] delimits."""
    N = row_ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=row_ptr.device), row_ptr[1:] - row_ptr[:-1],
                                   output_size=total)


def _free_bytes(dev):
    free, _ = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)  # blocks the caching allocator can hand out again


def _dense_fits(M, N, dev):
    """A dense M x N result the device cannot hold is refused here, by name, instead of by the allocator."""
    need = 4 * M * N
    free = _free_bytes(dev)
    if need > free:
        raise HipLibraryError('dense scores of %d x %d pairs need %.1f GiB, the device has %.1f GiB free: use the streaming form, '
                              'ops.pair_topk / DirectedInnerProductDecoder.topk (top-k links and counts per row, no N x N array)'
                              % (M, N, need / 2.0 ** 30, free / 2.0 ** 30))


class PairScoresFn(torch.autograd.Function):
    """out[i, j] = sigma(<s_i, t_j>) over all pairs (digae_layer.py:31-33), exact fp32 in ascending k; the backward writes ds = G t and
    dt = G^T s without atomics (mgv_pair_scores_bwd)."""

    @staticmethod
    def forward(ctx, s, t, sigmoid):
        sd, lds, td, ldt, H = _pair_operands(s, t)
        M, N = sd.shape[0], td.shape[0]
        _dense_fits(M, N, sd.device)
        out = torch.empty((M, N), dtype=F32, device=sd.device)
        _hip.call('mgv_pair_scores_fwd', H, M, N, ptr(sd), lds, ptr(td), ldt, int(bool(sigmoid)), ptr(out), max(N, 1))
        ctx.save_for_backward(sd, td, out)
        ctx.sigmoid = bool(sigmoid)
        return out

    @staticmethod
    def backward(ctx, gout):
        sd, td, out = ctx.saved_tensors
        lds, ldt = _pair_ld(sd), _pair_ld(td)
        M, N, H = sd.shape[0], td.shape[0], sd.shape[1]
        gout = check(gout.contiguous(), F32, 'gout')
        ds = torch.empty((M, H), dtype=F32, device=sd.device) if ctx.needs_input_grad[0] else None
        dt = torch.empty((N, H), dtype=F32, device=sd.device) if ctx.needs_input_grad[1] else None
        _hip.call('mgv_pair_scores_bwd', H, M, N, ptr(sd), lds, ptr(td), ldt, int(ctx.sigmoid), ptr(out), max(N, 1), ptr(gout), max(N, 1),
                  ptr(ds), H, ptr(dt), H)
        return ds, dt, None


def pair_scores(s, t, sigmoid=True):
    """Decoder scores of all M x N pairs at any size, under autograd."""
    return PairScoresFn.apply(s, t, sigmoid)


def pair_scores_at(s, t, edge_index, sigmoid=True):
    """Scores of the listed pairs in the arithmetic of pair_scores: equal to pair_scores(s, t)[src, dst] bit for bit (no grad; the
    training path's per-edge decoder is edge_dot)."""
    sd, lds, td, ldt, H = _pair_operands(s, t)
    src, dst = edge_rows(edge_index)
    E = src.numel()
    out = torch.empty(E, dtype=F32, device=sd.device)
    _hip.call('mgv_pair_scores_at', H, E, ptr(sd), lds, ptr(td), ldt, ptr(src), ptr(dst), int(bool(sigmoid)), ptr(out))
    return out


def pair_topk(s, t, k, graph_ptr=None, sigmoid=True, threshold=0.5, skip_self=False):
    """(idx [N, k] int32, score [N, k], n_above [N] int32) per row u over the nodes of u's own graph (graph_ptr [G + 1], None: one graph):
    the k best links by raw dot product (ties: lower id first; -1 / -inf past the end) and the number of candidates whose score is
    > threshold.  Streaming: no N x N array.  No grad; nothing is read back except the two ends of a graph_ptr, which the launcher
    checks (None: no host synchronisation at all)."""
    sd, lds, td, ldt, H = _pair_operands(s, t)
    N = _same_rows(sd, td, 'pair_topk ranks the nodes of one batch')
    k = int(k)
    dev = sd.device
    gp, G = _pair_graphs(graph_ptr, dev)
    kk = min(max(k, 1), 32)
    idx = torch.empty((N, kk), dtype=I32, device=dev)
    score = torch.empty((N, kk), dtype=F32, device=dev)
    n_above = torch.empty(N, dtype=I32, device=dev)
    _hip.call('mgv_pair_topk', H, N, ptr(sd), lds, ptr(td), ldt, ptr(gp), G, k, int(bool(sigmoid)), float(threshold), int(bool(skip_self)),
              ptr(idx), ptr(score), ptr(n_above))
    return idx, score, n_above


def _list_room(name, total, free, *, noun, listed, limit_name, limit, item_bytes, hint):
    """The two refusals between a selection's count and its fill (nothing is allocated before them): more than the caller's
    `limit_name` allows, or a result — `listed` in words — of item_bytes per `noun` the device cannot hold; by name, like _dense_fits."""
    if limit is not None and total > int(limit):
        raise HipLibraryError('%s: %d %s are above the threshold, %s allows %d: %s' % (name, total, noun, limit_name, int(limit), hint))
    need = item_bytes * total
    if free is not None and need > free:
        raise HipLibraryError('%s: %s above the threshold need %.1f GiB, the device has %.1f GiB free: %s'
                              % (name, listed % total, need / 2.0 ** 30, free / 2.0 ** 30, hint))


def _select_room(total, with_scores, max_edges, free):
    """pair_select's refusals: lists of int32 ids, float32 scores beside them when asked for."""
    _list_room('pair_select', total, free, noun='links', listed='the lists of %d links', limit_name='max_edges', limit=max_edges,
               item_bytes=8 if with_scores else 4,
               hint='raise the threshold, or take the k best links per node with ops.pair_topk / DirectedInnerProductDecoder.topk')


def _count_scan_fill(count_entry, fill_entry, N, common, dev, with_scores, room):
    """(row_ptr int64 [N + 1], col int32 [total], score float32 [total] or None) of a selection walk over N rows with the arguments
    `common` of both entries: count, exclusive scan on the device, ONE read-back of the total (the result must be allocated), room(total, free
    bytes) — which refuses by raising —, allocate, fill."""
    n_sel = torch.empty(N, dtype=I32, device=dev)
    _hip.call(count_entry, *common, ptr(n_sel))
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_sel, 0, dtype=torch.int64, out=row_ptr[1:])
    total = int(row_ptr[-1])                                      # the read-back
    room(total, _free_bytes(dev))
    col = torch.empty(total, dtype=I32, device=dev)
    score = torch.empty(total, dtype=F32, device=dev) if with_scores else None
    _hip.call(fill_entry, *common, ptr(row_ptr), total, ptr(col), ptr(score))
    return row_ptr, col, score


def pair_select(s, t, graph_ptr=None, sigmoid=True, threshold=0.5, skip_self=False, by='src', with_scores=False, max_edges=None):
    """(row_ptr int64 [N + 1], col int32 [E'], score float32 [E'] or None): the reconstructed graph as per-node lists — for every row u
    the nodes v of u's own graph (graph_ptr [G + 1], None: one graph; without v = u when skip_self) whose score is > threshold, as
    batch-wide ids in ascending order at col[row_ptr[u] : row_ptr[u + 1]].  The decision is the one behind pair_topk's n_above, on the
    dense entry's bits.  by='src': row u lists its targets v (<s_u, t_v>); by='dst': the operands change places and row v lists its
    sources u, the in-neighbour lists — every product commutes and k keeps its order, so the scores are the dense entries, transposed.
    Count, exclusive scan on the device, ONE read-back of the total (the result must be allocated; the only synchronisation besides the
    two ends of a graph_ptr), fill; no atomics, the same bytes from call to call, nothing of size N^2.  A total above `max_edges` or
    beyond the free memory raises HipLibraryError before the fill.  No grad."""
    if by not in ('src', 'dst'):
        raise HipLibraryError("pair_select: by must be 'src' (row u lists its targets) or 'dst' (row v lists its sources), got %r" % (by,))
    if s.dim() == 2 and t.dim() == 2 and s.shape[1] == t.shape[1]:
        _pair_width(s, 'pair_select')
    if by == 'dst':
        s, t = t, s
    sd, lds, td, ldt, H = _pair_operands(s, t)
    N = _same_rows(sd, td, 'pair_select lists the nodes of one batch')
    gp, G = _pair_graphs(graph_ptr, sd.device)
    common = (H, N, ptr(sd), lds, ptr(td), ldt, ptr(gp), G, int(bool(sigmoid)), float(threshold), int(bool(skip_self)))
    return _count_scan_fill('mgv_pair_select_count', 'mgv_pair_select_fill', N, common, sd.device, with_scores,
                            lambda total, free: _select_room(total, with_scores, max_edges, free))


def reconstruct_edges(s, t, graph_ptr=None, threshold=0.5, skip_self=False, by='src', with_scores=False, max_edges=None):
    """(edge_index int64 [2, E'], row_ptr, score or None): pair_select's lists (sigmoid scores) as (source, target) rows in list order,
    whichever side they are listed by.  E' is reconstruction_counts(...)[:, 1].sum() by construction (skip_self off)."""
    row_ptr, col, score = pair_select(s, t, graph_ptr=graph_ptr, sigmoid=True, threshold=threshold, skip_self=skip_self, by=by,
                                      with_scores=with_scores, max_edges=max_edges)
    rows = _list_rows(row_ptr, col.numel())
    col = col.to(torch.int64)
    return torch.stack([rows, col] if by == 'src' else [col, rows]), row_ptr, score


def reconstruction_counts(s, t, edge_index, graph_ptr, threshold=0.5):
    """int64 [G, 4] on the device, per graph of the batch: {true positives, predicted positives over all n_g^2 ordered pairs, edges,
    ordered pairs} of the decoder at `threshold` against the FULL adjacency (the sampled counters of ReconLossFn see E + N non-edges
    of N^2 - E).  The true positives are pair_scores_at over the edges and the predicted positives the n_above of pair_topk: the same
    bits on both sides of the same `>`.  Integer sums throughout; precision = [:, 0] / [:, 1] and recall = [:, 0] / [:, 2] are the
    caller's divisions.  An edge counts for the graph of its source."""
    dev = s.device
    gp = _graph_ptr64(graph_ptr, dev)
    G = gp.numel() - 1
    src, dst = edge_rows(edge_index)
    _, _, n_above = pair_topk(s, t, 1, graph_ptr=gp, sigmoid=True, threshold=threshold, skip_self=False)
    if G <= 0:
        return torch.zeros((0, 4), dtype=torch.int64, device=dev)
    hit = (pair_scores_at(s, t, edge_index, sigmoid=True) > threshold).to(torch.int64)
    gid = _graph_of(src, gp, G)
    tp = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, gid, hit)                     # integer adds: exact in any order
    edges = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, gid, torch.ones_like(hit))
    cs = torch.zeros(s.shape[0] + 1, dtype=torch.int64, device=dev)
    cs[1:] = torch.cumsum(n_above.to(torch.int64), 0)
    n = gp[1:] - gp[:-1]
    return torch.stack([tp, cs[gp[1:]] - cs[gp[:-1]], edges, n * n], dim=1)


def dense_scores(s, t):
    """s t^T for `forward_all` at any size (raw dot products)."""
    return pair_scores(s, t, sigmoid=False)


# ------------------------------------------------------------------------------------------------
# the distribution of all-pair scores (added functionality: thresholds chosen by count; mgv_pair_hist / mgv_sim_hist)
# ------------------------------------------------------------------------------------------------
# The two facts at the head of similarity.py hold here too: zero rows score 0 with everything, equal rows score within (2H + 6) 2^-24 of 1.
PROFILE_MAX_EDGES = 256


def _profile_edges(edges, dev):
    """The table as the launchers take it: float32 [B] on the device, converted ONCE — every count refers to these float32 values."""
    e = torch.as_tensor(edges).detach().to(device=dev, dtype=F32).contiguous().flatten()
    if not 1 <= e.numel() <= PROFILE_MAX_EDGES:
        raise HipLibraryError('a profile takes 1 to %d edges (got %d)' % (PROFILE_MAX_EDGES, e.numel()))
    return e


def pair_profile(s, t, edges, graph_ptr=None, sigmoid=True, skip_self=False):
    """int64 [G, B + 1] on the device (G = 1 without graph_ptr): per graph, the candidates of pair_select — v in u's graph, without v = u
    when skip_self, sigmoid or raw score — binned by the number of `edges` (float32, strictly ascending, 1 <= B <= 256) their score is
    > than: bin 0 holds score <= edges[0], bin B score > edges[-1]; a NaN score is in no bin.  ONE all-pairs walk for the whole table
    (mgv_pair_hist), the decisions the bits of pair_select's: counts_above(profile)[g, j] is the number of links pair_select would
    list for graph g at threshold edges[j].  Integer atomics: exact and the same from call to call.  No grad."""
    if s.dim() == 2 and t.dim() == 2 and s.shape[1] == t.shape[1]:
        _pair_width(s, 'pair_profile')
    with torch.no_grad():
        sd, lds, td, ldt, H = _pair_operands(s, t)
        N = _same_rows(sd, td, 'pair_profile bins the pairs of one batch')
        dev = sd.device
        e = _profile_edges(edges, dev)
        gp, G = _pair_graphs(graph_ptr, dev)
        hist = torch.empty((max(G, 1), e.numel() + 1), dtype=torch.int64, device=dev)
        _hip.call('mgv_pair_hist', H, N, ptr(sd), lds, ptr(td), ldt, ptr(gp), G, int(bool(sigmoid)), int(bool(skip_self)), ptr(e), e.numel(),
                  ptr(hist))
        return hist if gp is None else hist[:G]


def counts_above(profile):
    """int64 [G, B]: pairs above each edge — the reverse cumulative sum of a profile without its bin 0."""
    with torch.no_grad():
        return profile[:, 1:].flip(1).cumsum(1).flip(1)


def reconstruction_curve(s, t, edge_index, graph_ptr, thresholds):
    """int64 [G, B, 4] on the device: reconstruction_counts at every threshold of `thresholds` (strictly ascending), entry for entry
    equal to torch.stack([reconstruction_counts(s, t, edge_index, graph_ptr, thr) for thr in thresholds], 1), from ONE all-pairs walk:
    the predicted positives are counts_above of pair_profile, the true positives pair_scores_at over the edges, binned by the same
    float32 table (bucketize: the number of thresholds the score is > than) and added per source graph.  Integer sums throughout."""
    with torch.no_grad():
        dev = s.device
        gp = _graph_ptr64(graph_ptr, dev)
        G = gp.numel() - 1
        e = _profile_edges(thresholds, dev)
        B = e.numel()
        src, dst = edge_rows(edge_index)
        pp = counts_above(pair_profile(s, t, e, graph_ptr=gp, sigmoid=True, skip_self=False))
        if G <= 0:
            return torch.zeros((0, B, 4), dtype=torch.int64, device=dev)
        rep = pair_scores_at(s, t, edge_index, sigmoid=True)
        k = torch.bucketize(rep, e, right=False)                       # #{j : rep > e[j]}
        ok = ~torch.isnan(rep)                                         # a NaN passes no threshold (bucketize would put it behind all)
        gid = _graph_of(src, gp, G)
        tbin = torch.zeros(G * (B + 1), dtype=torch.int64, device=dev).index_add_(0, gid * (B + 1) + k, ok.to(torch.int64))
        tp = counts_above(tbin.view(G, B + 1))
        edges = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, gid, torch.ones_like(gid))
        n = gp[1:] - gp[:-1]
        return torch.stack([tp, pp, edges[:, None].expand(G, B), (n * n)[:, None].expand(G, B)], dim=2)


# ------------------------------------------------------------------------------------------------
# decode embeddings into a legal circuit (added functionality: fan-ins by arity, acyclic; mgv_fanin_decode)
# ------------------------------------------------------------------------------------------------
FANIN_MAX = 8                             # csrc/pair_scores.hip kFaninMax


def _node_ints(x, N, name, dev):
    x = torch.as_tensor(x).detach().to(device=dev, dtype=I32).contiguous().flatten()
    if x.numel() != N:
        raise HipLibraryError('fanin_decode: %s needs one entry per node, %d (got %d)' % (name, N, x.numel()))
    return x


def fanin_decode(s, t, key, want, graph_ptr=None, K=None, skip=True):
    """(idx [N, K] int32, score [N, K], n_cand [N] int32): for every node v the fan-ins a legal circuit gives it.  A candidate of v is a
    node u of v's own graph (graph_ptr [G + 1], None: one graph) with key[u] < key[v] whose score <s_u, t_v> is not NaN — never v
    itself, and every edge runs from a smaller key to a larger one, so the result is acyclic whatever the scores are.  v keeps its
    min(max(want[v], 0), K) best candidates by raw dot product (ties: lower id first; -1 / -inf past the end); n_cand counts them all
    (0 for a node that wants nothing), so n_cand < want marks a gate that could not be completed.  The scores are the bits of
    pair_scores_at(s, t, sigmoid=False).  K defaults to want.max() clamped to [1, 8] (ONE read-back, avoided when K is given).
    skip: allocate the per-tile key minima by which the walk steps over column tiles that hold no candidate (the same bytes either
    way).  Streaming: nothing of size N x N; no atomics.  No grad."""
    if s.dim() == 2 and t.dim() == 2 and s.shape[1] == t.shape[1]:
        _pair_width(s, 'fanin_decode')
    with torch.no_grad():
        td, ldt, sd, lds, H = _pair_operands(t, s)                 # rows are targets: by='dst'
        N = _same_rows(sd, td, 'fanin_decode decodes the nodes of one batch')
        dev = sd.device
        key = _node_ints(key, N, 'key', dev)
        want = _node_ints(want, N, 'want', dev)
        if K is None:
            K = min(max(int(want.max()) if N > 0 else 1, 1), FANIN_MAX)          # the read-back
        K = int(K)
        gp, G = _pair_graphs(graph_ptr, dev)
        kk = min(max(K, 1), FANIN_MAX)
        idx = torch.empty((N, kk), dtype=I32, device=dev)
        score = torch.empty((N, kk), dtype=F32, device=dev)
        n_cand = torch.empty(N, dtype=I32, device=dev)
        tile_min = torch.empty((N + 63) // 64, dtype=I32, device=dev) if skip and N > 0 else None
        _hip.call('mgv_fanin_decode', H, N, ptr(td), ldt, ptr(sd), lds, ptr(gp), G, ptr(key), ptr(want), K, ptr(tile_min), ptr(idx),
                  ptr(score), ptr(n_cand))
        return idx, score, n_cand


def fanin_edges(idx):
    """edge_index int64 [2, E'] of decoded fan-in lists idx [N, K] (-1: no entry): sources on row 0, ordered by target, then by rank."""
    with torch.no_grad():
        N, K = idx.shape
        keep = (idx >= 0).flatten()
        dst = torch.arange(N, dtype=torch.int64, device=idx.device).repeat_interleave(K)[keep]
        return torch.stack([idx.flatten()[keep].to(torch.int64), dst])
