"""Cosine search on hf and candidate classes: unit rows, top-k, equivalence pairs, score profiles and the threshold search on
them, connected components and class tables.  Added functionality beside the train step: it depends on _hip and pairs only (ops
re-binds the public names; metrics builds on this module).
"""
import torch

from . import _hip
from ._hip import F32, I32, HipLibraryError, check, edge_rows, ptr
from .pairs import (PROFILE_MAX_EDGES, _count_scan_fill, _graph_of, _list_room, _list_rows, _pair_graphs, _pair_rows, _pair_width,
                    _profile_edges, counts_above, pair_scores_at, pair_topk)


# ------------------------------------------------------------------------------------------------
# functional-similarity search on hf (added functionality: the inference side of the functional loss, trainer.py:158-160)
# ------------------------------------------------------------------------------------------------
# Two facts for every function below.  Primary inputs and other never-updated nodes have hf = 0: their cosine is 0 with everything, so no
# positive threshold ever reports them.  Bit-identical or exactly power-of-two-scaled rows score within (2H + 6) 2^-24 of 1 and are not
# clamped to it: threshold = 1.0 selects nothing reliably, hence the default 0.999.
SIM_THRESHOLD = 0.999


def row_unit(x, eps=1e-8, want_norm=False):
    """y[i] = x[i] / max(|x[i]|, eps), the per-row clamp of torch.cosine_similarity and of the functional loss (trainer.py:158-160,
    mgv_func_loss_fwd); with want_norm also |x[i]| unclamped: (y, norm).  A zero row stays a zero row, a row with a NaN becomes NaN.
    The sum of squares is float32 without rescaling (hf is a GRU output in (-1, 1)).  No grad."""
    _pair_width(x, 'row_unit')
    with torch.no_grad():
        xd, ldx = _pair_rows(x, 'x')
        N, H = xd.shape
        y = torch.empty((N, H), dtype=F32, device=xd.device)
        norm = torch.empty(N, dtype=F32, device=xd.device) if want_norm else None
        _hip.call('mgv_row_unit', H, N, ptr(xd), ldx, float(eps), ptr(y), H, ptr(norm))
    return (y, norm) if want_norm else y


def sim_topk(x, k, graph_ptr=None, threshold=SIM_THRESHOLD, eps=1e-8):
    """(idx [N, k] int32, cos [N, k], n_above [N] int32): per row u the k nodes v != u of u's own graph with the largest cosine
    (ties: lower id first; -1 / -inf past the end), and the number of ALL candidates v != u whose cosine is > threshold (so n_above
    is symmetric).  A row needs all its candidates, so this is pair_topk on the unit rows; a cosine is the same bits as in sim_pairs
    and sim_at.  Zero rows (primary inputs) score 0 with everything; equal rows score within (2H + 6) 2^-24 of 1, not exactly 1."""
    y = row_unit(x, eps)
    with torch.no_grad():
        return pair_topk(y, y, k, graph_ptr=graph_ptr, sigmoid=False, threshold=threshold, skip_self=True)


def _sim_room(total, with_scores, max_pairs, free):
    """sim_pairs' refusals: int64 pair_index, the int32 list it is made from, float32 scores when asked for."""
    _list_room('sim_pairs', total, free, noun='pairs', listed='%d pairs', limit_name='max_pairs', limit=max_pairs,
               item_bytes=24 if with_scores else 20,
               hint='raise the threshold, or take the k most similar gates per node with ops.sim_topk / similar_gates')


def sim_pairs(x, graph_ptr=None, threshold=SIM_THRESHOLD, with_scores=False, max_pairs=None, eps=1e-8):
    """(pair_index int64 [2, P] with pair_index[0] < pair_index[1], row_ptr int64 [N + 1], score [P] or None): every unordered pair of
    nodes of one graph whose cosine is > threshold, once, ordered by the smaller id and then the larger — the candidates for SAT
    sweeping and equivalence checking.  Unit rows, then the symmetric selection (mgv_sim_select_*: half the tiles of pair_select on
    the same rows): count, exclusive int64 scan, ONE read-back of the total, fill; nothing of size N^2, no atomics.  A total above
    `max_pairs` or beyond the free memory raises HipLibraryError before anything is allocated or filled.  Zero rows (primary inputs)
    pair with nothing at a positive threshold; threshold = 1.0 selects nothing reliably (equal rows score within (2H + 6) 2^-24 of 1)."""
    y = row_unit(x, eps)
    with torch.no_grad():
        N, H = y.shape
        dev = y.device
        gp, G = _pair_graphs(graph_ptr, dev)
        common = (H, N, ptr(y), H, ptr(gp), G, float(threshold))
        row_ptr, col, score = _count_scan_fill('mgv_sim_select_count', 'mgv_sim_select_fill', N, common, dev, with_scores,
                                               lambda total, free: _sim_room(total, with_scores, max_pairs, free))
        rows = _list_rows(row_ptr, col.numel())
        return torch.stack([rows, col.to(torch.int64)]), row_ptr, score


def sim_at(x, pair_index, eps=1e-8):
    """cos(x[a], x[b]) of the listed pairs [2, P], the cosine of the functional loss (1 - sim_at is its `dis`, trainer.py:158-160) in
    the arithmetic of sim_topk and sim_pairs: the same bits for the same pair."""
    y = row_unit(x, eps)
    with torch.no_grad():
        return pair_scores_at(y, y, pair_index, sigmoid=False)


# ------------------------------------------------------------------------------------------------
# the distribution of all-pair cosines (added functionality: thresholds chosen by count; mgv_sim_hist) and the threshold search on it
# ------------------------------------------------------------------------------------------------
def _unit_profile(y, e, graph_ptr):
    """mgv_sim_hist on unit rows y and a device table e -> int64 [G, B + 1]."""
    N, H = y.shape
    gp, G = _pair_graphs(graph_ptr, y.device)
    hist = torch.empty((max(G, 1), e.numel() + 1), dtype=torch.int64, device=y.device)
    _hip.call('mgv_sim_hist', H, N, ptr(y), H, ptr(gp), G, ptr(e), e.numel(), ptr(hist))
    return hist if gp is None else hist[:G]


def sim_profile(x, edges, graph_ptr=None, eps=1e-8):
    """int64 [G, B + 1]: pair_profile's bins for the cosine of sim_pairs — unit rows (row_unit), every unordered pair of one graph once
    (v > u), half the tiles (mgv_sim_hist).  counts_above(profile)[g, j] is the number of pairs sim_pairs lists for graph g at
    threshold edges[j], as integers.  Zero rows (primary inputs) score 0 with everything; equal rows score within (2H + 6) 2^-24 of
    1, not exactly 1."""
    _pair_width(x, 'sim_profile')
    y = row_unit(x, eps)
    with torch.no_grad():
        return _unit_profile(y, _profile_edges(edges, y.device), graph_ptr)


def _f32(v):
    return float(torch.tensor(float(v), dtype=F32))


def _f32_key(v):
    """The place of float32(v) in the order of all float32 values, as an integer: adjacent floats differ by 1, -0.0 and 0.0 are both 0."""
    bits = int(torch.tensor(float(v), dtype=F32).view(I32))
    return bits if bits >= 0 else -(bits & 0x7fffffff)


def _edges_between(lo, hi, bins):
    """min(bins, all) distinct float32 values across [lo, hi], both ends included, ascending, evenly spaced in the ORDER of the float32
    values (linear inside a binade, geometric across binades): a bracket of at most 2^32 floats shrinks by bins - 1 per round, so six
    rounds of 64 edges reach adjacent floats from any start."""
    a, b = _f32_key(lo), _f32_key(hi)
    n = max(min(int(bins), b - a + 1), 1)
    ks = a + (torch.arange(n, dtype=torch.int64) * (b - a)) // max(n - 1, 1)
    return torch.where(ks >= 0, ks, -ks - (1 << 31)).to(I32).view(F32)


def threshold_search(profile_fn, max_pairs, lo=0.0, hi=2.0, bins=64, max_rounds=6):
    """The bracket logic of sim_threshold_for on any walk: profile_fn(edges float32 [B], ascending) -> int64 [G, B + 1].  The bracket
    (lower, threshold] always has count(lower) > max_pairs >= count(threshold) with both counts taken from a walk; count(hi) must
    be 0 <= max_pairs for the caller's `hi`.  -> the dict of sim_threshold_for."""
    max_pairs = int(max_pairs)
    if max_pairs < 0:
        raise HipLibraryError('max_pairs must be >= 0 (got %d)' % max_pairs)
    bins = min(max(int(bins), 3), PROFILE_MAX_EDGES)
    lower, upper, pairs_lower, pairs, tight = _f32(lo), _f32(hi), None, None, False
    if not lower < upper:
        raise HipLibraryError('the search needs lo < %g (got %g)' % (upper, lower))
    for rnd in range(max(int(max_rounds), 1)):
        e = _edges_between(lower, upper, bins)
        above = counts_above(profile_fn(e)).sum(0).tolist()           # the round's ONE read-back: batch-wide pairs above each edge
        ev = e.tolist()
        j = next((i for i, n in enumerate(above) if n <= max_pairs), None)      # the count falls along the table
        if j is None:
            raise HipLibraryError('%d pairs are above %g, the upper end of the search: more than max_pairs = %d' % (above[-1], ev[-1], max_pairs))
        if j == 0:                                                     # only in the first round: the count at lo already fits
            return {'threshold': ev[0], 'pairs': above[0], 'lower': None, 'pairs_lower': None, 'tight': True}
        lower, pairs_lower, upper, pairs = ev[j - 1], above[j - 1], ev[j], above[j]
        tight = _f32_key(upper) - _f32_key(lower) <= 1                 # no float32 strictly between the two ends
        if tight:
            break
    return {'threshold': upper, 'pairs': pairs, 'lower': lower, 'pairs_lower': pairs_lower, 'tight': tight}


def sim_threshold_for(x, max_pairs, graph_ptr=None, lo=0.0, bins=64, max_rounds=6, eps=1e-8):
    """The lowest cosine threshold whose batch-wide pair count fits `max_pairs`, from the distribution instead of trial walks:
    {'threshold' (a Python float holding a float32 value), 'pairs', 'lower', 'pairs_lower', 'tight'}.  pairs <= max_pairs and pairs is
    the total sim_pairs lists at `threshold`; when `lower` is not None it is the bracket's other end, lower < threshold with
    pairs_lower > max_pairs.  The bracket starts as (lo, 2.0] — no cosine exceeds 1 + (2H + 6) 2^-24, so nothing is above 2.0 — and
    each round puts `bins` distinct float32 edges across it, both ends included, takes ONE sim_profile walk and ONE read-back, and
    keeps the adjacent pair of edges between which the count crosses max_pairs; it stops when no float32 lies strictly between the
    two ends (tight) or after max_rounds.  If the count at `lo` already fits, the result is lo with lower = None.
    Ties are the caller's to understand: 5,000 equal gates are 12.5 M pairs at ONE cosine value, which a threshold takes or leaves
    as a whole, so the tight answer can lie far below max_pairs.  Zero rows score 0 with everything and never pass a threshold
    >= 0; equal rows score within (2H + 6) 2^-24 of 1."""
    _pair_width(x, 'sim_threshold_for')
    y = row_unit(x, eps)
    with torch.no_grad():
        return threshold_search(lambda e: _unit_profile(y, _profile_edges(e, y.device), graph_ptr), max_pairs, lo=lo, hi=2.0, bins=bins,
                                max_rounds=max_rounds)


# ------------------------------------------------------------------------------------------------
# connected components and candidate classes (added functionality: csrc/components.hip, csrc/mgv_unionfind.h)
# ------------------------------------------------------------------------------------------------
_CC_ERR = {1: 'an entry of the forest outside [0, x] (parent was not initialised)', 2: 'a union-find loop reached its cap of 2^20 rounds',
           3: 'a listed node id outside [0, N)'}


def _cc_status(name, st):
    """st = the four ints of the union-find's status record, already on the host."""
    if st[0] != 0:
        raise HipLibraryError('%s: the union-find reported an error: %s (code %d, a = %d, b = %d, rounds = %d)'
                              % (name, _CC_ERR.get(st[0], 'unknown'), st[0], st[1], st[2], st[3]))


def _cc_forest(N, dev):
    if N >= 2 ** 31:
        raise HipLibraryError('components: node ids are int32, N = %d is beyond them' % N)
    parent = torch.empty(N, dtype=I32, device=dev)
    status = torch.empty(4, dtype=I32, device=dev)
    _hip.call('mgv_cc_init', N, ptr(parent), ptr(status))
    return parent, status


def _cc_labels(N, parent):
    label = torch.empty(N, dtype=I32, device=parent.device)
    _hip.call('mgv_cc_labels', N, ptr(parent), ptr(label), None)      # sizes come with the class table
    return label


def _cc_from_pairs(pair_index, N):
    """(label, status) of the pair list's components; status is still on the device."""
    a, b = edge_rows(pair_index)
    parent, status = _cc_forest(N, pair_index.device)
    _hip.call('mgv_cc_union_pairs', N, a.numel(), ptr(a), ptr(b), ptr(parent), ptr(status))
    return _cc_labels(N, parent), status


def _min_size(min_size):
    if int(min_size) != min_size or int(min_size) < 1:
        raise HipLibraryError('min_size must be an integer >= 1 (1 lists every node, singletons included), got %r' % (min_size,))
    return int(min_size)


def components(pair_index, N):
    """label int32 [N]: the connected components of the undirected graph on nodes 0 .. N - 1 whose edges are the columns of pair_index
    (int64 [2, P], P = 0 included; any order and orientation, duplicates and a == a allowed) — label[i] is the smallest id of i's
    component, so label[i] == i marks a component's representative and an untouched node is its own.  A concurrent union-find on the
    device in which a root is only ever hooked under a smaller root: exact, and the same bits from run to run.  For lists from
    sim_pairs / equivalence_candidates (candidate classes) and from reconstruct_edges (components of the decoded graph,
    digae_layer.py:31-33) alike.  One synchronisation: the union-find's status record is read back, and anything in it (an id outside
    [0, N)) raises HipLibraryError.  No grad."""
    N = int(N)
    if N < 0:
        raise HipLibraryError('components: N must be >= 0, got %d' % N)
    if not (torch.is_tensor(pair_index) and pair_index.dim() == 2 and pair_index.shape[0] == 2):
        raise HipLibraryError('components: pair_index must be an int64 tensor [2, P]')
    if not pair_index.is_cuda:
        raise HipLibraryError('pair_index must live on the GPU (got %s); the hot path has no CPU implementation' % pair_index.device)
    if pair_index.dtype != torch.int64:
        raise HipLibraryError('pair_index must be torch.int64 (got %s)' % pair_index.dtype)
    with torch.no_grad():
        label, status = _cc_from_pairs(pair_index, N)
        _cc_status('components', status.tolist())             # the read-back
    return label


def _class_table(label, min_size, status, name):
    N, dev = label.numel(), label.device
    ws_ints = _hip.call_value('mgv_cc_class_ws_ints', N)
    if ws_ints < 0:
        raise HipLibraryError('%s: MGV_EUNSUPPORTED (unsupported size): N = %d' % (name, N))
    ws = torch.empty(ws_ints, dtype=I32, device=dev)
    counts = torch.empty(6, dtype=I32, device=dev)
    _hip.call('mgv_cc_class_count', N, ptr(label), min_size, ptr(status), ptr(ws), ws_ints, ptr(counts))
    got = counts.tolist()                                     # the read-back: C, M and the status record
    _cc_status(name, got[2:])
    C, M = got[0], got[1]
    class_ptr = torch.empty(C + 1, dtype=torch.int64, device=dev)
    members = torch.empty(M, dtype=I32, device=dev)
    temp_ints = _hip.call_value('mgv_sort_pairs_temp_ints', 4, max(M, 1))
    temp = torch.empty(max(temp_ints, 1), dtype=I32, device=dev)
    _hip.call('mgv_cc_class_fill', N, ptr(label), C, M, ptr(ws), ws_ints, ptr(temp), temp_ints, ptr(class_ptr), ptr(members))
    return class_ptr, members


def class_table(label, min_size=2):
    """(class_ptr int64 [C + 1], members int32 [M]): the classes of `label` (int32 [N] as components / sim_classes return it) with at
    least min_size members, as one compact table.  Classes come in the order of their labels and members ascend inside a class, so
    members[class_ptr[c]] is class c's label (its smallest id, the natural representative) and members[class_ptr[c] : class_ptr[c + 1]]
    the whole class.  min_size = 2 leaves the singletons out; 1 lists every node.  Sizes, two scans and a stable sort by label on the
    device with ONE read-back (C and M: the result must be allocated).  No grad."""
    min_size = _min_size(min_size)
    check(label, I32, 'label')
    if label.dim() != 1:
        raise HipLibraryError('class_table: label must be int32 [N]')
    with torch.no_grad():
        return _class_table(label, min_size, None, 'class_table')


def sim_classes(x, graph_ptr=None, threshold=SIM_THRESHOLD, min_size=2, route='walk', eps=1e-8, max_pairs=None):
    """(label int32 [N], class_ptr int64 [C + 1], members int32 [M]): the candidate classes a SAT sweeper consumes — the connected
    components of the relation "same graph and cosine > threshold" on the rows of x (hf), as components' labels (label[i] = the
    smallest id of i's class) and class_table's table of the classes with at least min_size members.
    The classes are SINGLE-LINKAGE components of the thresholded relation: two members of one class can have a cosine below the
    threshold (a chain of close neighbours links them); every member has at least one other member above it.  Primary inputs
    (hf = 0: cosine 0 with everything) and rows that hold a NaN are always singletons at a positive threshold.  Classes never cross
    graphs (graph_ptr [G + 1]; None: one graph).  threshold = 1.0 is unreliable: equal rows score within (2H + 6) 2^-24 of 1, not
    exactly 1, hence the default 0.999.
    route='walk': the symmetric tile walk of sim_pairs unites each pair where it finds it (mgv_sim_union).  No pair list ever exists:
    memory is O(N) and nothing is refused for size — 5,000 equal gates are 12.5 M pairs but one class of 5,000.
    route='pairs': sim_pairs followed by components; it keeps sim_pairs' refusals (max_pairs, free memory).
    Both routes give the same labels, exactly, and the same bits from run to run.  Unit rows come from row_unit.  One read-back (the
    table's two sizes and the union-find's status record) besides the two ends of a graph_ptr.  No grad."""
    if route not in ('walk', 'pairs'):
        raise HipLibraryError("sim_classes: route must be 'walk' (classes straight from the tile walk) or 'pairs' (sim_pairs, then "
                              "components), got %r" % (route,))
    min_size = _min_size(min_size)
    if route == 'walk' and max_pairs is not None:
        raise HipLibraryError("sim_classes: max_pairs belongs to route='pairs'; the walk holds no pair list")
    if route == 'pairs':
        pi, _, _ = sim_pairs(x, graph_ptr=graph_ptr, threshold=threshold, max_pairs=max_pairs, eps=eps)
        with torch.no_grad():
            label, status = _cc_from_pairs(pi, x.shape[0])
            return (label,) + _class_table(label, min_size, status, 'sim_classes')
    y = row_unit(x, eps)
    with torch.no_grad():
        N, H = y.shape
        gp, G = _pair_graphs(graph_ptr, y.device)
        parent, status = _cc_forest(N, y.device)
        _hip.call('mgv_sim_union', H, N, ptr(y), H, ptr(gp), G, float(threshold), ptr(parent), ptr(status))
        label = _cc_labels(N, parent)
        return (label,) + _class_table(label, min_size, status, 'sim_classes')


# ------------------------------------------------------------------------------------------------
# matching across circuits (added functionality: mgv_cross_topk / mgv_cross_select_*; a golden design against its revision)
# ------------------------------------------------------------------------------------------------
# hf depends only on a circuit's own structure and one model embeds every circuit of a batch, so rows of different graphs are comparable
# as they stand.  `peer` [G] says who is a candidate: the candidates of a row of graph g are ALL rows of graph peer[g]; -1: none;
# peer[g] = g: the row's own graph, itself included (there is no skip_self here); it need not be an involution, and several graphs may
# name one peer (ten revisions against one golden design).  The two facts at the head of this file hold here too.
def _peer_table(peer, graph_ptr, name):
    """(graph_ptr int32 [G + 1], peer int32 [G]) on the HOST, checked before anything touches the device: peer needs a graph_ptr
    (HipLibraryError), has one integer per graph and every entry in [-1, G) (ValueError).  A table that lives on the device is read
    back for this."""
    if graph_ptr is None:
        raise HipLibraryError('%s: peer names graphs, so it needs graph_ptr [G + 1] (got None)' % name)
    gp = torch.as_tensor(graph_ptr).detach().cpu().flatten()
    if gp.numel() < 1:
        raise HipLibraryError('graph_ptr needs at least one entry')
    G = gp.numel() - 1
    p = torch.as_tensor(peer).detach().cpu()
    if p.numel() and (p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool):     # ([] is a float tensor)
        raise ValueError('%s: peer must hold integers, one graph index per graph (got %s)' % (name, p.dtype))
    if p.dim() != 1 or p.numel() != G:
        raise ValueError('%s: peer must have one entry per graph, [%d] (got shape %s)' % (name, G, tuple(p.shape)))
    if G and (int(p.min()) < -1 or int(p.max()) >= G):
        raise ValueError('%s: every entry of peer must be -1 (no candidates) or a graph index in [0, %d) (got %d .. %d)'
                         % (name, G, int(p.min()), int(p.max())))
    return gp.to(I32), p.to(I32)


def cross_topk(x, k, graph_ptr, peer, threshold=SIM_THRESHOLD, eps=1e-8):
    """(idx [N, k] int32, cos [N, k], n_above [N] int32): per row u of graph g the k rows of graph peer[g] with the largest cosine
    (batch-wide ids; ties: lower id first; -1 / -inf past the end, and everywhere when peer[g] = -1) and the number of ALL rows of
    peer[g] whose cosine is > threshold.  mgv_cross_topk on the unit rows: a cosine is the same bits as in cross_pairs and sim_at; a
    row tile walks only the column tiles that hold one of its rows' candidates.  Nothing is read back except graph_ptr's two ends and
    peer, which the launcher checks.  No grad."""
    gph, ph = _peer_table(peer, graph_ptr, 'cross_topk')
    y = row_unit(x, eps)
    with torch.no_grad():
        N, H = y.shape
        dev = y.device
        gp, pr, G = gph.to(dev), ph.to(dev), ph.numel()
        k = int(k)
        kk = min(max(k, 1), 32)
        idx = torch.empty((N, kk), dtype=I32, device=dev)
        cos = torch.empty((N, kk), dtype=F32, device=dev)
        n_above = torch.empty(N, dtype=I32, device=dev)
        _hip.call('mgv_cross_topk', H, N, ptr(y), H, ptr(gp), G, ptr(pr), k, float(threshold), ptr(idx), ptr(cos), ptr(n_above))
        return idx, cos, n_above


def _cross_room(total, with_scores, max_pairs, free):
    """cross_pairs' refusals, as _sim_room."""
    _list_room('cross_pairs', total, free, noun='pairs', listed='%d pairs', limit_name='max_pairs', limit=max_pairs,
               item_bytes=24 if with_scores else 20,
               hint='raise the threshold, or take the k best matches per gate with ops.cross_topk / match_gates')


def cross_pairs(x, graph_ptr, peer, threshold=SIM_THRESHOLD, with_scores=False, max_pairs=None, eps=1e-8):
    """(pair_index int64 [2, P], row_ptr int64 [N + 1], score [P] or None): pair_index[0] is a row u, pair_index[1] a row v of the peer
    of u's graph with cosine > threshold; ordered by u and then v, row_ptr delimits the rows' lists.  With an involutive peer
    (peer[peer[g]] = g) a pair appears ONCE FROM EACH SIDE, as (u, v) in u's list and as (v, u) in v's, with the same bits.
    mgv_cross_select_*: count, exclusive int64 scan, ONE read-back of the total (the result must be allocated: the synchronisation
    cross_topk does not have), fill; nothing of size N^2, no atomics, the same bytes from call to call.  A total above `max_pairs` or
    beyond the free memory raises HipLibraryError before anything is allocated or filled.  No grad."""
    gph, ph = _peer_table(peer, graph_ptr, 'cross_pairs')
    y = row_unit(x, eps)
    with torch.no_grad():
        N, H = y.shape
        dev = y.device
        gp, pr, G = gph.to(dev), ph.to(dev), ph.numel()
        common = (H, N, ptr(y), H, ptr(gp), G, ptr(pr), float(threshold))
        row_ptr, col, score = _count_scan_fill('mgv_cross_select_count', 'mgv_cross_select_fill', N, common, dev, with_scores,
                                               lambda total, free: _cross_room(total, with_scores, max_pairs, free))
        rows = _list_rows(row_ptr, col.numel())
        return torch.stack([rows, col.to(torch.int64)]), row_ptr, score


def cross_mutual(x, graph_ptr, peer, threshold=SIM_THRESHOLD, eps=1e-8):
    """(pair_index int64 [2, M], cos [M]): the reciprocal best matches — the pairs (u, v) where v is u's top-1 in the peer of u's graph,
    u is v's top-1 in the peer of v's graph and the cosine is > threshold — each once, with u in the lower-indexed graph (u <= v
    inside a graph that is its own peer), ordered by u.  Defined only where peer[peer[g]] = g: graphs where that fails contribute
    nothing.  From ONE cross_topk with k = 1 and device torch ops; a tie for a row's top-1 goes to the lower id, as there."""
    gph, ph = _peer_table(peer, graph_ptr, 'cross_mutual')
    idx, cos, _ = cross_topk(x, 1, gph, ph, threshold=threshold, eps=eps)
    with torch.no_grad():
        dev = idx.device
        N, G = idx.shape[0], ph.numel()
        if N == 0 or G == 0:
            return torch.zeros((2, 0), dtype=torch.int64, device=dev), torch.zeros(0, dtype=F32, device=dev)
        pl = ph.to(torch.int64)
        inv = (pl >= 0) & (pl[pl.clamp(min=0)] == torch.arange(G))          # peer[peer[g]] == g
        u = torch.arange(N, dtype=torch.int64, device=dev)
        v = idx[:, 0].to(torch.int64)
        back = idx[v.clamp(min=0), 0].to(torch.int64)
        gid = _graph_of(torch.cat([u, v.clamp(min=0)]), gph.to(device=dev, dtype=torch.int64), G)
        gu, gv = gid[:N], gid[N:]
        keep = (v >= 0) & (back == u) & (cos[:, 0] > threshold) & inv.to(dev)[gu] & ((gu < gv) | ((gu == gv) & (u <= v)))
        return torch.stack([u[keep], v[keep]]), cos[keep, 0]


def cross_classes(x, graph_ptr, peer, threshold=SIM_THRESHOLD, min_size=2, max_pairs=None, eps=1e-8, route='pairs'):
    """(label int32 [N], class_ptr int64 [C + 1], members int32 [M]) as sim_classes returns them: the connected components of
    "cosine > threshold" over the cross pairs (cross_pairs) TOGETHER WITH the within-circuit pairs (sim_pairs), so a class may now
    span a graph and its peer — and nothing else: two graphs share a class only through a chain of peer links (several graphs that
    name one peer can meet in it).  Single linkage, as sim_classes.
    route='pairs' (the default): components and class_table on the two lists; each list keeps its refusals (max_pairs applies to
    each, free memory).
    route='walk': one forest, on which the symmetric walk of sim_pairs (mgv_sim_union) and then the cross walk of cross_pairs
    (mgv_cross_union) unite each pair where they find it.  No pair list ever exists: memory is O(N) and nothing is refused for size —
    a revision that keeps 5,000 equal gates of its golden design is 25 M cross pairs (50 M with an involutive peer) but one class of
    10,000.  max_pairs belongs to route='pairs'.  One read-back (the table's two sizes and the union-find's status record) besides
    graph_ptr's two ends and peer, which the launchers check.
    Both routes give the same three tensors, exactly, and the same bits from run to run.  No grad."""
    if route not in ('walk', 'pairs'):
        raise HipLibraryError("cross_classes: route must be 'pairs' (cross_pairs and sim_pairs, then components) or 'walk' (classes "
                              "straight from the two tile walks), got %r" % (route,))
    min_size = _min_size(min_size)
    if route == 'walk' and max_pairs is not None:
        raise HipLibraryError("cross_classes: max_pairs belongs to route='pairs'; the walk holds no pair list")
    gph, ph = _peer_table(peer, graph_ptr, 'cross_classes')
    if route == 'walk':
        y = row_unit(x, eps)
        with torch.no_grad():
            N, H = y.shape
            dev = y.device
            gp, pr, G = gph.to(dev), ph.to(dev), ph.numel()
            parent, status = _cc_forest(N, dev)
            _hip.call('mgv_sim_union', H, N, ptr(y), H, ptr(gp), G, float(threshold), ptr(parent), ptr(status))
            _hip.call('mgv_cross_union', H, N, ptr(y), H, ptr(gp), G, ptr(pr), float(threshold), ptr(parent), ptr(status))
            label = _cc_labels(N, parent)
            return (label,) + _class_table(label, min_size, status, 'cross_classes')
    cross, _, _ = cross_pairs(x, gph, ph, threshold=threshold, max_pairs=max_pairs, eps=eps)
    own, _, _ = sim_pairs(x, graph_ptr=gph, threshold=threshold, max_pairs=max_pairs, eps=eps)
    with torch.no_grad():
        label, status = _cc_from_pairs(torch.cat([cross, own], dim=1), x.shape[0])
        return (label,) + _class_table(label, min_size, status, 'cross_classes')


# the distribution of cross cosines (mgv_cross_hist) and the threshold search on it
def _cross_unit_profile(y, e, gp, pr):
    """mgv_cross_hist on unit rows y, a device table e and the device tables gp [G + 1], pr [G] -> int64 [G, B + 1]."""
    N, H = y.shape
    G = pr.numel()
    hist = torch.empty((max(G, 1), e.numel() + 1), dtype=torch.int64, device=y.device)      # never a NULL pointer
    _hip.call('mgv_cross_hist', H, N, ptr(y), H, ptr(gp), G, ptr(pr), ptr(e), e.numel(), ptr(hist))
    return hist[:G]


def cross_profile(x, edges, graph_ptr, peer, eps=1e-8):
    """int64 [G, B + 1]: sim_profile's bins for the cosines of cross_pairs — unit rows (row_unit), every (row u of graph g, row v of
    graph peer[g]), binned by the number of `edges` (strictly ascending, at most 256) the cosine is above, in row g (mgv_cross_hist:
    ONE walk for all edges).  counts_above(profile)[g, j] is the number of pairs cross_pairs lists for the rows of graph g at
    threshold edges[j], as integers; with an involutive peer a pair is counted once from each side, in g's row and in its peer's.
    A graph with peer = -1 or without rows has a zero row; a NaN is counted nowhere.  No grad."""
    gph, ph = _peer_table(peer, graph_ptr, 'cross_profile')
    _pair_width(x, 'cross_profile')
    y = row_unit(x, eps)
    with torch.no_grad():
        return _cross_unit_profile(y, _profile_edges(edges, y.device), gph.to(y.device), ph.to(y.device))


def cross_threshold_for(x, max_pairs, graph_ptr, peer, lo=0.0, bins=64, max_rounds=6, eps=1e-8):
    """sim_threshold_for across circuits: the lowest cosine threshold whose batch-wide count of cross pairs fits `max_pairs`, from the
    distribution (cross_profile walks) instead of trial count walks -> the dict of sim_threshold_for, {'threshold', 'pairs', 'lower',
    'pairs_lower', 'tight'}.  "Pairs" are the entries of cross_pairs' lists, summed over all rows: pairs is exactly
    cross_pairs(threshold=result['threshold'])[0].shape[1], so with an involutive peer a pair counts ONCE FROM EACH SIDE (twice), and
    a self-peer counts (u, v), (v, u) and (u, u).  The bracket, the rounds, `tight` and what ties do are threshold_search's and
    sim_threshold_for's: one walk and one read-back per round.  No grad."""
    gph, ph = _peer_table(peer, graph_ptr, 'cross_threshold_for')
    _pair_width(x, 'cross_threshold_for')
    y = row_unit(x, eps)
    with torch.no_grad():
        gp, pr = gph.to(y.device), ph.to(y.device)
        return threshold_search(lambda e: _cross_unit_profile(y, _profile_edges(e, y.device), gp, pr), max_pairs, lo=lo, hi=2.0, bins=bins,
                                max_rounds=max_rounds)
