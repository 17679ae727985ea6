"""Host references for the connected-components entries (csrc/components.hip: mgv_cc_init, mgv_cc_union_pairs, mgv_cc_labels,
mgv_cc_class_count / mgv_cc_class_fill; csrc/pair_scores.hip: mgv_sim_union), the checker the device tests use, the seeded case
builders, and the device's hook restated in Python with planted defects.  CPU only; pinned by tests/test_components_spec.py.

Everything here is integer work: the device's labels, sizes and tables are compared EXACTLY.  A label is the smallest id of a node's
component.  Three independent labellings (a union-find, a breadth-first search, a vectorised min-label propagation for the large
forest) must agree before any of them is used as a yardstick.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import pair_scores_ref as PR  # noqa: E402

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
GRID_CAP_THREADS = 2048 * 256            # mgv::grid_for(.., 8) x 256 threads: one pair (or node) per thread up to here, then strides
SIM_THR = 0.999


# ------------------------------------------------------------------------------------------------ three labellings
def _np_pairs(pairs):
    p = pairs.numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
    return p.reshape(2, -1).astype(np.int64)


def uf_labels(pairs, N):
    """A plain union-find (the smaller root wins, full compression at the end) -> int64 [N]."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    a, b = _np_pairs(pairs).tolist()
    for u, v in zip(a, b):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return torch.tensor([find(i) for i in range(N)], dtype=I64)


def bfs_labels(pairs, N):
    """Adjacency lists and a breadth-first search from every unlabelled node in ascending order -> int64 [N]."""
    adj = [[] for _ in range(N)]
    a, b = _np_pairs(pairs).tolist()
    for u, v in zip(a, b):
        adj[u].append(v)
        adj[v].append(u)
    label = [-1] * N
    for s in range(N):
        if label[s] >= 0:
            continue
        label[s] = s
        todo = [s]
        while todo:
            nxt = []
            for u in todo:
                for v in adj[u]:
                    if label[v] < 0:
                        label[v] = s
                        nxt.append(v)
            todo = nxt
    return torch.tensor(label, dtype=I64)


def propagate_labels(pairs, N):
    """Min-label propagation with pointer jumping, vectorised (for the forest of a million pairs) -> int64 [N]."""
    a, b = _np_pairs(pairs)
    label = np.arange(N, dtype=np.int64)
    while True:
        m = np.minimum(label[a], label[b])
        new = label.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, label):
            return torch.from_numpy(label)
        label = new


def sizes_ref(label):
    """size[r] = number of nodes labelled r (0 where r is no label) -> int64 [N]."""
    return torch.bincount(label.to(I64), minlength=label.numel())


def class_table_ref(label, min_size=2):
    """(class_ptr int64 [C + 1], members int64 [M]): classes of at least min_size in label order, members ascending."""
    label = label.to(I64)
    size = sizes_ref(label)
    ptr, members = [0], []
    for r in torch.nonzero(size >= min_size).flatten().tolist():
        m = torch.nonzero(label == r).flatten().tolist()
        members += m
        ptr.append(len(members))
    return torch.tensor(ptr, dtype=I64), torch.tensor(members, dtype=I64)


def class_table_sorted(label, min_size=2):
    """The same table from a stable sort of the selected nodes by label (for labellings too large for class_table_ref's loop)."""
    lab = label.to(I64).numpy()
    size = np.bincount(lab, minlength=lab.size)
    ids = np.nonzero(size[lab] >= min_size)[0]
    members = ids[np.argsort(lab[ids], kind='stable')]
    roots = np.nonzero(size >= min_size)[0]
    ptr = np.concatenate([[0], np.cumsum(size[roots])]).astype(np.int64)
    return torch.from_numpy(ptr), torch.from_numpy(members.astype(np.int64))


def check_components(label, size, want):
    """The checker of the device tests: findings (strings) of a device result against a reference labelling `want`.  label / size as
    mgv_cc_labels wrote them (size may be None)."""
    bad = []
    label, want = label.to(I64).flatten().cpu(), want.to(I64)
    N = want.numel()
    if label.numel() != N:
        return ['%d labels for %d nodes' % (label.numel(), N)]
    if N and not bool(((label >= 0) & (label <= torch.arange(N))).all()):
        bad.append('a label outside [0, i]')
    elif N and not torch.equal(label[label], label):
        bad.append('a label that is not its own label (no root)')
    if not torch.equal(label, want):
        d = torch.nonzero(label != want).flatten()
        bad.append('%d labels differ from the reference, first at node %d: %d, reference %d'
                   % (d.numel(), int(d[0]), int(label[d[0]]), int(want[d[0]])))
    if size is not None:
        size = size.to(I64).flatten().cpu()
        if not torch.equal(size, sizes_ref(want)):
            bad.append('the sizes are not the reference\'s')
    return bad


def check_table(class_ptr, members, label, min_size):
    """Exact against class_table_ref, and the invariants a user relies on."""
    bad = []
    class_ptr, members = class_ptr.to(I64).flatten().cpu(), members.to(I64).flatten().cpu()
    rp, rm = class_table_ref(label, min_size) if label.numel() <= 10000 else class_table_sorted(label, min_size)
    if not torch.equal(class_ptr, rp):
        bad.append('class_ptr differs from the reference (%d against %d classes)' % (class_ptr.numel() - 1, rp.numel() - 1))
    if not torch.equal(members, rm):
        bad.append('members differ from the reference (%d against %d)' % (members.numel(), rm.numel()))
    if not bad:
        lab = label.to(I64)
        for c in range(min(class_ptr.numel() - 1, 2000)):
            m = members[int(class_ptr[c]):int(class_ptr[c + 1])]
            if not (int(m[0]) == int(lab[m[0]]) and bool((lab[m] == m[0]).all()) and bool((m[1:] > m[:-1]).all()) and m.numel() >= min_size):
                bad.append('class %d: first member is not the label, or members do not ascend' % c)
    return bad


# ------------------------------------------------------------------------------------------------ pair-list builders (seeded)
def _case(pairs, N):
    return {'pairs': torch.as_tensor(np.asarray(pairs, dtype=np.int64).reshape(2, -1)), 'N': N}


ORDERS = ('ascending', 'descending', 'shuffled', 'bit-reversed')


def path(n, order):
    """The path 0 - 1 - ... - (n - 1), its n - 1 pairs listed in one of ORDERS."""
    assert order in ORDERS
    i = np.arange(n - 1, dtype=np.int64)
    if order == 'descending':
        i = i[::-1].copy()
    elif order == 'shuffled':
        i = np.random.default_rng(n).permutation(i)
    elif order == 'bit-reversed':
        bits = max(1, int(n - 2).bit_length())
        rev = np.array([int(format(int(k), '0%db' % bits)[::-1], 2) for k in i])
        i = i[np.argsort(rev, kind='stable')]
    return _case([i, i + 1], n)


def star(leaves, centre_first):
    """leaves + 1 nodes, every leaf paired with the centre: id 0 (the final root from the start) or id N - 1 (the centre is hooked
    first and every later pair meets a moved root)."""
    N = leaves + 1
    c = 0 if centre_first else N - 1
    leaf = np.arange(1, N) if centre_first else np.arange(0, N - 1)
    return _case([np.full(leaves, c), leaf], N)


def two_paths_joined_last(n):
    """Paths 0 .. n - 1 and n .. 2 n - 1, and as the very last pair their far ends (2 n - 1, n - 1)."""
    i = np.arange(n - 1, dtype=np.int64)
    return _case([np.concatenate([i, i + n, [2 * n - 1]]), np.concatenate([i + 1, i + n + 1, [n - 1]])], 2 * n)


def clique(n=64):
    """All n (n - 1) / 2 pairs, larger id first: every thread contends for one root."""
    a, b = np.triu_indices(n, 1)
    return _case([b, a], n)


def forest(N, P, seed):
    """P random pairs, each inside one block of 32 consecutive ids: about N / 32 components, isolated nodes among them."""
    g = np.random.default_rng(seed)
    a = g.integers(0, N, P)
    b = np.minimum(a // 32 * 32 + g.integers(0, 32, P), N - 1)
    return _case([a, b], N)


def with_noise(case, seed=0):
    """The same components from a noisier list: every third pair twice, every second pair flipped, a == a pairs, shuffled."""
    p = case['pairs'].numpy()
    g = np.random.default_rng(seed + 17)
    dup = p[:, ::3]
    same = g.integers(0, case['N'], max(3, p.shape[1] // 5))
    q = np.concatenate([p, dup, np.stack([same, same])], axis=1)
    flip = g.random(q.shape[1]) < 0.5
    q[:, flip] = q[::-1, flip]
    return _case(q[:, g.permutation(q.shape[1])], case['N'])


def list_cases():
    """name -> case, everything the list test runs except the large forest."""
    out = {'P=0': _case([[], []], 37), 'N=1': _case([[], []], 1), 'N=1 self': _case([[0], [0]], 1)}
    for o in ORDERS:
        out['path 4097 ' + o] = path(4097, o)
    out['star centre 0'] = star(1100, True)
    out['star centre N-1'] = star(1100, False)
    out['two paths joined last'] = two_paths_joined_last(700)
    out['clique 64'] = clique(64)
    for k in ('path 4097 shuffled', 'star centre N-1', 'clique 64', 'two paths joined last'):
        out[k + ' + noise'] = with_noise(out[k])
    return out


# ------------------------------------------------------------------------------------------------ the cluster
CLUSTER_SIZES = (700, 70)
CLUSTER_MEMBERS = 300


def cluster_case(H, seed):
    """One 700-node graph followed by a 70-node graph, rows PR._rows(770, H, g, 3.0).  Planted: 300 rows of the first graph, spread over
    all 11 of its row tiles, are power-of-two multiples of one row (one class of 300: 44,850 pairs); one more copy of that row is the
    first node of the second graph (it must stay outside); three doubles (x[b] = 2 x[a]): two in the first graph, one in the second."""
    g = torch.Generator().manual_seed(7001 * seed + H)
    n0, n1 = CLUSTER_SIZES
    N = n0 + n1
    x = PR._rows(N, H, g, 3.0)
    free = torch.randperm(n0, generator=g).tolist()
    members = sorted(free[:CLUSTER_MEMBERS])
    assert len({m // 64 for m in members}) == (n0 + 63) // 64
    base = x[members[0]].clone()
    for j, m in enumerate(members):
        x[m] = base * 2.0 ** ((j % 9) - 4)
    x[n0] = base
    rest = free[CLUSTER_MEMBERS:]
    doubles = [(min(rest[0], rest[1]), max(rest[0], rest[1])), (min(rest[2], rest[3]), max(rest[2], rest[3])), (n0 + 11, n0 + 50)]
    for a, b in doubles:
        x[b] = 2 * x[a]
    return {'x': x, 'graph_ptr': [0, n0, N], 'N': N, 'H': H, 'members': members, 'copy': n0, 'doubles': doubles}


def truth_pairs(x, graph_ptr, threshold):
    """(pairs int64 [2, P], cos_ref dict, mask): the float64 relation — upper candidates with cos > threshold."""
    r = ER.cos_ref(x)
    N = x.shape[0]
    mask = ER.upper_mask(N, graph_ptr)
    keep = mask & (r['cos'] > threshold)
    return torch.nonzero(keep).T.contiguous(), r, mask


# ------------------------------------------------------------------------------------------------ the hook, restated with defects
DEFECTS = ('larger_root', 'drop_last', 'no_flatten', 'no_border', 'late_tile')
HARMLESS = ('col_ge_row',)


def restated_union(pairs, N, defect=None):
    """The device's union-find run one pair after the other: find both roots, hook the larger root under the smaller one; then the
    final labelling.  -> int64 [N].
      larger_root  the smaller root is hooked under the larger one (a component's label becomes its LARGEST id);
      drop_last    the last listed pair is never united (a grid-stride loop that ends one short);
      no_flatten   the labels are the parent entries as the hooks left them, without the final find."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    a, b = _np_pairs(pairs).tolist()
    if defect == 'drop_last':
        a, b = a[:-1], b[:-1]
    for u, v in zip(a, b):
        ru, rv = find(u), find(v)
        if ru == rv:
            continue
        hi, lo = max(ru, rv), min(ru, rv)
        if defect == 'larger_root':
            parent[lo] = hi
        else:
            parent[hi] = lo
    if defect == 'no_flatten':
        return torch.tensor(parent, dtype=I64)
    return torch.tensor([find(i) for i in range(N)], dtype=I64)


def restated_walk_pairs(score, graph_ptr, threshold, defect=None):
    """The pairs the symmetric walk unites, in its order: per row u the 64-column tiles from u's own tile to the end of its graph, the
    decision `col > row && col < hi && v == v && v > threshold`.  -> int64 [2, P].
      no_border    hi is N for every row (the graph border is ignored);
      late_tile    the walk starts one tile after the row's own tile;
      col_ge_row   the diagonal is admitted (col >= row): HARMLESS for components, a node united with itself changes nothing — listed
                   to show exactly that."""
    N = score.shape[0]
    hi = PR.row_range(graph_ptr, N)[1].tolist()
    rows = score.tolist()
    out = [[], []]
    for u in range(N):
        h = N if defect == 'no_border' else hi[u]
        first = (u // 64 + (1 if defect == 'late_tile' else 0)) * 64
        for v in range(first, h):
            s = rows[u][v]
            if (v >= u if defect == 'col_ge_row' else v > u) and s == s and s > threshold:
                out[0].append(u)
                out[1].append(v)
    return torch.tensor(out, dtype=I64).reshape(2, -1)
