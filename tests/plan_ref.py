"""Integer restatement of the on-device batch builder (csrc/plan_build.hip), entry by entry, written from include/mgvae_hip.h and the
comments of plan_build.hip: plain NumPy and Python loops over int64.  It is not a port of the kernels (no scans over blocks, no
atomics, no sorting networks) and it does not call deepgate/graph_plan.py: tests/test_plan_spec.py holds it to the host
implementations on a CPU, tests/test_hip_plan_entries.py then holds every entry to it on the GPU, array by array.

The second half builds the designed inputs: graphs whose list lengths, key populations, depths and signatures sit exactly on the
switches of the builder (register sort / heavy list / rank sort, tile cut, exact check / left to the caller, one-workgroup scan /
three kernels, level retry).  Every generator is seeded with np.random.Generator(PCG64(seed))."""
import numpy as np

TILE = 64                    # entries of one key per tile
NO_GATE = 255                # slot byte of a node that is never updated
CHECK_MAX = 48               # longest list mgv_colour_check compares itself
ROW_INTS = 32
I64 = np.int64

LIST_LENGTHS = (0, 1, 2, 31, 32, 33, 48, 49, 255, 256, 4095, 4096, 4097)
POPULATIONS = (0, 1, 63, 64, 65, 128, 129)


def _a(x):
    return np.asarray(x, dtype=I64).reshape(-1)


def _ptr(counts):
    p = np.zeros(len(counts) + 1, dtype=I64)
    np.cumsum(counts, out=p[1:])
    return p


# ------------------------------------------------------------------------------------------------ CSR
def csr(src, dst, N):
    """Both CSRs of the edge list in the stable order of a sort by destination / source over the VALID edges (both ends in [0, N)):
    in_ptr, in_src, in_dst, in_eid, out_ptr, out_dst, out_slot, out_eid, status.  Slots behind the valid edges are 0, status = 1
    when an edge was skipped.  out_slot = in-CSR position of the same edge."""
    src, dst = _a(src), _a(dst)
    E = src.size
    eid = np.nonzero((src >= 0) & (src < N) & (dst >= 0) & (dst < N))[0]
    V = eid.size
    by_dst = eid[np.argsort(dst[eid], kind='stable')]
    by_src = eid[np.argsort(src[eid], kind='stable')]
    in_ptr = _ptr(np.bincount(dst[eid], minlength=N)[:N])
    out_ptr = _ptr(np.bincount(src[eid], minlength=N)[:N])
    z = lambda: np.zeros(E, dtype=I64)
    in_src, in_dst, in_eid, out_dst, out_slot, out_eid, pos = z(), z(), z(), z(), z(), z(), z()
    in_src[:V], in_dst[:V], in_eid[:V] = src[by_dst], dst[by_dst], by_dst
    pos[by_dst] = np.arange(V)
    out_dst[:V], out_slot[:V], out_eid[:V] = dst[by_src], pos[by_src], by_src
    return in_ptr, in_src, in_dst, in_eid, out_ptr, out_dst, out_slot, out_eid, int(V < E)


def sort_lists(ptr, vals):
    """Every list vals[ptr[n] : ptr[n + 1]] ascending."""
    ptr, out = _a(ptr), _a(vals).copy()
    for n in range(ptr.size - 1):
        out[ptr[n]:ptr[n + 1]] = np.sort(out[ptr[n]:ptr[n + 1]])
    return out


def scan(x):
    """Exclusive prefix sums with the total behind them: n + 1 values."""
    return _ptr(_a(x))


# ------------------------------------------------------------------------------------------------ levels
def levels(in_ptr, out_ptr, out_dst, rounds):
    """`rounds` steps of frontier relaxation: level[n] = the round in which the last parent of n was evaluated (-1: n was not
    reached, its level is left out of a comparison), done = nodes on levels below `rounds` (the frontiers the steps consumed)."""
    in_ptr, out_ptr, out_dst = _a(in_ptr), _a(out_ptr), _a(out_dst)
    N = in_ptr.size - 1
    pending = (in_ptr[1:] - in_ptr[:-1]).copy()
    level = np.full(N, -1, dtype=I64)
    frontier = [n for n in range(N) if pending[n] == 0]
    for n in frontier:
        level[n] = 0
    done = 0
    for r in range(rounds):
        nxt = []
        for n in frontier:
            for e in range(out_ptr[n], out_ptr[n + 1]):
                c = out_dst[e]
                pending[c] -= 1
                if pending[c] == 0:
                    level[c] = r + 1
                    nxt.append(int(c))
        done += len(frontier)
        frontier = nxt
        if not frontier:
            break
    return level, done


# ------------------------------------------------------------------------------------------------ buckets
def slot_table(gate_ids):
    tab = np.full(256, NO_GATE, dtype=I64)
    for s, g in enumerate(gate_ids):
        tab[int(g)] = s
    return tab


def keys(gate, level64, table, T, clamp=True, min_level=1):
    """gslot (255: never updated), level32, key = level * T + slot (-1: never updated), maxlevel (over ALL nodes, at least 0).
    A node is updated when its level is >= 1 and its gate id, cut to an integer and clamped to [0, 255], has a slot."""
    g = np.trunc(np.asarray(gate, dtype=np.float64).reshape(-1)).astype(I64)
    lv = _a(level64)
    if clamp:
        slot = table[np.clip(g, 0, 255)]
    else:
        slot = np.where((g >= 0) & (g <= 255), table[np.clip(g, 0, 255)], NO_GATE)
    active = (lv >= min_level) & (slot != NO_GATE)
    gslot = np.where(active, slot, NO_GATE)
    key = np.where(active, lv * T + slot, -1)
    return gslot, lv.copy(), key, int(max(0, lv.max())) if lv.size else 0


def check_levels(in_src, in_dst, gslot, level, strict=True):
    """2 when an updated node has a source that is not on a strictly lower level, else 0."""
    s, d, gslot, level = _a(in_src), _a(in_dst), _a(gslot), _a(level)
    if s.size == 0:
        return 0
    bad = (gslot[d] != NO_GATE) & ((level[s] >= level[d]) if strict else (level[s] > level[d]))
    return 2 if bad.any() else 0


def count_sort(key, K):
    """order = items with key >= 0 by (key, item id); key_start[K + 1] = first position of every key."""
    key = _a(key)
    keep = np.nonzero(key >= 0)[0]
    order = keep[np.argsort(key[keep], kind='stable')]
    return order, _ptr(np.bincount(key[keep], minlength=K)[:K])


def tiles(key_start, order, in_ptr, out_ptr, T, L, tile=TILE):
    """ntile[K], tile_first[K + 1], tile_start / tile_count / tile_slot per tile, order_span [n_active, 4], level_tile_ptr[L + 1]:
    every key's run cut into tiles of <= 64 entries; a level's tiles are those of its T keys."""
    key_start, order, in_ptr, out_ptr = _a(key_start), _a(order), _a(in_ptr), _a(out_ptr)
    K = L * T
    ntile = np.array([-(-int(key_start[k + 1] - key_start[k]) // tile) for k in range(K)], dtype=I64)
    tile_first = _ptr(ntile)
    t_start, t_count, t_slot = [], [], []
    for k in range(K):
        c = int(key_start[k + 1] - key_start[k])
        for t in range(int(ntile[k])):
            t_start.append(int(key_start[k]) + t * tile)
            t_count.append(min(tile, c - t * tile))
            t_slot.append(k % T)
    span = np.stack([in_ptr[order], in_ptr[order + 1], out_ptr[order], out_ptr[order + 1]], 1) if order.size else np.zeros((0, 4), dtype=I64)
    ltp = np.array([tile_first[l * T] for l in range(L + 1)], dtype=I64)
    return ntile, tile_first, _a(t_start), _a(t_count), _a(t_slot), span, ltp


def order_rows(order, in_ptr, in_src, out_ptr, out_dst, out_slot, gslot, n_src=4, n_out=8):
    """[n_active, 32]: ints 0..3 the spans, 4..7 the first 4 sources, 8..23 the first 8 consumers as (node, in-CSR slot), 24..25 the
    consumers' slot bytes (little endian, 0xff where there is none or it is never updated), everything else -1."""
    order, in_ptr, in_src, out_ptr, out_dst, out_slot, gslot = (_a(v) for v in (order, in_ptr, in_src, out_ptr, out_dst, out_slot, gslot))
    rows = np.full((order.size, ROW_INTS), -1, dtype=I64)
    for i, v in enumerate(order):
        a, b, c, d = in_ptr[v], in_ptr[v + 1], out_ptr[v], out_ptr[v + 1]
        rows[i, 0:4] = (a, b, c, d)
        for k in range(min(n_src, b - a)):
            rows[i, 4 + k] = in_src[a + k]
        byte = [0xff] * 8
        for j in range(min(n_out, d - c)):
            rows[i, 8 + 2 * j], rows[i, 9 + 2 * j] = out_dst[c + j], out_slot[c + j]
            byte[j] = int(gslot[out_dst[c + j]])
        for w in range(2):
            u = sum(byte[4 * w + j] << (8 * j) for j in range(4))
            rows[i, 24 + w] = u - (1 << 32) if u >= (1 << 31) else u
    return rows


def pairs(in_ptr, xcls, cap=255):
    """(in-degree, class) pairs numbered ascending in degree * 256 + class: cid[N], C, cls_deg[C], cls_x[C], status (3: a degree
    above 255; such a node marks no pair and takes the number its pair (255, class) has or would have)."""
    in_ptr, x = _a(in_ptr), _a(xcls)
    deg = in_ptr[1:] - in_ptr[:-1]
    fits = deg <= cap
    present = np.zeros(65536, dtype=I64)
    present[(deg * 256 + x)[fits]] = 1
    rank = _ptr(present)
    cid = rank[np.minimum(deg, cap) * 256 + x]
    codes = np.nonzero(present)[0]
    return cid, int(codes.size), codes >> 8, codes & 255, 0 if fits.all() else 3


def first_stage(in_ptr, xcls, max_classes=256):
    """What GraphPlan.first_stage_classes returns: (cid, C, ptr[C + 1], idx, cls_x) over the (TRUE in-degree, class) pairs — a list
    of `degree` zeros per pair — or None when there are more than max_classes pairs.  Below degree 256 this is `pairs`."""
    in_ptr, x = _a(in_ptr), _a(xcls)
    code = (in_ptr[1:] - in_ptr[:-1]) * 256 + x
    uniq, cid = np.unique(code, return_inverse=True)
    if not 0 < uniq.size <= max_classes:
        return None
    p = _ptr(uniq // 256)
    return _a(cid), int(uniq.size), p, np.zeros(max(int(p[-1]), 1), dtype=I64), uniq % 256


CSR_FIELDS = ('in_ptr', 'in_src', 'in_dst', 'in_eid', 'out_ptr', 'out_dst', 'out_slot', 'out_eid', 'status')


def plan_fields(src, dst, N, gate, level, gate_ids):
    """Every field of a levelised plan, the entries above chained the way the header describes: CSR, keys, stable sort by key, tiles,
    packed rows, and the tiles grouped by slot (a second stable sort)."""
    T = len(gate_ids)
    f = dict(zip(CSR_FIELDS, csr(src, dst, N)))
    gslot, lv, key, maxlevel = keys(gate, level, slot_table(gate_ids), T)
    L = maxlevel + 1 if N > 0 else 0
    Lk = max(L, 1)
    order, key_start = count_sort(key, Lk * T)
    _, _, t_start, t_count, t_slot, span, ltp = tiles(key_start, order, f['in_ptr'], f['out_ptr'], T, Lk)
    slot_tiles, slot_start = count_sort(t_slot, T)
    f.update(gslot=gslot, level=lv, num_levels=L, order=order, order_span=span,
             order_rows=order_rows(order, f['in_ptr'], f['in_src'], f['out_ptr'], f['out_dst'], f['out_slot'], gslot),
             tile_start=t_start, tile_count=t_count, tile_slot=t_slot, slot_tiles=slot_tiles, slot_tile_ptr=[int(v) for v in slot_start],
             level_tile_ptr=[int(v) for v in ltp], num_tiles=int(t_start.size), n_active=int(order.size), num_slots=T, key=key,
             key_start=key_start, bad_levels=check_levels(f['in_src'], f['in_dst'], gslot, lv))
    return f


# ------------------------------------------------------------------------------------------------ colours
M64 = (1 << 64) - 1


def colour_signature(i, ptr, idx, prev, xcls):
    """(class, previous colour, degree, neighbours' previous colours ascending)."""
    lst = sorted(int(prev[j]) for j in idx[ptr[i]:ptr[i + 1]])
    return (int(xcls[i]), int(prev[i]), len(lst), tuple(lst))


def colour_keys(ptr, idx, prev, f, xcls, key_bits):
    """The documented key in Python integers mod 2^64, cut to its top key_bits bits; f [3][fstride]."""
    out = []
    for i in range(len(ptr) - 1):
        h1 = h2 = 0
        for j in idx[ptr[i]:ptr[i + 1]]:
            h1 += int(f[0][prev[j]])
            h2 += int(f[1][prev[j]])
        k = (h1 * 0x1E3779B97F4A7C15 + h2 + int(f[2][prev[i]]) + int(xcls[i]) * 0x632BE59BD9B4E019
             + int(ptr[i + 1] - ptr[i]) * 0x2545F4914F6CDD1D) & M64
        out.append(k >> (64 - key_bits))
    return out


def colour_check(ptr, idx, prev, xcls, cid, rep, multiset=True, check_max=CHECK_MAX):
    """flags[0] = 1 when a node differs from its colour's representative in class, previous colour, degree or (lists of at most 48)
    neighbour-colour multiset; flags[1] = nodes that agree in the first three and whose longer lists were not compared."""
    bad = n_long = 0
    for i in range(len(ptr) - 1):
        r = int(rep[cid[i]])
        if r == i:
            continue
        a, b = colour_signature(i, ptr, idx, prev, xcls), colour_signature(r, ptr, idx, prev, xcls)
        if a[:3] != b[:3]:
            bad = 1
        elif a[2] > check_max:
            n_long += 1
        elif (a[3] != b[3]) if multiset else (set(a[3]) != set(b[3])):
            bad = 1
    return bad, n_long


def true_grouping(ptr, idx, prev, xcls):
    """The grouping by signature: colours numbered in order of their first member, rep = first member."""
    seen, cid, rep = {}, [], []
    for i in range(len(ptr) - 1):
        s = colour_signature(i, ptr, idx, prev, xcls)
        if s not in seen:
            seen[s] = len(rep)
            rep.append(i)
        cid.append(seen[s])
    return _a(cid), _a(rep)


def colour_groups(skey, by_colour):
    """Runs of equal sorted keys -> cid[N], starts[C + 1] (starts[C] = N), rep[C] (a run's first member), C."""
    skey, by = list(skey), _a(by_colour)
    N = len(skey)
    cid, starts, rep = np.zeros(N, dtype=I64), [], []
    for i in range(N):
        if i == 0 or skey[i] != skey[i - 1]:
            starts.append(i)
            rep.append(int(by[i]))
        cid[by[i]] = len(rep) - 1
    return cid, _a(starts + [N]), _a(rep), len(rep)


def rep_rows(C, rep, ptr, prev, xcls, heavy_row):
    """rptr[C + 1], own[C], xrep[C], n_heavy (lists LONGER than heavy_row)."""
    rep, ptr, prev, xcls = _a(rep)[:C], _a(ptr), _a(prev), _a(xcls)
    d = ptr[rep + 1] - ptr[rep]
    return _ptr(d), prev[rep], xcls[rep], int((d > heavy_row).sum())


def rep_lists(C, rep, ptr, idx, prev):
    """ent = the representatives' lists in previous colours, one after the other; row = the colour every entry belongs to."""
    ent, row = [], []
    for c in range(C):
        r = int(rep[c])
        for j in idx[ptr[r]:ptr[r + 1]]:
            ent.append(int(prev[j]))
            row.append(c)
    return _a(ent), _a(row)


def sorted_key_counts(sorted_keys, K):
    """Members per key k in [0, K) of an ascending key array."""
    s = _a(sorted_keys)
    return np.array([int((s == k).sum()) for k in range(K)], dtype=I64)


def seg_level(counts, gid, seg, base, at_least_one=True):
    """One level of the segment tables: totals {segments, members, partial rows, colours with more than one segment}, seg_ptr
    [segments + 1], out_row [segments] (a colour's only segment writes row gid[g], g without gid; a partial row base + its running
    number), gid_next / counts_next of the colours that go on."""
    counts = _a(counts)
    G = counts.size
    nseg = -(-counts // seg)
    if at_least_one:
        nseg = np.maximum(1, nseg)
    start = _ptr(counts)
    seg_ptr, out_row, gid_next, counts_next = [], [], [], []
    partial = 0
    for g in range(G):
        name = int(gid[g]) if gid is not None else g
        for j in range(int(nseg[g])):
            seg_ptr.append(int(start[g]) + seg * j)
            if nseg[g] > 1:
                out_row.append(base + partial)
                partial += 1
            else:
                out_row.append(name)
        if nseg[g] > 1:
            gid_next.append(name)
            counts_next.append(int(nseg[g]))
    seg_ptr.append(int(start[G]))
    totals = [int(nseg.sum()), int(start[G]), partial, len(gid_next)]
    return totals, _a(seg_ptr), _a(out_row), _a(gid_next), _a(counts_next)


def sum_levels(counts, seg=64, at_least_one=True):
    """All levels of the tables for C colours: dict(C, rows, levels=[(n_seg, seg_ptr, out_row | None, src_row)]); out_row is None
    on a single level where segment s writes row s."""
    C = len(counts)
    out, gid, base, src_row = [], None, C, 0
    while True:
        totals, sp, orow, gid_n, counts_n = seg_level(counts, gid, seg, base, at_least_one)
        plain = totals[2] == 0 and gid is None and base == C
        out.append((totals[0], sp, None if plain else orow, src_row))
        if totals[2] == 0:
            return dict(C=C, rows=base, levels=out)
        gid, counts = gid_n, counts_n
        src_row, base = base, base + totals[2]


# ================================================================================================ designed inputs
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def lists_graph(N=1501, seed=1):
    """A multigraph in shuffled edge order with parallel edges and self loops: node k < 13 has exactly LIST_LENGTHS[k] in-edges and as
    many out-edges (one of each a self loop from length 2 on); the other ends are drawn, with repetition, from the remaining nodes,
    which also carry a few self loops of their own.  N = 1: one node with 33 self loops.  -> (src, dst, N)"""
    rng = _rng(seed)
    if N == 1:
        return np.zeros(33, dtype=I64), np.zeros(33, dtype=I64), 1
    S = len(LIST_LENGTHS)
    assert N > S + 8
    src, dst = [], []
    for k, d in enumerate(LIST_LENGTHS):
        loop = 1 if d >= 2 else 0
        if loop:
            src.append([k]); dst.append([k])
        other = rng.integers(S, N, size=d - loop)
        src.append(np.full(d - loop, k)); dst.append(other)                 # k's out-list
        other = rng.integers(S, N, size=d - loop)
        src.append(other); dst.append(np.full(d - loop, k))                 # k's in-list
    fill = rng.integers(S, N, size=40)
    src.append(fill); dst.append(fill)                                      # self loops among the rest
    src, dst = np.concatenate(src).astype(I64), np.concatenate(dst).astype(I64)
    p = rng.permutation(src.size)
    return src[p], dst[p], N


GATE_SETS = {1: [255], 2: [0, 9], 5: [1, 2, 3, 255, 7]}      # position = slot; the last slot of T = 2 and T = 5 gets no node
ODD_GATES = (-3.0, 0.0, 255.0, 300.0, 77.0, 254.0)             # clamped from below / above, the table's ends, outside every gate set


def levelled_dag(T, seed=2):
    """A levelised DAG for a model with T slots: levels 0..10.  Levels 1..7: slot j of the used slots holds exactly
    POPULATIONS[(level - 1 + j) % 7] updated nodes (so every population meets every used slot, and the last slot none); level 8
    holds only nodes outside the gate set, level 9 one updated node, level 10 (the deepest) one node that is never updated.  Level 0
    holds sources, some of an active gate type.  Gate values include ODD_GATES.  Every node above level 0 has 1..5 in-edges (cycling:
    4 and 5 occur) from lower levels; four updated nodes of the lowest level that has four have exactly 0, 8, 9 and 20 consumers, half of them never
    updated.  -> dict(N, src, dst, gate float32, level int64, gate_ids, T, consumers={count: node})"""
    rng = _rng(seed + T)
    gate_ids = GATE_SETS[T]
    tab = slot_table(gate_ids)
    used = list(range(T - 1)) if T > 1 else [0]
    target = {(l, s): POPULATIONS[(l - 1 + j) % 7] for l in range(1, 8) for j, s in enumerate(used)}
    target[(9, used[0])] = 1
    gate, level = [], []

    def add(g, l):
        gate.append(float(g)); level.append(l)
        return len(gate) - 1
    for i in range(40):                                  # level 0: sources, every fourth of an active type
        add(gate_ids[0] if i % 4 == 0 else 100, 0)
    have = {k: 0 for k in target}
    for g in ODD_GATES:                                  # twice each, where the key they fall into has room (or anywhere, if none)
        s = int(tab[int(np.clip(np.trunc(g), 0, 255))])
        spots = [l for l in range(1, 8) if s == NO_GATE or target.get((l, s), 0) - have.get((l, s), 0) >= 60][:2]
        assert len(spots) == 2
        for l in spots:
            add(g, l)
            if s != NO_GATE:
                have[(l, s)] += 1
    for (l, s), want in sorted(target.items()):
        for _ in range(want - have[(l, s)]):
            add(gate_ids[s], l)
    for l in (3, 8, 8, 8, 10):                           # never updated: outside the gate set
        add(77, l)
    gate, level = np.array(gate, dtype=np.float32), np.array(level, dtype=I64)
    N = gate.size
    gslot = keys(gate, level, tab, T)[0]
    lsp = min(l for l in range(1, 7) if int(((level == l) & (gslot != NO_GATE)).sum()) >= 4)      # the lowest level with four updated nodes
    first = [n for n in range(N) if level[n] == lsp and gslot[n] != NO_GATE]
    special = dict(zip((0, 8, 9, 20), first[:4]))
    src, dst = [], []
    plain = np.array([n for n in range(N) if n not in special.values()])
    for n in range(N):
        if level[n] == 0:
            continue
        low = plain[level[plain] < level[n]]
        k = (1, 2, 3, 4, 5, 2)[n % 6]
        for s in rng.choice(low, size=k):
            src.append(int(s)); dst.append(n)
    above = np.nonzero(level > lsp)[0]
    on, off = above[gslot[above] != NO_GATE], above[gslot[above] == NO_GATE]
    for cnt, node in special.items():
        half = cnt // 2
        cons = np.concatenate([rng.choice(off, size=half), rng.choice(on, size=cnt - half, replace=False)])
        for c in rng.permutation(cons):
            src.append(int(node)); dst.append(int(c))
    src, dst = np.array(src, dtype=I64), np.array(dst, dtype=I64)
    p = rng.permutation(src.size)
    return dict(N=N, src=src[p], dst=dst[p], gate=gate, level=level, gate_ids=gate_ids, T=T, consumers=special)


def chain(n):
    """n levels: the chain 0 -> 1 -> ... -> n - 1 with skip edges i -> i + 2 on every seventh node (a node waits for its LAST parent)
    and a side branch: the leaf n off node n - 2, on the chain's last level.  n + 1 nodes.  -> (src, dst, N, level)"""
    assert n >= 4
    src = list(range(n - 1)) + list(range(0, n - 2, 7)) + [n - 2]
    dst = list(range(1, n)) + list(range(2, n, 7)) + [n]
    level = np.concatenate([np.arange(n), [n - 1]]).astype(I64)
    return np.array(src, dtype=I64), np.array(dst, dtype=I64), n + 1, level


def degree_graph(extra=None):
    """Node d < 256 (class d % 3 of {0, 1, 255}) has in-degree d; `extra`: one more node with that in-degree, of node 255's class.
    Sources: seven nodes behind.  -> (src, dst, N, xcls)"""
    cls = np.array([0, 1, 255])
    deg = list(range(256)) + ([extra] if extra is not None else [])
    n = len(deg)
    dst = np.repeat(np.arange(n), deg)
    src = n + (np.arange(dst.size) % 7)
    x = np.concatenate([cls[np.minimum(np.arange(n), 255) % 3], np.zeros(7, dtype=np.int64)]).astype(np.uint8)
    return src.astype(np.int64), dst.astype(np.int64), n + 7, x


PAIR_LENGTHS = (0, 1, 48, 49, 300)


def coloured_lists(seed=3):
    """Lists over a pool of 24 leaf nodes in 6 previous colours (leaf j: colour j % 6, class 0, no list).  Behind the pool:
      * per length in PAIR_LENGTHS two nodes with EQUAL signatures whose lists are permuted and name different leaves of the same
        colours ('equal');
      * pairs that differ in exactly one thing: one neighbour colour at length 48 ('colour48') and at 49 ('colour49') — the two
        lists hold the same SET of colours —, the class only ('class'), the previous colour only ('prev'), the degree only
        ('degree': 20 and 21 entries of one colour).
    -> dict(N, ptr, idx, prev, xcls, Cp, pairs={name: (a, b)})"""
    rng = _rng(seed)
    P, Cp = 24, 8
    prev, xcls, lists, pairs_ = [j % 6 for j in range(P)], [0] * P, [[] for _ in range(P)], {}

    def leaf(colour):
        return int(colour + 6 * rng.integers(0, 4))

    def node(colours, pv, xc):
        lists.append([leaf(c) for c in colours]); prev.append(pv); xcls.append(xc)
        return len(lists) - 1
    for d in PAIR_LENGTHS:
        cols = list(rng.integers(0, 6, size=d))
        pairs_['equal%d' % d] = (node(cols, 6, 1), node(list(rng.permutation(cols)), 6, 1))
    for d in (48, 49):
        cols = [0, 0, 1] + list(rng.integers(0, 6, size=d - 3))
        other = [0, 1, 1] + cols[3:]
        pairs_['colour%d' % d] = (node(cols, 7, 2), node(list(rng.permutation(other)), 7, 2))
    cols = list(rng.integers(0, 6, size=12))
    pairs_['class'] = (node(cols, 6, 3), node(list(rng.permutation(cols)), 6, 4))
    pairs_['prev'] = (node(cols, 6, 5), node(list(rng.permutation(cols)), 7, 5))
    pairs_['degree'] = (node([2] * 20, 7, 6), node([2] * 21, 7, 6))
    ptr = _ptr([len(l) for l in lists])
    idx = _a([j for l in lists for j in l])
    return dict(N=len(lists), ptr=ptr, idx=idx, prev=_a(prev), xcls=_a(xcls), Cp=Cp, pairs=pairs_)


def colour_f(Cp, seed=4):
    """The random values of the grouping key: int64 [3][Cp + 1] in [1, 2^62)."""
    return _rng(seed).integers(1, 1 << 62, size=(3, Cp + 1), dtype=I64)
