"""GPU tests of the batch builder's entries one by one (csrc/plan_build.hip through the C ABI): every output array of every entry equals
the integer restatement tests/plan_ref.py (held to the host implementations by tests/test_plan_spec.py) on the designed inputs —
list lengths, key populations, depths, colour counts and signatures that sit exactly on the builder's switches.  Equality is exact
everywhere: no tolerances.  Each test hands an entry its own buffers: outputs pre-filled with a sentinel (0x5a5a5a5a ints, 0xA5 bytes)
with guard words behind their documented extents that must stay untouched, scratch sized by the entry's own size query and also
pre-filled; a second call on fresh buffers must be bit-identical (arrival order of the atomics must not leak)."""
import ctypes

import numpy as np
import pytest
import torch

import plan_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x5a5a5a5a
GUARD = 16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def ints(n):
    """n sentinel ints and GUARD more behind them."""
    return torch.full((int(n) + GUARD,), SENT, dtype=torch.int32, device='cuda:0')


def octets(n):
    return torch.full((int(n) + GUARD,), 0xA5, dtype=torch.uint8, device='cuda:0')


def up(a, dtype=torch.int32):
    """A host array on the device (at least one element behind the pointer, so that it is never NULL)."""
    a = np.asarray(a).reshape(-1)
    t = torch.zeros(max(a.size, 1), dtype=dtype, device='cuda:0')
    if a.size:
        t[:a.size] = torch.from_numpy(a.astype(np.int64 if dtype != torch.float32 else np.float32)).to('cuda:0').to(dtype)
    return t


def eq(buf, want, name=''):
    """buf[:len(want)] == want exactly, and everything behind it is still the sentinel."""
    want = np.asarray(want).reshape(-1)
    w = torch.from_numpy(want.astype(np.int64)).to('cuda:0').to(buf.dtype)
    assert torch.equal(buf[:want.size], w), name
    untouched(buf, want.size, name)


def untouched(buf, n, name=''):
    fill = SENT if buf.dtype == torch.int32 else 0xA5
    assert bool((buf[n:] == fill).all()), (name, 'written behind', n)


def twice(run):
    """Two calls on fresh buffers: bit-identical outputs (guards included).  -> the first call's outputs"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for k, (u, v) in enumerate(zip(a, b)):
        if torch.is_tensor(u):
            assert torch.equal(u, v), ('second call differs', k)
    return a


def call(name, *args):
    from deepgate import _hip
    _hip.call(name, *args)


def value(name, *args):
    from deepgate import _hip
    return _hip.call_value(name, *args)


def ptr(t):
    from deepgate import _hip
    return _hip.ptr(t)


# ------------------------------------------------------------------------------------------------ mgv_plan_csr
def run_csr(src, dst, N, eids=True):
    E = len(src)
    s, d = up(src, torch.int64), up(dst, torch.int64)
    in_ptr, out_ptr = ints(N + 1), ints(N + 1)
    in_src, in_dst, out_dst, out_slot, in_eid, out_eid = (ints(E) for _ in range(6))
    n_s = value('mgv_plan_csr_scratch_ints', N, E)
    scratch, status = ints(n_s), ints(2)
    call('mgv_plan_csr', N, E, ptr(s), ptr(d), ptr(in_ptr), ptr(in_src), ptr(in_dst), ptr(out_ptr), ptr(out_dst), ptr(out_slot),
         ptr(in_eid) if eids else None, ptr(out_eid) if eids else None, ptr(scratch), n_s, ptr(status))
    untouched(scratch, n_s, 'scratch')
    return in_ptr, in_src, in_dst, in_eid, out_ptr, out_dst, out_slot, out_eid, status


def check_csr(src, dst, N, eids=True):
    got = twice(lambda: run_csr(src, dst, N, eids))
    want = R.csr(src, dst, N)
    E = len(src)
    for name, g, w in zip(R.CSR_FIELDS, got, want):
        if name == 'status':
            eq(g, [w, 0], name)
        elif name.endswith('_eid') and not eids:
            untouched(g, 0, name)
        elif E == 0 and not name.endswith('_ptr'):
            untouched(g, 0, name)                        # nothing to write
        else:
            eq(g, w, name)
    return want


@pytest.mark.parametrize('N', [1, 1501, 2048])
def test_csr_on_the_designed_lists(N):
    """mgv_plan_csr with in_eid / out_eid and without: lists of 0 .. 4097 entries (register network, LDS bitonic sort, rank sort and
    both of each switch), parallel edges, self loops, shuffled edge order."""
    _dev()
    src, dst, n = R.lists_graph(N)
    check_csr(src, dst, n, eids=True)
    check_csr(src, dst, n, eids=False)


@pytest.mark.parametrize('case', ['empty1', 'empty777', 'bad_source', 'negative_destination', 'all_bad', 'three_kernel_scans'])
def test_csr_edge_cases(case):
    """mgv_plan_csr: no edges; edges out of range are skipped, the pointers count the valid ones only, the tails are zero and
    status[0] = 1; N = 40,000 / E = 90,000 puts both scans on the three-kernel path with a partial last block."""
    _dev()
    rng = np.random.Generator(np.random.PCG64(12))
    if case.startswith('empty'):
        N, src, dst = int(case[5:]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    elif case == 'three_kernel_scans':
        N = 40000
        src, dst = rng.integers(0, N, size=90000), rng.integers(0, N, size=90000)
    else:
        N = 300
        src, dst = rng.integers(0, N, size=900), rng.integers(0, N, size=900)
        if case == 'bad_source':
            src[451] = N
        elif case == 'negative_destination':
            dst[17] = -1
        else:
            src[::2], dst[1::2] = N + 5, -7
    want = check_csr(src, dst, N)
    assert want[8] == (0 if case in ('empty1', 'empty777', 'three_kernel_scans') else 1)
    if case == 'all_bad':
        assert not want[0].any() and not want[4].any() and not want[1].any() and not want[6].any()


# ------------------------------------------------------------------------------------------------ mgv_sort_lists_i32
def test_sort_lists_with_heavy_duplication():
    """mgv_sort_lists_i32 on lists of the designed lengths whose values repeat heavily (five distinct values), and a list of 4,097
    copies of one value (the rank sort's tie rule)."""
    _dev()
    rng = np.random.Generator(np.random.PCG64(13))
    lengths = list(rng.permutation(np.array(R.LIST_LENGTHS))) + [4097]
    p = R.scan(lengths)
    vals = rng.integers(0, 5, size=int(p[-1])) * 1000 - 2000
    vals[p[-2]:] = 7
    N, E = len(lengths), int(p[-1])

    def run():
        v = ints(E)
        v[:E] = up(vals)
        scratch = ints(N + 1 + E)
        call('mgv_sort_lists_i32', N, E, ptr(up(p)), ptr(v), ptr(scratch), N + 1 + E)
        untouched(scratch, N + 1 + E)
        return (v,)
    eq(twice(run)[0], R.sort_lists(p, vals))


# ------------------------------------------------------------------------------------------------ mgv_scan_exclusive_i32
@pytest.mark.parametrize('n,in_place', [(32768, False), (32769, False), (34816, False), (34817, False), (1000, True), (34817, True)])
def test_scan_at_the_switch_and_in_place(n, in_place):
    """mgv_scan_exclusive_i32 at the last size of the one-workgroup scan, the first of the three-kernel scan, a whole number of blocks
    (17 x 2,048) and one more; in == out always takes the three-kernel path."""
    _dev()
    x = np.random.Generator(np.random.PCG64(n)).integers(0, 9, size=n)

    def run():
        out, scratch = ints(n + 1), ints(n // 2048 + 2)
        src = out if in_place else up(x)
        if in_place:
            out[:n] = up(x)
        call('mgv_scan_exclusive_i32', n, ptr(src), ptr(out), ptr(scratch))
        untouched(scratch, n // 2048 + 2)
        return (out,)
    eq(twice(run)[0], R.scan(x))


# ------------------------------------------------------------------------------------------------ mgv_plan_levels
def run_levels(c, N, rounds):
    level, done = ints(N), ints(1)
    n_s = 3 * N + rounds + 2
    scratch = ints(n_s)
    call('mgv_plan_levels', N, ptr(up(c['in_ptr'])), ptr(up(c['out_ptr'])), ptr(up(c['out_dst'])), ptr(level), rounds, ptr(scratch), n_s, ptr(done))
    untouched(scratch, n_s)
    return level, done


def check_levels_entry(src, dst, N, rounds):
    c = dict(zip(R.CSR_FIELDS, R.csr(src, dst, N)))
    level, done = twice(lambda: run_levels(c, N, rounds))
    want, n_done = R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], rounds)
    eq(done, [n_done], 'done')
    untouched(level, N)
    reached = torch.from_numpy(want >= 0).to('cuda:0')
    assert torch.equal(level[:N][reached].long(), torch.from_numpy(want[want >= 0]).to('cuda:0'))
    return want, n_done


def test_levels_and_the_done_contract():
    """mgv_plan_levels: done = the nodes on levels below `rounds`; the levels of the levelised nodes are right, a node that was never
    reached is left out."""
    _dev()
    src, dst, N, level = R.chain(513)
    want, done = check_levels_entry(src, dst, N, 512)
    assert done == 512 and np.array_equal(want, level)
    want, done = check_levels_entry(src, dst, N, 513)
    assert done == N
    none = np.zeros(0, dtype=np.int64)
    assert check_levels_entry(none, none, 300, 1)[1] == 300                                      # isolated nodes: one round
    want, done = check_levels_entry(np.array([0, 0, 0, 1, 2, 2]), np.array([2, 2, 2, 2, 3, 3]), 4, 5)    # parallel edges between levels
    assert want.tolist() == [0, 0, 1, 2] and done == 4
    want, done = check_levels_entry(np.array([0, 1, 2, 2, 3, 5]), np.array([1, 2, 0, 3, 4, 3]), 7, 8)    # a 3-cycle and its tail
    assert done == 2 < 7 and want.tolist() == [-1, -1, -1, -1, -1, 0, 0]


@pytest.mark.parametrize('n', [512, 513])
def test_asap_levels_without_and_with_the_retry(n, monkeypatch):
    """GraphPlan.asap_levels: 512 levels fit the first batch of rounds, 513 take the retry."""
    dev = _dev()
    from deepgate import _hip
    from deepgate.graph_plan import GraphPlan
    monkeypatch.setenv('MGV_PLAN', 'hip')
    src, dst, N, level = R.chain(n)
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = GraphPlan(torch.from_numpy(np.stack([src, dst])).to(dev), N).asap_levels()
    c = dict(zip(R.CSR_FIELDS, R.csr(src, dst, N)))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], N + 1)[0]))
    assert calls.count('mgv_plan_levels') == (1 if n == 512 else 2)


# ------------------------------------------------------------------------------------------------ keys -> check -> sort -> tiles -> rows
def run_count_sort(key, n, K):
    order, key_start = ints(n), ints(K + 1)
    n_s = value('mgv_count_sort_scratch_ints', n, K)
    scratch = ints(n_s)
    call('mgv_count_sort_i32', n, ptr(up(key)), K, ptr(order), ptr(key_start), ptr(scratch), n_s)
    untouched(scratch, n_s)
    return order, key_start


@pytest.mark.parametrize('T', [1, 2, 5])
def test_the_level_chain_stage_by_stage(T):
    """mgv_plan_keys, mgv_plan_check_levels, mgv_count_sort_i32, mgv_plan_tile_counts, mgv_plan_tiles, mgv_plan_order_rows chained as
    GraphPlan._set_levels_hip chains them, on levelled_dag(T): every stage's outputs equal the restatement before they feed the next
    (the next stage reads the restatement's arrays).  Key populations 0, 1, 63, 64, 65, 128, 129; an empty level; an empty slot;
    clamped gate ids; level-0 nodes of an active type; 4 and 5 in-edges; 0, 8, 9 and 20 consumers, some never updated."""
    _dev()
    g = R.levelled_dag(T)
    N = g['N']
    f = R.plan_fields(g['src'], g['dst'], N, g['gate'], g['level'], g['gate_ids'])
    E = len(g['src'])
    tab = (ctypes.c_uint8 * 256)(*[int(v) for v in R.slot_table(g['gate_ids'])])
    gate, lv64 = up(g['gate'], torch.float32), up(g['level'], torch.int64)

    def run_keys():
        gslot, level32, key, flags = octets(N), ints(N), ints(N), ints(1)
        call('mgv_plan_keys', N, T, ptr(gate), ptr(lv64), tab, ptr(gslot), ptr(level32), ptr(key), ptr(flags))
        return gslot, level32, key, flags
    gslot, level32, key, maxlevel = twice(run_keys)
    eq(gslot, f['gslot'], 'gslot'); eq(level32, f['level'], 'level'); eq(key, f['key'], 'key')
    eq(maxlevel, [10], 'maxlevel')                       # the deepest node is never updated: the maximum is over all nodes
    L = f['num_levels']
    K = L * T
    in_ptr, in_src, in_dst, out_ptr, out_dst, out_slot = (up(f[k]) for k in ('in_ptr', 'in_src', 'in_dst', 'out_ptr', 'out_dst', 'out_slot'))
    gs = up(f['gslot'], torch.uint8)

    def run_check():
        err = ints(1)
        call('mgv_plan_check_levels', E, ptr(in_src), ptr(in_dst), ptr(gs), ptr(up(f['level'])), ptr(err))
        return (err,)
    eq(twice(run_check)[0], [0], 'err')

    order, key_start = twice(lambda: run_count_sort(f['key'], N, K))
    n_active = f['n_active']
    eq(order, f['order'], 'order')                       # (behind the n_active updated nodes nothing is written)
    eq(key_start, f['key_start'], 'key_start')
    want = R.tiles(f['key_start'], f['order'], f['in_ptr'], f['out_ptr'], T, L)
    ks, od = up(f['key_start']), up(f['order'])

    def run_counts():
        ntile, tile_first, scan = ints(K), ints(K + 1), ints(K // 2048 + 2)
        call('mgv_plan_tile_counts', K, ptr(ks), ptr(ntile), ptr(tile_first), ptr(scan))
        return ntile, tile_first
    ntile, tile_first = twice(run_counts)
    eq(ntile, want[0], 'ntile'); eq(tile_first, want[1], 'tile_first')
    num_tiles = int(want[1][-1])
    assert num_tiles == f['num_tiles']
    tf = up(want[1])

    def run_tiles():
        t_start, t_count, t_slot, span, ltp = ints(num_tiles), ints(num_tiles), ints(num_tiles), ints(4 * n_active), ints(L + 1)
        call('mgv_plan_tiles', K, T, L, n_active, ptr(ks), ptr(tf), ptr(od), ptr(in_ptr), ptr(out_ptr), ptr(t_start), ptr(t_count), ptr(t_slot),
             ptr(span), ptr(ltp))
        return t_start, t_count, t_slot, span, ltp
    for name, got, w in zip(('tile_start', 'tile_count', 'tile_slot', 'order_span', 'level_tile_ptr'), twice(run_tiles), want[2:]):
        eq(got, w, name)
    assert f['level_tile_ptr'][8] == f['level_tile_ptr'][9]                                       # (the empty level: a repeated pointer)

    def run_rows():
        rows = ints(32 * n_active)
        call('mgv_plan_order_rows', n_active, ptr(od), ptr(in_ptr), ptr(in_src), ptr(out_ptr), ptr(out_dst), ptr(out_slot), ptr(gs), ptr(rows))
        return (rows,)
    eq(twice(run_rows)[0], f['order_rows'], 'order_rows')
    # the tiles grouped by slot: the second counting sort of the chain (a slot without a tile keeps an empty run)
    st, sstart = twice(lambda: run_count_sort(f['tile_slot'], num_tiles, T))
    eq(st, f['slot_tiles'], 'slot_tiles'); eq(sstart, f['slot_tile_ptr'], 'slot_tile_ptr')


def test_check_levels_cases():
    """mgv_plan_check_levels: an equal-level edge into an updated node is 2, the same edge into a node that is never updated is 0, no
    edges is 0."""
    _dev()
    level = up([0, 1, 1, 2])

    def err(in_src, in_dst, gslot):
        def run():
            e = ints(1)
            call('mgv_plan_check_levels', len(in_src), ptr(up(in_src)), ptr(up(in_dst)), ptr(up(gslot, torch.uint8)), ptr(level), ptr(e))
            return (e,)
        out = twice(run)[0]
        eq(out, [R.check_levels(in_src, in_dst, gslot, [0, 1, 1, 2])])
        return int(out[0].item())
    assert err([0, 1, 0], [1, 2, 3], [255, 0, 0, 1]) == 2
    assert err([0, 1, 0], [1, 2, 3], [255, 0, 255, 1]) == 0
    assert err([0, 0, 2], [1, 2, 3], [255, 0, 0, 1]) == 0
    assert err([3], [1], [255, 0, 0, 1]) == 2                                                     # a source on a HIGHER level
    assert err([], [], [255, 0, 0, 1]) == 0


def test_count_sort_cases():
    """mgv_count_sort_i32: every key -1 leaves key_start all zero and `order` untouched; K = 8192 with n = 2,049 runs three blocks of
    full-width histograms."""
    _dev()
    order, key_start = twice(lambda: run_count_sort(np.full(700, -1), 700, 5))
    eq(key_start, np.zeros(6), 'key_start'); untouched(order, 0, 'order')
    key = np.random.Generator(np.random.PCG64(14)).integers(-1, 8192, size=2049)
    key[5:40] = 8191
    key[2040:] = 0
    want = R.count_sort(key, 8192)
    order, key_start = twice(lambda: run_count_sort(key, 2049, 8192))
    eq(order, want[0], 'order'); eq(key_start, want[1], 'key_start')


# ------------------------------------------------------------------------------------------------ mgv_plan_pairs
def run_pairs(in_ptr, xcls, N):
    present, rank, scan = ints(65537), ints(65537), ints(65536 // 2048 + 2)
    cid, cls_deg, cls_x, status = ints(N), ints(65536), octets(65536), ints(1)
    call('mgv_plan_pairs', N, ptr(up(in_ptr)), ptr(up(xcls, torch.uint8)), ptr(present), ptr(rank), ptr(scan), ptr(cid), ptr(cls_deg), ptr(cls_x),
         ptr(status))
    return cid, rank[65536:65537].clone(), cls_deg, cls_x, status


@pytest.mark.parametrize('extra', [None, 256])
def test_pairs_over_every_degree(extra):
    """mgv_plan_pairs: in-degrees 0..255 with classes {0, 1, 255}; one node of degree 256 more gives status 3, and its id is still the
    number of a pair of the table.  cls_deg / cls_x behind C stay untouched."""
    _dev()
    src, dst, N, x = R.degree_graph(extra)
    in_ptr = R.csr(src, dst, N)[0]
    cid, C, cls_deg, cls_x, status = twice(lambda: run_pairs(in_ptr, x, N))
    w_cid, w_C, w_deg, w_x, w_status = R.pairs(in_ptr, x)
    assert w_status == (3 if extra else 0) and w_C == 256
    eq(status, [w_status], 'status'); assert int(C.item()) == w_C
    eq(cid, w_cid, 'cid'); eq(cls_deg, w_deg, 'cls_deg'); eq(cls_x, w_x, 'cls_x')
    assert 0 <= int(cid[:N].min()) and int(cid[:N].max()) < w_C


@pytest.mark.parametrize('case', ['plain', 'degree256', 'too_many'])
def test_first_stage_classes_on_the_device_plan(case, monkeypatch):
    """GraphPlan.first_stage_classes on the device plan: the table of the pair kernels, the fallback at an in-degree above 255 (the
    torch composition on the device CSR), and None when there are more pairs than max_classes."""
    dev = _dev()
    from deepgate.graph_plan import GraphPlan
    monkeypatch.setenv('MGV_PLAN', 'hip')
    src, dst, N, x = R.degree_graph(256 if case == 'degree256' else None)
    if case == 'plain':
        keep = dst < 100
        src, dst = src[keep], dst[keep]
    plan = GraphPlan(torch.from_numpy(np.stack([src, dst])).to(dev), N)
    assert plan.hip
    cap = 200 if case == 'too_many' else 512
    got = plan.first_stage_classes(torch.from_numpy(x).to(dev), max_classes=cap)
    want = R.first_stage(R.csr(src, dst, N)[0], x, cap)
    assert (want is None) == (case == 'too_many') and (got is None) == (want is None)
    if want is not None:
        assert got[1] == want[1]
        for k in (0, 2, 3, 4):
            assert torch.equal(got[k].cpu().long(), torch.from_numpy(np.asarray(want[k], dtype=np.int64))), k


# ------------------------------------------------------------------------------------------------ GraphPlan.set_levels and its fallback
@pytest.mark.parametrize('n', [4096, 4097])
def test_set_levels_at_the_key_limit(n, monkeypatch):
    """GraphPlan.set_levels with two slots: 4,096 levels are K = 8,192 keys, the counting sort's limit (the HIP path); 4,097 levels are
    8,194 and take the torch composition on the HIP-built CSR.  Every field and the packed rows equal the restatement."""
    dev = _dev()
    from deepgate.graph_plan import GraphPlan
    monkeypatch.setenv('MGV_PLAN', 'hip')
    src, dst, N, level = R.chain(n)
    gate = (1 + np.arange(N) % 2).astype(np.float32)
    took = []
    real = GraphPlan._set_levels_hip
    monkeypatch.setattr(GraphPlan, '_set_levels_hip', lambda self, *a: (took.append(real(self, *a)), took[-1])[1])
    plan = GraphPlan(torch.from_numpy(np.stack([src, dst])).to(dev), N)
    plan.set_levels(torch.from_numpy(gate).to(dev), torch.from_numpy(level).to(dev), [1, 2])
    assert plan.hip and len(took) == 1 and (took[0] is False) == (n == 4097)
    want = R.plan_fields(src, dst, N, gate, level, [1, 2])
    assert want['num_levels'] * 2 == (8192 if n == 4096 else 8194)
    for name in ['in_ptr', 'in_src', 'in_dst', 'out_ptr', 'out_dst', 'out_slot', 'gslot', 'level', 'num_levels', 'order', 'order_span', 'order_rows',
                 'tile_start', 'tile_count', 'tile_slot', 'slot_tiles', 'slot_tile_ptr', 'level_tile_ptr', 'num_tiles', 'n_active', 'num_slots']:
        a, b = getattr(plan, name), want[name]
        if torch.is_tensor(a):
            b = np.asarray(b, dtype=np.int64)
            assert tuple(a.shape) == b.shape, (name, a.shape, b.shape)
            assert torch.equal(a.cpu().long(), torch.from_numpy(b)), name
        else:
            assert a == b, name


@pytest.mark.parametrize('levels', [[0, 1, 1, 2, 0], [0, 0, 0, 0, 0]])
def test_a_levelised_plan_without_edges(levels, monkeypatch):
    """GraphPlan.set_levels / order_rows on the device with E = 0 (the CSR payloads are empty tensors, which have no address): updated
    nodes whose spans are all empty, and no updated node at all (no tile, no row)."""
    dev = _dev()
    from deepgate.graph_plan import GraphPlan
    monkeypatch.setenv('MGV_PLAN', 'hip')
    none = np.zeros(0, dtype=np.int64)
    gate, level = np.array([1, 1, 2, 1, 7], dtype=np.float32), np.array(levels, dtype=np.int64)
    plan = GraphPlan(torch.zeros(2, 0, dtype=torch.int64, device=dev), 5)
    plan.set_levels(torch.from_numpy(gate).to(dev), torch.from_numpy(level).to(dev), [1, 2])
    want = R.plan_fields(none, none, 5, gate, level, [1, 2])
    assert plan.hip and plan.n_active == want['n_active'] == (3 if max(levels) else 0) and plan.num_tiles == want['num_tiles']
    assert plan.level_tile_ptr == want['level_tile_ptr'] and plan.slot_tile_ptr == want['slot_tile_ptr']
    for name in ('gslot', 'level', 'order', 'order_span', 'order_rows', 'tile_start', 'tile_count', 'tile_slot', 'slot_tiles'):
        a, b = getattr(plan, name), np.asarray(want[name], dtype=np.int64)
        assert tuple(a.shape) == b.shape and torch.equal(a.cpu().long(), torch.from_numpy(b)), name


# ------------------------------------------------------------------------------------------------ mgv_colour_keys / mgv_colour_check
def _coloured():
    c = R.coloured_lists()
    dev = {k: up(c[k]) for k in ('ptr', 'idx', 'prev')}
    dev['xcls'] = up(c['xcls'], torch.uint8)
    return c, dev


@pytest.mark.parametrize('bits', [16, 63])
def test_colour_keys_equal_the_documented_formula(bits):
    """mgv_colour_keys on the designed lists: the device keys equal the documented formula evaluated in Python integers mod 2^64, lie
    in [0, 2^key_bits), agree on equal signatures, and at 63 bits differ on the designed distinct ones."""
    _dev()
    c, d = _coloured()
    f = R.colour_f(c['Cp'])
    N = c['N']
    fd = up(f, torch.int64)

    def run():
        key = torch.full((N + GUARD,), SENT, dtype=torch.int64, device='cuda:0')
        call('mgv_colour_keys', N, ptr(d['ptr']), ptr(d['idx']), ptr(d['prev']), ptr(fd), c['Cp'] + 1, ptr(d['xcls']), bits, ptr(key))
        return (key,)
    key = twice(run)[0]
    want = R.colour_keys(c['ptr'], c['idx'], c['prev'], f, c['xcls'], bits)
    assert key[:N].cpu().tolist() == want and bool((key[N:] == SENT).all())
    assert all(0 <= k < (1 << bits) for k in want)
    cid, rep = R.true_grouping(c['ptr'], c['idx'], c['prev'], c['xcls'])
    assert all(want[i] == want[rep[cid[i]]] for i in range(N))
    if bits == 63:
        assert len(set(want)) == rep.size


def test_colour_check_on_single_differences():
    """mgv_colour_check: the true grouping passes and counts the members whose lists of more than 48 entries it left to the caller
    (flags[1], never produced by another test); a pair merged across ONE difference — a neighbour colour, the class, the previous
    colour, the degree — is refuted at list lengths up to 48; the one-colour difference at length 49 is not looked at but counted,
    and GraphPlan._colour_lists_equal, the caller's sort-based check, finds it."""
    dev = _dev()
    from deepgate.graph_plan import GraphPlan
    c, d = _coloured()
    N = c['N']
    cid, rep = R.true_grouping(c['ptr'], c['idx'], c['prev'], c['xcls'])
    rep_d = up(rep)

    def flags(grouping):
        cid_d = up(grouping)

        def run():
            fl = ints(2)
            fl[:2] = 0                                   # (zeroed by the caller)
            call('mgv_colour_check', N, ptr(d['ptr']), ptr(d['idx']), ptr(d['prev']), ptr(d['xcls']), ptr(cid_d), ptr(rep_d), ptr(fl))
            return (fl,)
        out = twice(run)[0]
        eq(out, R.colour_check(c['ptr'], c['idx'], c['prev'], c['xcls'], grouping, rep))
        return out[:2].tolist()
    n_long = sum(1 for i in range(N) if rep[cid[i]] != i and c['ptr'][i + 1] - c['ptr'][i] > 48)
    assert flags(cid) == [0, n_long] and n_long == 2
    for name in ('colour48', 'class', 'prev', 'degree'):
        a, b = c['pairs'][name]
        merged = cid.copy()
        merged[b] = merged[a]
        assert flags(merged)[0] == 1, name
    a, b = c['pairs']['colour49']
    merged = cid.copy()
    merged[b] = merged[a]
    assert flags(merged) == [0, n_long + 1]
    plan = GraphPlan(torch.tensor([[0], [1]], device=dev), 2)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(dev)
    owner = t(np.repeat(np.arange(N), np.diff(c['ptr'])))
    assert plan._colour_lists_equal(t(c['ptr']), t(c['idx']), owner, t(c['prev']), t(cid), t(rep), t(c['xcls']), c['Cp'])
    assert not plan._colour_lists_equal(t(c['ptr']), t(c['idx']), owner, t(c['prev']), t(merged), t(rep), t(c['xcls']), c['Cp'])


# ------------------------------------------------------------------------------------------------ groups, representatives, key counts
def run_groups(skey, by, N):
    cid, starts, rep, n_col = ints(N), ints(N + 1), ints(N), ints(1)
    n_s = 2 * N + N // 2048 + 66
    scratch = ints(n_s)
    call('mgv_colour_groups', N, ptr(up(skey, torch.int64)), ptr(up(by)), ptr(cid), ptr(starts), ptr(rep), ptr(n_col), ptr(scratch), n_s)
    untouched(scratch, n_s)
    return cid, starts, rep, n_col


@pytest.mark.parametrize('case', ['one', 'equal512', 'equal513', 'distinct512', 'distinct513', 'last_run_of_one', 'designed'])
def test_colour_groups(case):
    """mgv_colour_groups: runs of equal sorted keys -> cid, starts[C + 1], rep[C], C; starts[C + 1 .. N] and rep[C .. N) stay untouched."""
    _dev()
    rng = np.random.Generator(np.random.PCG64(15))
    if case == 'designed':
        c = R.coloured_lists()
        key = np.array(R.colour_keys(c['ptr'], c['idx'], c['prev'], R.colour_f(c['Cp']), c['xcls'], 63), dtype=np.int64)
        by = np.argsort(key, kind='stable')
        skey = key[by]
    else:
        N = {'one': 1, 'last_run_of_one': 777}.get(case, int(case[-3:]) if case[-1].isdigit() else 0)
        if case.startswith('equal') or case == 'one':
            skey = np.full(N, (1 << 62) + 5, dtype=np.int64)
        elif case.startswith('distinct'):
            skey = np.cumsum(rng.integers(1, 1000, size=N)).astype(np.int64) << 22
        else:
            skey = np.sort(np.concatenate([rng.integers(0, 50, size=N - 1), [1 << 61]])).astype(np.int64)
        by = rng.permutation(N)
    N = skey.size
    cid, starts, rep, n_col = twice(lambda: run_groups(skey, by, N))
    w_cid, w_starts, w_rep, C = R.colour_groups(skey, by)
    eq(n_col, [C], 'n_colours'); eq(cid, w_cid, 'cid'); eq(starts, w_starts, 'starts'); eq(rep, w_rep, 'rep')
    assert C == {'one': 1, 'equal512': 1, 'equal513': 1, 'distinct512': 512, 'distinct513': 513}.get(case, C)
    if case == 'last_run_of_one':
        assert w_starts[-2] == N - 1


@pytest.mark.parametrize('heavy_row', [49, 48])
def test_representatives_rows_and_lists(heavy_row):
    """mgv_colour_rep_rows / mgv_colour_rep_lists on the designed lists: heavy_row at a representative's exact degree (49: not heavy)
    and one below it."""
    _dev()
    c, d = _coloured()
    cid, rep = R.true_grouping(c['ptr'], c['idx'], c['prev'], c['xcls'])
    C = rep.size
    rep_d = up(rep)

    def run_rows():
        rptr, own, xrep, n_heavy = ints(C + 1), ints(C), octets(C), ints(1)
        n_s = C + C // 2048 + 66
        scratch = ints(n_s)
        call('mgv_colour_rep_rows', C, ptr(rep_d), ptr(d['ptr']), ptr(d['prev']), ptr(d['xcls']), heavy_row, ptr(rptr), ptr(own), ptr(xrep), ptr(n_heavy),
             ptr(scratch), n_s)
        untouched(scratch, n_s)
        return rptr, own, xrep, n_heavy
    want = R.rep_rows(C, rep, c['ptr'], c['prev'], c['xcls'], heavy_row)
    for name, got, w in zip(('rptr', 'own', 'xrep', 'n_heavy'), twice(run_rows), want[:3] + ([want[3]],)):
        eq(got, w, name)
    assert want[3] == (1 if heavy_row == 49 else 4)
    rptr_d, n_ent = up(want[0]), int(want[0][-1])

    def run_lists():
        ent, row = ints(n_ent), ints(n_ent)
        call('mgv_colour_rep_lists', C, ptr(rep_d), ptr(d['ptr']), ptr(d['idx']), ptr(d['prev']), ptr(rptr_d), ptr(ent), ptr(row))
        return ent, row
    ent, row = twice(run_lists)
    w_ent, w_row = R.rep_lists(C, rep, c['ptr'], c['idx'], c['prev'])
    eq(ent, w_ent, 'ent'); eq(row, w_row, 'row')


def test_representatives_of_a_single_node():
    """mgv_colour_rep_rows / mgv_colour_rep_lists at C = 1: a node with two entries, heavy_row at its degree and below."""
    _dev()
    ptr_d, idx_d, prev_d, x_d, rep_d = up([0, 2]), up([0, 0]), up([6]), up([3], torch.uint8), up([0])
    for heavy_row, heavy in ((2, 0), (1, 1)):
        rptr, own, xrep, n_heavy, scratch = ints(2), ints(1), octets(1), ints(1), ints(67)
        call('mgv_colour_rep_rows', 1, ptr(rep_d), ptr(ptr_d), ptr(prev_d), ptr(x_d), heavy_row, ptr(rptr), ptr(own), ptr(xrep), ptr(n_heavy), ptr(scratch), 67)
        want = R.rep_rows(1, [0], [0, 2], [6], [3], heavy_row)
        eq(rptr, want[0]); eq(own, want[1]); eq(xrep, want[2]); eq(n_heavy, [heavy]); untouched(scratch, 67)
        assert want[3] == heavy
    ent, row = ints(2), ints(2)
    call('mgv_colour_rep_lists', 1, ptr(rep_d), ptr(ptr_d), ptr(idx_d), ptr(prev_d), ptr(up([0, 2])), ptr(ent), ptr(row))
    eq(ent, [6, 6]); eq(row, [0, 0])


@pytest.mark.parametrize('case', ['empty', 'absent_ends', 'wide'])
def test_sorted_key_counts(case):
    """mgv_sorted_key_counts: no keys at all; keys absent at both ends of [0, K); K larger than the largest key + 1."""
    _dev()
    rng = np.random.Generator(np.random.PCG64(16))
    if case == 'empty':
        keys, K = np.zeros(0, dtype=np.int64), 300
    elif case == 'absent_ends':
        keys, K = np.sort(rng.integers(3, 290, size=1000)), 300
    else:
        keys, K = np.sort(rng.integers(0, 40, size=513)), 700

    def run():
        counts = ints(K)
        call('mgv_sorted_key_counts', keys.size, ptr(up(keys)) if keys.size else None, K, ptr(counts))
        return (counts,)
    eq(twice(run)[0], R.sorted_key_counts(keys, K))


# ------------------------------------------------------------------------------------------------ mgv_seg_level_scan / _fill
def run_seg_level(counts, gid, seg, base, with_rows, with_next):
    G = len(counts)
    w_i = value('mgv_seg_level_work_ints', G)
    work = ints(w_i)
    cd = up(counts)
    call('mgv_seg_level_scan', G, ptr(cd), seg, ptr(work), w_i)
    totals = work[:4].tolist()
    untouched(work, w_i, 'work')
    n_seg, g_next = totals[0], totals[3]
    seg_ptr, out_row, gid_n, counts_n = ints(n_seg + 1), ints(n_seg), ints(g_next), ints(g_next)
    gd = up(gid) if gid is not None else None
    call('mgv_seg_level_fill', G, n_seg, ptr(gd), seg, base, ptr(work), ptr(seg_ptr), ptr(out_row) if with_rows else None,
         ptr(gid_n) if with_next else None, ptr(counts_n) if with_next else None)
    return work[:4].clone(), seg_ptr, out_row, gid_n, counts_n


def check_seg_level(counts, gid, seg, base, with_rows=True, with_next=True):
    got = twice(lambda: run_seg_level(counts, gid, seg, base, with_rows, with_next))
    totals, seg_ptr, out_row, gid_n, counts_n = R.seg_level(counts, gid, seg, base)
    assert got[0].tolist() == totals
    eq(got[1], seg_ptr, 'seg_ptr')
    if with_rows:
        eq(got[2], out_row, 'out_row')
    else:
        untouched(got[2], 0, 'out_row')
    if with_next:
        eq(got[3], gid_n, 'gid_next'); eq(got[4], counts_n, 'counts_next')
    return totals


@pytest.mark.parametrize('seg', [64, 2])
def test_seg_level_on_designed_counts(seg):
    """mgv_seg_level_scan / mgv_seg_level_fill: colours with 0, 1, seg, seg + 1, seg^2 and seg^2 + 1 members; gid NULL and given;
    out_row NULL and given; a level where no colour has more than one segment, with the next-level pair NULL."""
    _dev()
    counts = [0, 1, seg, seg + 1, seg * seg, seg * seg + 1, 3 % (seg + 1), 0]
    G = len(counts)
    totals = check_seg_level(counts, None, seg, G)
    assert totals[3] == 3 and totals[2] == 2 + seg + seg + 1
    check_seg_level(counts, None, seg, G, with_rows=False)
    gid = [5, 9, 11, 2, 40, 41, 7, 0]
    check_seg_level(counts, gid, seg, 100)
    single = [0, 1, seg, 1, 0, seg - 1]
    assert check_seg_level(single, None, seg, len(single), with_next=False)[2:] == [0, 0]
    check_seg_level(single, [3, 1, 4, 1, 5, 9], seg, 50, with_rows=True, with_next=False)


@pytest.mark.parametrize('extra', [0, 1])
def test_seg_level_at_the_one_workgroup_limit(extra):
    """65,536 colours are the last size of the one-workgroup level kernel, 65,537 (the same counts and one colour more) the first of
    the multi-kernel level: the tables of both equal the restatement."""
    _dev()
    rng = np.random.Generator(np.random.PCG64(17))
    counts = rng.integers(0, 6, size=65537)
    counts[::4099] = 200
    counts = counts[:65536 + extra]
    G = counts.size
    check_seg_level(counts, None, 2, G)
    check_seg_level(counts, rng.permutation(G), 64, 2 * G)
