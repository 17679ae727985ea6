"""Host side of the batch builder (no GPU).  tests/plan_ref.py — the integer restatement tests/test_hip_plan_entries.py holds every
entry of csrc/plan_build.hip to — equals the host implementations that exist already, on every designed input and on the recorded
loader fixture: GraphPlan on CPU tensors (the torch composition: CSR, set_levels, order_rows, first_stage_classes, class_sum_levels),
parser.forward_levels and the fixture's forward_level / backward_level.  The designed inputs discriminate: a deliberately wrong
variant of the RESTATEMENT (never of a kernel) differs from the right one on them, family by family.  And the argument checks of
the plan entries return MGV_EINVAL / MGV_OK before any launch: the pointers are distinct non-NULL dummies that are never
dereferenced (as in tests/test_seg_lists_spec.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import plan_ref as R
from conftest import GOLDEN
from deepgate import _hip
from deepgate.graph_plan import GraphPlan
from deepgate.parser import forward_levels

OK, EINVAL = 0, -1
CSR = ['in_ptr', 'in_src', 'in_dst', 'out_ptr', 'out_dst', 'out_slot']
LEVELS = ['gslot', 'level', 'num_levels', 'order', 'order_span', 'order_rows', 'tile_start', 'tile_count', 'tile_slot', 'slot_tiles', 'slot_tile_ptr',
          'level_tile_ptr', 'num_tiles', 'n_active', 'num_slots']


def _same(plan, want, names):
    for n in names:
        a, b = getattr(plan, n), want[n]
        if torch.is_tensor(a):
            a = a.numpy()
            if a.dtype == np.uint8:
                a = a.astype(np.int64)
            assert a.shape == np.asarray(b).shape, (n, a.shape, np.asarray(b).shape)
            assert np.array_equal(a.astype(np.int64), b), n
        else:
            assert a == b, (n, a, b)


def _fixture():
    z = np.load(os.path.join(GOLDEN, 'g6_loader.npz'))
    out = {}
    for tag, gate_ids in (('aig', [1, 2]), ('xmg', [1, 2, 3, 4, 5])):
        ei, x = z[tag + '_edge_index'], z[tag + '_x']
        gate = z['xmg_gate'].reshape(-1) if tag == 'xmg' else z['aig_in_x'][:, 1].astype(np.float32)
        out[tag] = dict(src=ei[0], dst=ei[1], N=x.shape[0], gate=gate, level=z[tag + '_forward_level'], gate_ids=gate_ids, T=len(gate_ids),
                        backward=z[tag + '_backward_level'])
    return out


def _chain_graph(n):
    src, dst, N, level = R.chain(n)
    return dict(src=src, dst=dst, N=N, gate=(1 + np.arange(N) % 2).astype(np.float32), level=level, gate_ids=[1, 2], T=2)


def _levelled():
    out = {'dag%d' % T: R.levelled_dag(T) for T in (1, 2, 5)}
    out.update({'chain%d' % n: _chain_graph(n) for n in (512, 513, 4096, 4097)})
    out.update({'fixture_' + k: v for k, v in _fixture().items()})
    return out


LEVELLED = _levelled()
LISTS = {'lists%d' % N: R.lists_graph(N) for N in (1, 1501, 2048)}


def _plan(src, dst, N):
    return GraphPlan(torch.from_numpy(np.stack([src, dst]).astype(np.int64)), N)


# ------------------------------------------------------------------------------------------------ the designed inputs are what they say
def test_lists_graph_is_the_one_described():
    for name in ('lists1501', 'lists2048'):
        src, dst, N = LISTS[name]
        c = dict(zip(R.CSR_FIELDS, R.csr(src, dst, N)))
        assert tuple(np.diff(c['in_ptr'])[:13]) == R.LIST_LENGTHS and tuple(np.diff(c['out_ptr'])[:13]) == R.LIST_LENGTHS
        assert N <= 4096 and c['status'] == 0 and int((src == dst).sum()) > 20
        pair = src * N + dst
        assert np.unique(pair).size < pair.size and not np.array_equal(pair, np.sort(pair))      # parallel edges, shuffled
    assert LISTS['lists2048'][2] % 256 == 0 and LISTS['lists1'][2] == 1


@pytest.mark.parametrize('T', [1, 2, 5])
def test_levelled_dag_is_the_one_described(T):
    g = LEVELLED['dag%d' % T]
    f = R.plan_fields(g['src'], g['dst'], g['N'], g['gate'], g['level'], g['gate_ids'])
    pop = np.diff(f['key_start']).reshape(-1, T)
    assert set(pop.reshape(-1).tolist()) == set(R.POPULATIONS)
    assert pop[8].sum() == 0 and pop[9].sum() == 1 and pop[10].sum() == 0 and f['num_levels'] == 11       # an empty level inside; the deepest node never updated
    assert f['level_tile_ptr'][8] == f['level_tile_ptr'][9] and f['bad_levels'] == 0
    if T > 1:
        assert pop[:, T - 1].sum() == 0 and T - 1 not in set(f['tile_slot'].tolist())                     # a slot with no node, no tile
    assert set(R.ODD_GATES) <= set(g['gate'].tolist())
    lv0 = g['level'] == 0
    assert (g['gate'][lv0] == g['gate_ids'][0]).any() and (f['gslot'][lv0] == R.NO_GATE).all()            # level 0 of an active type: never updated
    indeg = np.diff(f['in_ptr'])[f['order']]
    assert {4, 5} <= set(indeg.tolist())
    for cnt, node in g['consumers'].items():
        a, b = f['out_ptr'][node], f['out_ptr'][node + 1]
        assert b - a == cnt and f['gslot'][node] != R.NO_GATE
        if cnt:
            first = f['gslot'][f['out_dst'][a:a + 8]]
            assert (first == R.NO_GATE).any() and (first != R.NO_GATE).any()                             # 0xff bytes beside real ones
    assert np.array_equal(R.levels(f['in_ptr'], f['out_ptr'], f['out_dst'], g['N'] + 1)[0] >= 0, np.ones(g['N'], dtype=bool))


def test_coloured_lists_are_the_ones_described():
    c = R.coloured_lists()
    sig = lambda i: R.colour_signature(i, c['ptr'], c['idx'], c['prev'], c['xcls'])
    for d in R.PAIR_LENGTHS:
        a, b = c['pairs']['equal%d' % d]
        assert sig(a) == sig(b) and sig(a)[2] == d
        if d > 1:
            assert list(c['idx'][c['ptr'][a]:c['ptr'][a + 1]]) != list(c['idx'][c['ptr'][b]:c['ptr'][b + 1]])
    for d in (48, 49):
        sa, sb = (sig(i) for i in c['pairs']['colour%d' % d])
        assert sa[:3] == sb[:3] and sa[2] == d and set(sa[3]) == set(sb[3])
        assert sum(x != y for x, y in zip(sa[3], sb[3])) == 1                                                # one neighbour colour
    for name, k in (('class', 0), ('prev', 1), ('degree', 2)):
        sa, sb = (sig(i) for i in c['pairs'][name])
        assert [j for j in range(3) if sa[j] != sb[j]] == [k] and (k == 2 or sa[3] == sb[3])


# ------------------------------------------------------------------------------------------------ restatement = torch composition
@pytest.mark.parametrize('name', sorted(LISTS) + sorted(LEVELLED))
def test_csr_equals_the_torch_composition(name):
    src, dst, N = LISTS[name] if name in LISTS else (LEVELLED[name][k] for k in ('src', 'dst', 'N'))
    plan = _plan(src, dst, N)
    want = dict(zip(R.CSR_FIELDS, R.csr(src, dst, N)))
    assert not plan.hip and want['status'] == 0
    _same(plan, want, CSR)
    assert np.array_equal(plan.perm_in.numpy(), want['in_eid'])
    assert np.array_equal(want['out_eid'], np.argsort(src, kind='stable'))
    rng = np.random.Generator(np.random.PCG64(0))                # a list in any order, sorted, is the stable order again
    mixed = [rng.permutation(want['in_eid'][a:b]) for a, b in zip(want['in_ptr'][:-1], want['in_ptr'][1:])]
    assert np.array_equal(R.sort_lists(want['in_ptr'], np.concatenate(mixed) if mixed else []), want['in_eid'])


@pytest.mark.parametrize('name', sorted(LEVELLED))
def test_levelled_fields_equal_the_torch_composition(name):
    g = LEVELLED[name]
    plan = _plan(g['src'], g['dst'], g['N'])
    plan.set_levels(torch.from_numpy(np.asarray(g['gate'], dtype=np.float32)), torch.from_numpy(np.asarray(g['level'], dtype=np.int64)), g['gate_ids'])
    want = R.plan_fields(g['src'], g['dst'], g['N'], g['gate'], g['level'], g['gate_ids'])
    _same(plan, want, CSR + LEVELS)
    assert want['bad_levels'] == 0
    if name.startswith('chain'):
        assert want['num_levels'] * 2 == {'chain512': 1024, 'chain513': 1026, 'chain4096': 8192, 'chain4097': 8194}[name]


@pytest.mark.parametrize('name', sorted(LEVELLED))
def test_levels_equal_the_host_levelisation_and_the_fixture(name):
    g = LEVELLED[name]
    c = dict(zip(R.CSR_FIELDS, R.csr(g['src'], g['dst'], g['N'])))
    lv, done = R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], g['N'] + 1)
    assert done == g['N']
    assert np.array_equal(lv, forward_levels(np.stack([g['src'], g['dst']]), g['N']))
    assert np.array_equal(lv, _plan(g['src'], g['dst'], g['N']).asap_levels().numpy())
    if name.startswith('chain') or name.startswith('fixture'):
        assert np.array_equal(lv, np.asarray(g['level'], dtype=np.int64))
    if name.startswith('fixture'):
        c = dict(zip(R.CSR_FIELDS, R.csr(g['dst'], g['src'], g['N'])))
        assert np.array_equal(R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], g['N'] + 1)[0], g['backward'].astype(np.int64))
    if name == 'chain513':                               # the `done` contract: nodes on levels below `rounds`
        c = dict(zip(R.CSR_FIELDS, R.csr(g['src'], g['dst'], g['N'])))
        part, done = R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], 512)
        assert done == 512 and np.array_equal(part, lv)  # (the last level's nodes have their level, they are only not counted)
        assert R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], 513)[1] == g['N']


def test_levels_stop_short_of_a_cycle():
    src, dst = np.array([0, 1, 2, 2, 3]), np.array([1, 2, 0, 3, 4])           # a 3-cycle and its tail, and an isolated node
    c = dict(zip(R.CSR_FIELDS, R.csr(src, dst, 6)))
    lv, done = R.levels(c['in_ptr'], c['out_ptr'], c['out_dst'], 7)
    assert done == 1 and lv.tolist() == [-1, -1, -1, -1, -1, 0]
    with pytest.raises(ValueError):
        forward_levels(np.stack([src, dst]), 6)


def _xcls(N, seed=9):
    return np.random.Generator(np.random.PCG64(seed)).choice(np.array([0, 1, 255]), size=N).astype(np.uint8)


@pytest.mark.parametrize('name', sorted(LISTS) + ['dag5', 'fixture_xmg', 'degrees', 'degree256'])
def test_first_stage_classes_equal_the_torch_composition(name):
    if name.startswith('degree'):
        src, dst, N, x = R.degree_graph(256 if name == 'degree256' else None)
    else:
        src, dst, N = LISTS[name] if name in LISTS else (LEVELLED[name][k] for k in ('src', 'dst', 'N'))
        x = _xcls(N)
    plan = _plan(src, dst, N)
    in_ptr = R.csr(src, dst, N)[0]
    xt = torch.from_numpy(x)
    for cap in (256, 1 << 15, 3):                        # (one tensor, three caps: the cap is part of the cache's key)
        got, want = plan.first_stage_classes(xt, max_classes=cap), R.first_stage(in_ptr, x, cap)
        assert (got is None) == (want is None), cap
        if want is not None:
            assert got[1] == want[1]
            for u, v in zip((got[0], got[2], got[3], got[4]), (want[0], want[2], want[3], want[4])):
                assert np.array_equal(u.numpy().astype(np.int64), v)
    cid, C, cls_deg, cls_x, status = R.pairs(in_ptr, x)
    assert status == (3 if int(np.diff(in_ptr).max()) > 255 else 0) and 0 <= cid.min() and cid.max() <= C - (status == 0)     # (a degree above 255: up to C)
    if status == 0:                                      # below degree 256 the kernel's table IS the first stage
        want = R.first_stage(in_ptr, x, 1 << 16)
        assert C == want[1] and np.array_equal(cid, want[0]) and np.array_equal(cls_deg, np.diff(want[2])) and np.array_equal(cls_x, want[4])
    if name == 'degrees':
        assert set(np.diff(in_ptr)[:256].tolist()) == set(range(256))


def test_the_table_cache_hits_on_objects_and_drops_the_level_derived_kinds():
    """GraphPlan.cache on dag5: an entry hits only for the very tensors its key was derived from (equal contents under another
    identity miss) and then returns the stored object; set_levels drops exactly the kinds declared level-derived where they are
    built; the cap is part of first_stage_classes' key (256, 32768 and 3 in a row: three right answers without a reset)."""
    g = LEVELLED['dag5']
    plan = _plan(g['src'], g['dst'], g['N'])
    gate, level = torch.from_numpy(np.asarray(g['gate'], dtype=np.float32)), torch.from_numpy(np.asarray(g['level'], dtype=np.int64))
    plan.set_levels(gate, level, g['gate_ids'])
    assert len(plan.cache) == 0 and 'quotient' not in plan.cache and plan.cache.peek('quotient', 2) is None
    x = _xcls(g['N'])
    xt, twin = torch.from_numpy(x), torch.from_numpy(x.copy())
    q = plan.quotient(xt, 2, force=True)
    assert len(q) == 2 and plan.quotient(xt, 2, force=True) is q and plan.cache.peek('quotient', 2) is q
    q2 = plan.quotient(twin, 2, force=True)
    assert q2 is not q and torch.equal(q2[-1]['cid'], q[-1]['cid']) and plan.cache.peek('quotient', 2) is q2
    cid = q[0]['cid']
    tagged = plan.tagged_idx(True, cid)
    assert plan.tagged_idx(True, cid) is tagged and plan.tagged_idx(True, cid.clone()) is not tagged
    entries = plan.seg_entries(q[-1]['rev'], *q[-1]['sum_levels'])
    assert plan.seg_entries(q[-1]['rev'], *q[-1]['sum_levels']) is entries
    order, tables = q[-1]['sum_levels']
    again = plan.seg_entries(q[-1]['rev'], order.clone(), tables)
    assert again is not entries and torch.equal(again[0], entries[0]) and torch.equal(again[1], entries[1])
    in_ptr = R.csr(g['src'], g['dst'], g['N'])[0]
    for cap in (256, 1 << 15, 3):
        got, want = plan.first_stage_classes(xt, max_classes=cap), R.first_stage(in_ptr, x, cap)
        assert (got is None) == (want is None) == (cap == 3), cap
        assert plan.first_stage_classes(xt, max_classes=cap) is got and (want is None or got[1] == want[1])
    assert plan.first_stage_classes(twin) is not plan.first_stage_classes(xt)
    plan.count_self_loops(), plan.heavy(True), plan.heavy_segments(True, active_by_level=True), plan.slot_nodes(), plan.order_rows
    plan.cache.put('sweep_steps', None, 1, level_derived=True)     # (as ops._sweep_rows counts a plan's forward sweeps)
    from deepgate.prefetch import _record_all
    seen = set()
    _record_all(plan.__dict__, None, seen)               # (the prefetcher's walk over a plan's tensors reaches the cached tables and ends there)
    assert id(entries) in seen and len(seen) < 200
    level_derived = {'tagged', 'heavy_segments', 'slot_nodes', 'order_rows', 'sweep_steps'}
    kept = {'quotient', 'seg_entries', 'first_stage', 'self_loops', 'heavy'}
    kinds = lambda: {k for k in level_derived | kept if k in plan.cache}
    assert kinds() == level_derived | kept
    heavy, rows = plan.heavy(True), plan.order_rows
    plan.set_levels(gate, level, g['gate_ids'])
    assert kinds() == kept and plan.heavy(True) is heavy and plan.quotient(twin, 2, force=True) is q2
    assert plan.cache.peek('sweep_steps') is None and plan.order_rows is not rows and torch.equal(plan.order_rows, rows)
    plan.cache.drop('quotient', 'heavy')
    assert kinds() == (kept | {'order_rows'}) - {'quotient', 'heavy'}


SEG_COUNTS = {64: [0, 1, 64, 65, 4096, 4097, 3, 0], 2: [0, 1, 2, 3, 4, 5, 9, 0, 7]}


@pytest.mark.parametrize('seg', [64, 2])
def test_segment_tables_equal_the_torch_composition(seg):
    counts = np.array(SEG_COUNTS[seg], dtype=np.int64)
    C = counts.size
    plan = _plan(np.array([0]), np.array([1]), 2)
    cid = torch.from_numpy(np.repeat(np.arange(C), counts))
    for presorted in (None, (torch.arange(cid.numel()), torch.from_numpy(counts))):
        order, got = plan.class_sum_levels(cid, C, seg=seg, presorted=presorted)
        want = R.sum_levels(counts, seg)
        assert got['C'] == want['C'] and got['rows'] == want['rows'] and len(got['levels']) == len(want['levels'])
        for (na, spa, ora, sra), (nb, spb, orb, srb) in zip(got['levels'], want['levels']):
            assert na == nb and sra == srb and np.array_equal(spa.numpy().astype(np.int64), spb)
            assert (ora is None) == (orb is None) and (ora is None or np.array_equal(ora.numpy().astype(np.int64), orb))
        assert np.array_equal(order.numpy(), np.arange(cid.numel()))
    assert len(want['levels']) == (4 if seg == 2 else 3)
    assert R.sum_levels([2, 0, 1], seg)['levels'][0][2] is None                   # one level, every colour one segment: segment s writes row s


def test_colour_entries_on_a_cpu():
    """The grouping entries chained on the designed lists: keys -> sort -> groups -> check -> representatives' rows and lists; the
    63-bit keys of the designed distinct signatures are distinct (fixed inputs: a fact), equal signatures share a key."""
    c = R.coloured_lists()
    ptr, idx, prev, xcls = c['ptr'], c['idx'], c['prev'], c['xcls']
    f = R.colour_f(c['Cp'])
    cid, rep = R.true_grouping(ptr, idx, prev, xcls)
    for bits in (16, 63):
        key = R.colour_keys(ptr, idx, prev, f, xcls, bits)
        assert all(0 <= k < (1 << bits) for k in key)
        assert all(key[i] == key[rep[cid[i]]] for i in range(c['N']))
    assert len(set(key)) == rep.size                     # 63 bits: one key per signature
    by = np.argsort(np.array(key, dtype=np.int64), kind='stable')
    g_cid, starts, g_rep, C = R.colour_groups([key[i] for i in by], by)
    assert C == rep.size and len(set(zip(cid.tolist(), g_cid.tolist()))) == C and starts[-1] == c['N']
    assert all(g_rep[k] == min(i for i in range(c['N']) if g_cid[i] == k) for k in range(C))
    n_long = sum(1 for i in range(c['N']) if rep[cid[i]] != i and ptr[i + 1] - ptr[i] > R.CHECK_MAX)
    assert R.colour_check(ptr, idx, prev, xcls, cid, rep) == (0, n_long) and n_long == 2
    assert R.colour_check(ptr, idx, prev, xcls, g_cid, g_rep) == (0, n_long)
    # the sort-based check of the torch composition agrees: the true grouping passes, the length-49 merge is found
    plan = _plan(np.array([0]), np.array([1]), 2)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64))
    owner = t(np.repeat(np.arange(c['N']), np.diff(ptr)))
    assert plan._colour_lists_equal(t(ptr), t(idx), owner, t(prev), t(cid), t(rep), t(xcls), c['Cp'])
    for name in ('colour48', 'colour49', 'class', 'prev', 'degree'):
        m = merged(cid, c['pairs'][name])
        assert not plan._colour_lists_equal(t(ptr), t(idx), owner, t(prev), t(m), t(rep), t(xcls), c['Cp']), name
        assert R.colour_check(ptr, idx, prev, xcls, m, rep) == ((0, n_long + 1) if name == 'colour49' else (1, n_long)), name
    rptr, own, xrep, n_heavy = R.rep_rows(C, g_rep, ptr, prev, xcls, 48)
    ent, row = R.rep_lists(C, g_rep, ptr, idx, prev)
    assert rptr[-1] == ent.size == row.size and n_heavy == 4 and R.rep_rows(C, g_rep, ptr, prev, xcls, 49)[3] == 1      # lists LONGER than heavy_row: three of 49 and the 300; the 300
    assert np.array_equal(R.sorted_key_counts(np.sort(ent), c['Cp']), np.bincount(ent, minlength=c['Cp']))


def merged(cid, pair):
    """The grouping with the pair's second node moved into the first node's colour."""
    m = np.array(cid).copy()
    m[pair[1]] = m[pair[0]]
    return m


# ------------------------------------------------------------------------------------------------ the designed inputs discriminate
def test_wrong_variants_of_the_restatement_differ_on_the_designed_inputs():
    src, dst, N = LISTS['lists1501']
    right = R.csr(src, dst, N)
    eid = np.arange(src.size)
    rev_in = np.lexsort((-eid, dst))                      # ties by descending edge id: an unstable order
    assert not np.array_equal(rev_in, right[3]) and not np.array_equal(src[rev_in], right[1])
    for T in (1, 2, 5):
        g = LEVELLED['dag%d' % T]
        f = R.plan_fields(g['src'], g['dst'], g['N'], g['gate'], g['level'], g['gate_ids'])
        tab = R.slot_table(g['gate_ids'])
        L = f['num_levels']
        t64 = R.tiles(f['key_start'], f['order'], f['in_ptr'], f['out_ptr'], T, L)
        t63 = R.tiles(f['key_start'], f['order'], f['in_ptr'], f['out_ptr'], T, L, tile=63)
        assert not np.array_equal(t64[0], t63[0]) and t64[2].size != t63[2].size                           # tile size 63
        assert not np.array_equal(R.keys(g['gate'], g['level'], tab, T, min_level=0)[2], f['key'])          # lv >= 0
        assert not np.array_equal(R.keys(g['gate'], g['level'], tab, T, clamp=False)[0], f['gslot'])        # no gate clamp
        rows = f['order_rows']
        args = (f['order'], f['in_ptr'], f['in_src'], f['out_ptr'], f['out_dst'], f['out_slot'], f['gslot'])
        assert not np.array_equal(R.order_rows(*args, n_src=3), rows) and not np.array_equal(R.order_rows(*args, n_out=7), rows)
        assert np.array_equal(rows[:, 26:], np.full((rows.shape[0], 6), -1))
    # the level check: an equal-level edge into an updated node
    gslot, level = np.array([255, 0, 0]), np.array([0, 1, 1])
    assert R.check_levels([1], [2], gslot, level) == 2 and R.check_levels([1], [2], gslot, level, strict=False) == 0
    assert R.check_levels([1], [0], gslot, level) == 0 and R.check_levels([], [], gslot, level) == 0
    # a degree cap of 254
    src, dst, N, x = R.degree_graph()
    in_ptr = R.csr(src, dst, N)[0]
    assert R.pairs(in_ptr, x)[4] == 0 and R.pairs(in_ptr, x, cap=254)[4] == 3
    assert not np.array_equal(R.pairs(in_ptr, x)[0], R.pairs(in_ptr, x, cap=254)[0])
    # sets instead of multisets
    c = R.coloured_lists()
    cid, rep = R.true_grouping(c['ptr'], c['idx'], c['prev'], c['xcls'])
    m = merged(cid, c['pairs']['colour48'])
    args = (c['ptr'], c['idx'], c['prev'], c['xcls'], m, rep)
    assert R.colour_check(*args)[0] == 1 and R.colour_check(*args, multiset=False)[0] == 0
    # nseg without the max(1, .)
    for seg, counts in SEG_COUNTS.items():
        assert R.seg_level(counts, None, seg, len(counts))[0] != R.seg_level(counts, None, seg, len(counts), at_least_one=False)[0]


# ------------------------------------------------------------------------------------------------ argument refusals
def P(k):
    return ctypes.c_void_p(64 * k)


def _refusals(name, good, bad, ok=()):
    """`good`: ordered (argument name, value) pairs that would pass every check; each of `bad` overrides some and must be refused;
    each of `ok` is an empty problem that returns MGV_OK before a launch."""
    fn = getattr(_hip.load(), name)
    names = [k for k, _ in good]
    for over in bad:
        assert set(over) <= set(names), (name, over)
        args = [over.get(k, v) for k, v in good]
        assert fn(*args, None) == EINVAL, (name, over)
    for over in ok:
        args = [over.get(k, v) for k, v in good]
        assert fn(*args, None) == OK, (name, over)


def _nulls(*names):
    return [{n: None} for n in names]


def test_csr_sort_and_level_refusals():
    q = lambda N, E: _hip.call_value('mgv_plan_csr_scratch_ints', N, E)
    assert q(10, 20) == 2 * 10 + 4 * 20 + 30 // 2048 + 64
    good = [('N', 10), ('E', 20), ('src', P(1)), ('dst', P(2)), ('in_ptr', P(3)), ('in_src', P(4)), ('in_dst', P(5)), ('out_ptr', P(6)),
            ('out_dst', P(7)), ('out_slot', P(8)), ('in_eid', None), ('out_eid', None), ('scratch', P(9)), ('scratch_ints', q(10, 20)), ('status', P(10))]
    _refusals('mgv_plan_csr', good, [{'N': -1}, {'E': -1}, {'N': 1 << 31}, {'E': 1 << 31}, {'scratch_ints': q(10, 20) - 1}]
              + _nulls('in_ptr', 'out_ptr', 'scratch', 'status', 'src', 'dst', 'in_src', 'in_dst', 'out_dst', 'out_slot'))
    good = [('N', 10), ('E', 20), ('ptr', P(1)), ('vals', P(2)), ('scratch', P(3)), ('scratch_ints', 31)]
    _refusals('mgv_sort_lists_i32', good, [{'N': -1}, {'E': -1}, {'scratch_ints': 30}] + _nulls('ptr', 'vals', 'scratch'),
              ok=[{'N': 0}, {'E': 0}, {'N': 0, 'ptr': None, 'scratch': None, 'scratch_ints': 0}, {'E': 0, 'vals': None, 'scratch_ints': 11}])
    good = [('N', 10), ('in_ptr', P(1)), ('out_ptr', P(2)), ('out_dst', P(3)), ('level', P(4)), ('rounds', 5), ('scratch', P(5)), ('scratch_ints', 37),
            ('done', P(6))]
    _refusals('mgv_plan_levels', good, [{'N': -1}, {'rounds': 0}, {'scratch_ints': 36}] + _nulls('in_ptr', 'out_ptr', 'level', 'scratch', 'done'),
              ok=[{'N': 0, 'scratch_ints': 7}])
    good = [('n', 10), ('in', P(1)), ('out', P(2)), ('scratch', P(3))]
    _refusals('mgv_scan_exclusive_i32', good, [{'n': -1}] + _nulls('in', 'out', 'scratch'))


def test_bucket_refusals():
    tab = (ctypes.c_uint8 * 256)(*([255] * 256))
    good = [('N', 10), ('T', 2), ('gate', P(1)), ('level64', P(2)), ('tab', tab), ('gslot', P(3)), ('level32', P(4)), ('key', P(5)), ('maxlevel', P(6))]
    _refusals('mgv_plan_keys', good, [{'N': -1}, {'T': 0}, {'T': 256}] + _nulls('tab', 'maxlevel', 'gate', 'level64', 'gslot', 'level32', 'key'))
    good = [('E', 10), ('in_src', P(1)), ('in_dst', P(2)), ('gslot', P(3)), ('level', P(4)), ('err', P(5))]
    _refusals('mgv_plan_check_levels', good, [{'E': -1}] + _nulls('err', 'in_src', 'in_dst', 'gslot', 'level'))
    q = lambda n, K: _hip.call_value('mgv_count_sort_scratch_ints', n, K)
    assert q(2049, 8192) == 2 * (8192 * 3 + 1) + (8192 * 3 + 1) // 2048 + 64 and q(0, 5) == 2 * 6 + 64
    good = [('n', 10), ('key', P(1)), ('K', 7), ('order', P(2)), ('key_start', P(3)), ('scratch', P(4)), ('scratch_ints', q(10, 7))]
    _refusals('mgv_count_sort_i32', good, [{'n': -1}, {'K': 0}, {'K': 8193, 'scratch_ints': 1 << 20}, {'scratch_ints': q(10, 7) - 1}]
              + _nulls('key_start', 'scratch', 'key', 'order'))
    good = [('K', 6), ('key_start', P(1)), ('ntile', P(2)), ('tile_first', P(3)), ('scan', P(4))]
    _refusals('mgv_plan_tile_counts', good, [{'K': 0}] + _nulls('key_start', 'ntile', 'tile_first', 'scan'))
    good = [('K', 6), ('T', 2), ('L', 3), ('n_active', 10), ('key_start', P(1)), ('tile_first', P(2)), ('order', P(3)), ('in_ptr', P(4)), ('out_ptr', P(5)),
            ('tile_start', P(6)), ('tile_count', P(7)), ('tile_slot', P(8)), ('order_span', P(9)), ('ltp', P(10))]
    _refusals('mgv_plan_tiles', good, [{'K': 0}, {'T': 0}, {'L': 0}, {'K': 7}, {'n_active': -1}]
              + _nulls('key_start', 'tile_first', 'ltp', 'tile_start', 'tile_count', 'tile_slot', 'order', 'in_ptr', 'out_ptr', 'order_span')
              + [{'n_active': 0, 'ltp': None}, {'n_active': 0, 'key_start': None}])
    good = [('n_active', 10), ('order', P(1)), ('in_ptr', P(2)), ('in_src', P(3)), ('out_ptr', P(4)), ('out_dst', P(5)), ('out_slot', P(6)), ('gslot', P(7)),
            ('rows', P(8))]
    _refusals('mgv_plan_order_rows', good, [{'n_active': -1}, {'rows': ctypes.c_void_p(64 + 4)}]
              + _nulls('order', 'in_ptr', 'in_src', 'out_ptr', 'out_dst', 'out_slot', 'gslot', 'rows'),
              ok=[{'n_active': 0}, {'n_active': 0, 'order': None, 'in_src': None, 'rows': None}])
    good = [('N', 10), ('in_ptr', P(1)), ('xcls', P(2)), ('present', P(3)), ('rank', P(4)), ('scan', P(5)), ('cid', P(6)), ('cls_deg', P(7)), ('cls_x', P(8)),
            ('status', P(9))]
    _refusals('mgv_plan_pairs', good, [{'N': 0}, {'N': -1}] + _nulls('in_ptr', 'xcls', 'present', 'rank', 'scan', 'cid', 'cls_deg', 'cls_x', 'status'))


def test_colour_and_segment_refusals():
    good = [('N', 10), ('nbr_ptr', P(1)), ('nbr_idx', P(2)), ('prev', P(3)), ('f', P(4)), ('fstride', 5), ('xcls', P(5)), ('key_bits', 40), ('key', P(6))]
    _refusals('mgv_colour_keys', good, [{'N': -1}, {'key_bits': 15}, {'key_bits': 64}] + _nulls('nbr_ptr', 'nbr_idx', 'prev', 'f', 'xcls', 'key')
              + [{'N': 0, 'nbr_idx': None}], ok=[{'N': 0}])
    good = [('N', 10), ('nbr_ptr', P(1)), ('nbr_idx', P(2)), ('prev', P(3)), ('xcls', P(4)), ('cid', P(5)), ('rep', P(6)), ('flags', P(7))]
    _refusals('mgv_colour_check', good, [{'N': -1}] + _nulls('nbr_ptr', 'nbr_idx', 'prev', 'xcls', 'cid', 'rep', 'flags'), ok=[{'N': 0}])
    need = 2 * 4096 + 2 + 66
    good = [('N', 4096), ('skey', P(1)), ('by', P(2)), ('cid', P(3)), ('starts', P(4)), ('rep', P(5)), ('n_colours', P(6)), ('scratch', P(7)),
            ('scratch_ints', need)]
    _refusals('mgv_colour_groups', good, [{'N': 0}, {'N': -1}, {'scratch_ints': need - 1}]
              + _nulls('skey', 'by', 'cid', 'starts', 'rep', 'n_colours', 'scratch'))
    need = 4096 + 2 + 66
    good = [('C', 4096), ('rep', P(1)), ('nbr_ptr', P(2)), ('prev', P(3)), ('xcls', P(4)), ('heavy_row', 64), ('rptr', P(5)), ('own', P(6)), ('xrep', P(7)),
            ('n_heavy', P(8)), ('scratch', P(9)), ('scratch_ints', need)]
    _refusals('mgv_colour_rep_rows', good, [{'C': 0}, {'scratch_ints': need - 1}]
              + _nulls('rep', 'nbr_ptr', 'prev', 'xcls', 'rptr', 'own', 'xrep', 'n_heavy', 'scratch'))
    good = [('C', 10), ('rep', P(1)), ('nbr_ptr', P(2)), ('nbr_idx', P(3)), ('prev', P(4)), ('rptr', P(5)), ('ent', P(6)), ('row', P(7))]
    _refusals('mgv_colour_rep_lists', good, [{'C': 0}] + _nulls('rep', 'nbr_ptr', 'nbr_idx', 'prev', 'rptr', 'ent', 'row'))
    good = [('n', 10), ('sorted', P(1)), ('K', 5), ('counts', P(2))]
    _refusals('mgv_sorted_key_counts', good, [{'n': -1}, {'K': 0}] + _nulls('counts', 'sorted'))
    w = lambda G: _hip.call_value('mgv_seg_level_work_ints', G)
    assert w(10) == 4 + 30 + 44 + 66 and w(4096) == 4 + 3 * 4096 + 4 * 4097 + 2 + 66
    good = [('G', 10), ('counts', P(1)), ('seg', 64), ('work', P(2)), ('work_ints', w(10))]
    _refusals('mgv_seg_level_scan', good, [{'G': 0}, {'seg': 1}, {'work_ints': w(10) - 1}] + _nulls('counts', 'work'))
    good = [('G', 10), ('n_seg', 12), ('gid', None), ('seg', 64), ('base', 10), ('work', P(1)), ('seg_ptr', P(2)), ('out_row', None), ('gid_next', P(3)),
            ('counts_next', P(4))]
    _refusals('mgv_seg_level_fill', good, [{'G': 0}, {'n_seg': 9}, {'gid_next': None}, {'counts_next': None}] + _nulls('work', 'seg_ptr'))
