"""The block-partition route of the negative sampler (csrc/neg_partition.hip: mgv_neg_partition, the default of
sampling.negative_sampling_device) against tests/neg_sample_ref.py, the numpy restatement of the draw and of its buckets.

Every comparison is integer equality on all five arrays of NegativeEdges.  The shapes are the smallest at which each part can go
wrong: one block of one or two nodes, chunks that end one slot before / at / one slot behind a wave boundary, a block of a million
pairs (finished in trips over node sub-ranges: the status record says so), lists past the one-thread sort and past a trip's capacity,
node counts on either side of a block edge, several hundred chunks with a ragged last one, and a node count whose block count sends
the host to the two-entry route.  Trips and lists finished in their output rows are computed from the restatement's pointer rows
(_trips) and compared with the entry's status record.  63 GPU tests and one CPU test, 5 s on one MI355X."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neg_sample_ref as R  # noqa: E402

PAD = 16                                    # guard entries behind every output and behind the workspace
SENT = -0x5A5A5A5B                          # what the workspace and the outputs hold before the call
BASES = (0, 1234)                           # torch seeds of the surface cases: seed_of(0, 0), and seed_of(1234, 0) with its top bit set
CAP, CHUNK, MAX_BLOCKS, MAX_SHIFT = 16384, 16384, 2048, 12        # csrc/neg_partition.hip
NONE = np.zeros((2, 0), dtype=np.int64)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _dev_arr(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan_from(dev, N, pos):
    from deepgate.graph_plan import GraphPlan
    plan = GraphPlan(_dev_arr(pos, dev), N)
    plan._check_status()
    return plan


def _edge_graph(N, L, seed):
    """Positives around every block edge of an N-node graph with L nodes per block: the nodes L-2 .. L+1 (and the last two nodes) each
    point at 150 random nodes and at their neighbours across the edge, over a sparse random background."""
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, N, size=(2, 2 * N))]
    near = sorted({n for e in range(L, N + L, L) for n in (e - 2, e - 1, e, e + 1) if 0 <= n < N} | {N - 2, N - 1})
    for n in near:
        dst = np.r_[rng.integers(0, N, size=150), [m for m in near if m != n]]
        parts.append(np.stack([np.full(dst.size, n), dst]))
    return np.concatenate(parts, axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> dict(N, E, pos[, shift: the block size the C-ABI run asks for, where the host's own choice would not reach the path])."""
    L = 1 << MAX_SHIFT
    big = R.three_pass_case()
    c = {'2 nodes, no edges, E=%d' % E: dict(N=2, E=E, pos=NONE) for E in (1, 255, 256, 257)}
    c['2 nodes complete (the cap)'] = dict(N=2, E=1000, pos=R.COMPLETE2)
    c['3 nodes, one free pair'] = dict(N=3, E=5000, pos=R.ONE_FREE_OF_3)
    c['one block of a million pairs'] = dict(N=64, E=1000000, pos=R.tiny_graph(64, 600), shift=6)
    c['three lists of 3,300'] = dict(N=3, E=10000, pos=NONE)
    c['300 lists of 100'] = dict(N=300, E=30000, pos=np.random.default_rng(5).integers(0, 300, size=(2, 400)).astype(np.int64))
    c['two lists above a trip'] = dict(N=2, E=40000, pos=NONE)
    c['last block of one node'] = dict(N=2 * L + 1, E=3 * (2 * L + 1), pos=_edge_graph(2 * L + 1, L, 21))
    c['whole blocks'] = dict(N=2 * L, E=6 * L, pos=_edge_graph(2 * L, L, 22))
    c['one node short of a block'] = dict(N=L - 1, E=3 * (L - 1), pos=_edge_graph(L - 1, L, 23))
    c['many blocks and chunks'] = dict(N=big['N'], E=big['E'], pos=big['pos'])
    return c


SMALL = [n for n in _cases() if n != 'many blocks and chunks']


@functools.lru_cache(maxsize=None)
def _ref(name, seed):
    """(draw, buckets) of a case from the restatement, computed once per seed and left unchanged."""
    c = _cases()[name]
    d = R.case_draw('three passes', seed) [1] if name == 'many blocks and chunks' else R.draw(c['N'], c['E'], seed, c['pos'])
    b = R.buckets(d[0], d[1], c['N'])
    for a in b:
        a.setflags(write=False)
    return d, b


def _run_abi(dev, N, E, seed, pos, shift, ws_fill=SENT):
    """mgv_neg_partition into sentinel-filled outputs with guard entries and a sentinel-filled workspace.
    -> (the five arrays, status[4]); the guards and the entries behind the workspace are checked here."""
    from deepgate import _hip
    from deepgate._hip import ptr
    plan = _plan_from(dev, N, pos)
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', N, E)
    assert n_ws > 4 * E
    ws = torch.full((n_ws + PAD,), ws_fill, dtype=torch.int32, device=dev)
    ei = torch.full((2 * E + PAD,), SENT, dtype=torch.int64, device=dev)
    out_ptr, in_ptr = (torch.full((N + 1 + PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(2))
    out_dst, in_src = (torch.full((E + PAD,), SENT, dtype=torch.int32, device=dev) for _ in range(2))
    _hip.call('mgv_neg_partition', N, E, seed, shift, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(ei), ptr(out_ptr), ptr(out_dst), ptr(in_ptr),
              ptr(in_src), ptr(ws), n_ws)
    torch.cuda.synchronize()
    for t, n, what in ((ei, 2 * E, 'edge_index'), (out_ptr, N + 1, 'out_ptr'), (in_ptr, N + 1, 'in_ptr'), (out_dst, E, 'out_dst'),
                       (in_src, E, 'in_src')):
        assert bool((t[n:] == SENT).all()), 'the guard behind %s was written' % what
    assert bool((ws[n_ws:] == ws_fill).all()), 'entries behind the workspace were written'
    got = (ei[:2 * E].view(2, E).cpu().numpy(), out_ptr[:N + 1].cpu().numpy(), out_dst[:E].cpu().numpy(), in_ptr[:N + 1].cpu().numpy(),
           in_src[:E].cpu().numpy())
    return got, ws[:4].cpu().numpy()


def _trips(ptr, N, shift):
    """(finishing trips, lists finished in their output rows) of one side, from the restatement's pointer row: a block's nodes are
    taken in order, as many per trip as hold at most CAP pairs; a list above CAP is a trip of its own."""
    ptr = np.asarray(ptr, dtype=np.int64)
    trips = wide = 0
    for node0 in range(0, N, 1 << shift):
        lo, end = node0, min(node0 + (1 << shift), N)
        while lo < end:
            if ptr[lo + 1] - ptr[lo] > CAP:
                hi, wide = lo + 1, wide + 1
            else:
                hi = lo + int(np.searchsorted(ptr[lo + 1:end + 1], ptr[lo] + CAP, side='right'))
            lo, trips = hi, trips + 1
    return trips, wide


def _shift_of(c):
    from deepgate import sampling
    return c.get('shift', sampling.partition_shift(c['N'], c['E']))


def _surface(dev, monkeypatch, N, pos, num, base, partition=True, call=0, plan=None):
    from deepgate import sampling
    plan = plan or _plan_from(dev, N, pos)
    monkeypatch.setattr(sampling, 'PARTITION', partition)
    monkeypatch.setattr(sampling, '_CALLS', itertools.count(call))
    torch.manual_seed(base)
    neg = sampling.negative_sampling_device(plan, num_neg_samples=num)
    torch.cuda.synchronize()
    return neg


def _arrays(neg):
    return [neg.edge_index.cpu().numpy()] + [t.cpu().numpy() for t in neg.csr]


# ---- the host's choice: no GPU ----

def test_the_hosts_choice_is_a_pure_function_of_the_sizes_and_stays_inside_the_caps():
    from deepgate import sampling
    assert (sampling.PART_MAX_SHIFT, sampling.PART_MAX_BLOCKS) == (MAX_SHIFT, MAX_BLOCKS) and sampling.PART_TARGET < CAP
    bench_N, bench_E = 4194304, 6558720 + 4194304          # the benchmark's config 2
    sizes_N = [2, 3, 5, 64, 300, 4095, 4096, 4097, 8191, 8192, 8193, 1 << 20, bench_N, MAX_BLOCKS << MAX_SHIFT, (MAX_BLOCKS << MAX_SHIFT) + 1,
               1 << 24, (1 << 31) - 1]
    sizes_E = [1, 255, 257, 1000, 10000, 1000000, 3 * (1 << 20) + 5, bench_E, (1 << 28) - 1]
    for N in sizes_N:
        for E in sizes_E:
            s = sampling.partition_shift(N, E)
            assert s == sampling.partition_shift(N, E) == sampling.partition_shift(np.int64(N), np.int64(E))
            if N > MAX_BLOCKS << MAX_SHIFT:
                assert s is None, (N, E)                   # more blocks than the partition pass ranks in LDS: the two-entry route
                continue
            assert s is not None and 0 <= s <= MAX_SHIFT and -(-N // (1 << s)) <= MAX_BLOCKS, (N, E, s)
            # raised only while the expected pairs per block stay inside the target; below it only where the block cap forces it
            if s > 0 and -(-N // (1 << (s - 1))) <= MAX_BLOCKS:
                assert E * (1 << s) <= sampling.PART_TARGET * N, (N, E, s)
            if s < MAX_SHIFT:
                assert E * (1 << (s + 1)) > sampling.PART_TARGET * N, (N, E, s)
    assert sampling.partition_shift(bench_N, bench_E) == 12
    for N, E in ((1, 5), (2, 0), (2, -1), (2, 1 << 28), (1 << 31, 5)):
        assert sampling.partition_shift(N, E) is None


# ---- the entry against the restatement ----

@pytest.mark.gpu
@pytest.mark.parametrize('k', (0, 1))
@pytest.mark.parametrize('name', SMALL)
def test_the_entry_equals_the_restatement(name, k):
    dev = _dev()
    c, seed = _cases()[name], R.seed_of(BASES[k], 0)
    d, want = _ref(name, seed)
    shift = _shift_of(c)
    got, status = _run_abi(dev, c['N'], c['E'], seed, c['pos'], shift)
    R.assert_same_buckets(got, want)
    nb = -(-c['N'] // (1 << shift))
    largest = max(int(np.bincount(idx >> shift, minlength=nb).max()) for idx in (d[0], d[1]))
    assert int(status[0]) == nb and int(status[1]) == largest
    print('%s: shift %d, %d blocks, largest %d pairs, %d trips, %d lists finished in their rows' % (name, shift, nb, status[1], status[2], status[3]))
    trips, wide = (sum(x) for x in zip(_trips(want[1], c['N'], shift), _trips(want[3], c['N'], shift)))
    assert (int(status[2]), int(status[3])) == (trips, wide)
    if name == 'one block of a million pairs':
        assert nb == 1 and largest == 1000000 and trips >= 2 * (1000000 // CAP)          # the overflow path: trips over node sub-ranges
    elif name == 'two lists above a trip':
        assert int(np.diff(want[1]).min()) > CAP and wide == 4
    elif name.startswith(('last block', 'whole blocks', 'one node short')):
        L = 1 << MAX_SHIFT
        assert shift == MAX_SHIFT and nb == -(-c['N'] // L) and trips == 2 * nb
        pos_len = np.bincount(c['pos'][0], minlength=c['N'])
        for e in range(L, c['N'], L):                    # positive and negative lists on both sides of every block edge
            assert pos_len[e - 1] >= 150 and pos_len[e] >= 150
            assert np.diff(want[1])[e - 2:e + 2].sum() > 0 and np.diff(want[3])[e - 2:e + 2].sum() > 0
        assert pos_len[c['N'] - 1] >= 150
    else:
        assert trips == 2 * nb and wide == 0


@pytest.mark.gpu
def test_every_block_size_gives_the_same_arrays():
    dev = _dev()
    name, seed = '300 lists of 100', R.seed_of(1234, 0)
    c, (d, want) = _cases()[name], _ref(name, seed)
    for shift in (0, 3, 8, 12):
        got, status = _run_abi(dev, c['N'], c['E'], seed, c['pos'], shift)
        R.assert_same_buckets(got, want)
        assert int(status[0]) == -(-300 // (1 << shift))
    assert int(status[1]) == 30000 and int(status[2]) >= 4          # shift 12: one block, two trips a side at the least


@pytest.mark.gpu
def test_many_blocks_and_chunks_with_a_ragged_last_chunk():
    dev = _dev()
    name, seed = 'many blocks and chunks', R.SEEDS[0]
    c, (d, want) = _cases()[name], _ref(name, seed)
    assert R.SEEDS[0] == R.seed_of(0, 0) and c['E'] % CHUNK == 5 and c['E'] // CHUNK == 192
    shift = _shift_of(c)
    got, status = _run_abi(dev, c['N'], c['E'], seed, c['pos'], shift)
    R.assert_same_buckets(got, want)
    assert shift == 11 and int(status[0]) == 512 and int(status[2]) == 1024 and int(status[1]) < CAP


# ---- through sampling.negative_sampling_device ----

@pytest.mark.gpu
@pytest.mark.parametrize('base', BASES)
@pytest.mark.parametrize('name', SMALL + ['many blocks and chunks'])
def test_the_python_surface_equals_the_restatement_and_itself(name, base, monkeypatch):
    dev = _dev()
    if name == 'many blocks and chunks' and base != 0:
        name = 'last block of one node'                      # the large shape has one reference draw, at seed_of(0, 0); call 7 instead
        call = 7
    else:
        call = 0
    c = _cases()[name]
    seed = R.seed_of(base, call)
    want = _ref(name, seed)[1] if call == 0 else R.buckets(*R.draw(c['N'], c['E'], seed, c['pos'])[:2], c['N'])
    plan = _plan_from(dev, c['N'], c['pos'])
    first = _surface(dev, monkeypatch, c['N'], c['pos'], c['E'], base, call=call, plan=plan)
    assert first.edge_index.dtype == torch.int64 and all(t.dtype == torch.int32 for t in first.csr)
    R.assert_same_buckets(_arrays(first), want)
    second = _surface(dev, monkeypatch, c['N'], c['pos'], c['E'], base, call=call, plan=plan)      # twice in a row: nothing depends on arrival order
    assert torch.equal(first.edge_index, second.edge_index) and all(torch.equal(a, b) for a, b in zip(first.csr, second.csr))


@pytest.mark.gpu
@pytest.mark.parametrize('base', BASES)
def test_the_count_rule_and_a_given_count(base, monkeypatch):
    dev = _dev()
    N, pos = 64, R.tiny_graph(64, 600)
    loops = int((pos[0] == pos[1]).sum())
    assert loops > 0 and np.unique(pos[0] * N + pos[1]).size < 600           # self loops and duplicate edges
    plan = _plan_from(dev, N, pos)
    seed = R.seed_of(base, 0)
    for num, E in ((None, 600 - loops + N), (1000, 1000)):
        neg = _surface(dev, monkeypatch, N, pos, num, base, plan=plan)
        assert neg.edge_index.shape == (2, E)
        d = R.draw(N, E, seed, pos)
        R.assert_same_buckets(_arrays(neg), R.buckets(d[0], d[1], N))
    neg = _surface(dev, monkeypatch, N, pos, 0, base, plan=plan)
    assert neg.edge_index.shape == (2, 0) and neg.edge_index.dtype == torch.int64
    assert not bool(neg.out_ptr.any()) and not bool(neg.in_ptr.any()) and neg.out_ptr.shape == (N + 1,)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ('3 nodes, one free pair', '300 lists of 100', 'last block of one node'))
def test_both_routes_give_the_same_arrays_in_one_process(name, monkeypatch):
    dev = _dev()
    c = _cases()[name]
    plan = _plan_from(dev, c['N'], c['pos'])
    new = _surface(dev, monkeypatch, c['N'], c['pos'], c['E'], 1234, partition=True, plan=plan)
    old = _surface(dev, monkeypatch, c['N'], c['pos'], c['E'], 1234, partition=False, plan=plan)
    assert torch.equal(new.edge_index, old.edge_index)
    for a, b in zip(new.csr, old.csr):
        assert a.dtype == b.dtype and torch.equal(a, b)
    R.assert_same_buckets(_arrays(old), _ref(name, R.seed_of(1234, 0))[1])


@pytest.mark.gpu
def test_more_blocks_than_the_cap_takes_the_two_entry_route(monkeypatch):
    dev = _dev()
    from deepgate import _hip, sampling
    N, E = (MAX_BLOCKS << MAX_SHIFT) + 1, 1000
    pos = np.random.default_rng(2).integers(0, N, size=(2, 500)).astype(np.int64)
    assert sampling.partition_shift(N, E) is None and sampling.partition_shift(N - 1, E) == MAX_SHIFT
    called = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a: (called.append(name), real(name, *a))[1])
    neg = _surface(dev, monkeypatch, N, pos, E, 1234)
    assert 'mgv_neg_sample' in called and 'mgv_neg_partition' not in called
    d = R.draw(N, E, R.seed_of(1234, 0), pos)
    R.assert_same_buckets(_arrays(neg), R.buckets(d[0], d[1], N))
    # the entry itself refuses the shape as unsupported, whatever block size it is asked for
    i32 = dict(dtype=torch.int32, device=dev)
    ws = torch.zeros(_hip.call_value('mgv_neg_partition_ws_ints', N, E), **i32)
    ptrs, lists, ei = torch.zeros(2, N + 1, **i32), torch.zeros(2, E, **i32), torch.zeros(2, E, dtype=torch.int64, device=dev)
    for shift in (MAX_SHIFT, MAX_SHIFT + 1, -1):
        with pytest.raises(_hip.HipLibraryError, match='MGV_EUNSUPPORTED'):
            real('mgv_neg_partition', N, E, 1, shift, _hip.ptr(ptrs[0]), None, _hip.ptr(ei), _hip.ptr(ptrs[0]), _hip.ptr(lists[0]),
                 _hip.ptr(ptrs[1]), _hip.ptr(lists[1]), _hip.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    assert not bool(ws.any()) and not bool(lists.any())


@pytest.mark.gpu
def test_the_entry_refuses_what_the_header_says_it_refuses():
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import ptr
    N, E = 8, 100
    plan = _plan_from(dev, N, R.tiny_graph(8, 20))
    i32 = dict(dtype=torch.int32, device=dev)
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', N, E)
    ws = torch.full((n_ws,), SENT, **i32)
    ei = torch.full((2, E), SENT, dtype=torch.int64, device=dev)
    out_ptr, in_ptr, out_dst, in_src = (torch.full((n,), SENT, **i32) for n in (N + 1, N + 1, E, E))
    good = dict(N=N, E=E, seed=R.SEEDS[0], shift=0, pos_ptr=ptr(plan.out_ptr), pos_dst=ptr(plan.out_dst), ei=ptr(ei), out_ptr=ptr(out_ptr),
                out_dst=ptr(out_dst), in_ptr=ptr(in_ptr), in_src=ptr(in_src), ws=ptr(ws), ws_ints=n_ws)
    bad = [dict(N=1), dict(N=0), dict(N=1 << 31), dict(E=-1), dict(E=1 << 28), dict(ws_ints=n_ws - 1), dict(ws_ints=0)]
    bad += [{k: None} for k in ('pos_ptr', 'ei', 'out_ptr', 'out_dst', 'in_ptr', 'in_src', 'ws')]
    for change in bad:
        with pytest.raises(_hip.HipLibraryError, match='MGV_EINVAL'):
            _hip.call('mgv_neg_partition', *dict(good, **change).values())
    for N_, E_ in ((1, 5), (1 << 31, 5), (8, -1), (8, 1 << 28)):
        assert _hip.call_value('mgv_neg_partition_ws_ints', N_, E_) == -1
    torch.cuda.synchronize()
    for t in (ws, ei, out_ptr, in_ptr, out_dst, in_src):
        assert bool((t == SENT).all())                       # a refused call writes nothing
    # E = 0: empty buckets, no payload needed
    _hip.call('mgv_neg_partition', *dict(good, E=0, ei=None, out_dst=None, in_src=None).values())
    torch.cuda.synchronize()
    assert not bool(out_ptr.any()) and not bool(in_ptr.any()) and bool((out_dst == SENT).all())
    # and the good call is good
    _hip.call('mgv_neg_partition', *good.values())
    torch.cuda.synchronize()
    d = R.draw(N, E, R.SEEDS[0], R.tiny_graph(8, 20))
    R.assert_same_buckets((ei.cpu().numpy(), out_ptr.cpu().numpy(), out_dst.cpu().numpy(), in_ptr.cpu().numpy(), in_src.cpu().numpy()),
                          R.buckets(d[0], d[1], N))
