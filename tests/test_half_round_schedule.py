"""CPU tests of ops.half_round_schedule: the list of half-round records that StructEncoderFn walks forward and, in reverse,
backward.  Which kernel rows a half round computes, what it reads and how the gradient reaches it is data; here that data
is checked on plans small enough to read, in every regime (per node, (degree, class) table, table mode, colour quotient
cut short and through the last half round), without a launch."""
import numpy as np
import pytest
import torch

from deepgate import ops, synthetic as syn
from deepgate.graph_plan import GraphPlan

MODES = {'x3-64': (True, 64), 'x3-32': (True, 32), 'f32-64': (False, 64)}       # (the bf16x3 kernels serve H, H)


def _netlist(hub):
    """Two random AIGs (N = 608); `hub`: node 5 also feeds 80 later gates, so it is a heavy row of the out-CSR."""
    a = syn.collate([syn.make_graph('aig', 64 + 12 * 20, 12, 900 + i, n_inputs=64) for i in range(2)])
    ei = a['edge_index']
    if hub:
        later = np.nonzero(a['forward_level'] > 0)[0]
        ei = np.unique(np.concatenate([ei, np.stack([np.full(80, 5), later[:80]])], axis=1), axis=1)
    return ei, a['num_nodes'], a['x'][:, 1].astype('uint8')


def _trees(copies=6, leaves=16):
    """Balanced AND trees, an inverter behind every gate of alternate levels (as the 70-tree netlist of test_hip_struct_paths)."""
    src, dst, gate = [], [], []
    nxt = 0
    for _ in range(copies):
        ids = list(range(nxt, nxt + leaves))
        gate += [0] * leaves
        nxt += leaves
        lvl = 0
        while len(ids) > 1:
            new = []
            for a, b in zip(ids[0::2], ids[1::2]):
                src += [a, b]; dst += [nxt, nxt]; gate.append(1); v = nxt; nxt += 1
                if lvl % 2 == 1:
                    src.append(v); dst.append(nxt); gate.append(2); v = nxt; nxt += 1
                new.append(v)
            ids, lvl = new, lvl + 1
    return np.array([src, dst], dtype=np.int64), nxt, (np.array(gate) == 1).astype('uint8')


_BUILT = {}


def _plan(name):
    """(plan, xcls, first, quot): built once per graph and shared."""
    if name not in _BUILT:
        ei, n, xc = {'aig': lambda: _netlist(False), 'hub': lambda: _netlist(True), 'trees': _trees}[name]()
        plan, xcls = GraphPlan(torch.from_numpy(ei), n), torch.from_numpy(xc)
        _BUILT[name] = (plan, xcls, plan.first_stage_classes(xcls), plan.quotient(xcls, 4, force=True))
    return _BUILT[name]


def test_the_plans_are_the_ones_described():
    plan, _, first, quot = _plan('aig')
    assert plan.N == 608 and first[1] == 3 and [s['C'] for s in quot] == [3, 38, 340, 505] and 'sum_levels' in quot[-1]
    plan, _, _, quot = _plan('trees')
    assert plan.N == 216 and [s['C'] for s in quot] == [3, 5, 6, 7]
    plan, _, _, quot = _plan('hub')
    assert plan.heavy(True)[0] == 1 and plan.heavy(False)[0] == 0 and len(quot) == 4


def _check_lists(plan, sched):
    """Every record's lists fit the rows it computes, and every entry names a row its input provides."""
    N = plan.N
    avail = 1                       # rows of the previous output: the colour stages start from a one-row table
    for k, r in enumerate(sched):
        assert r.rev == (k % 2 == 1)
        assert r.ptr.numel() == r.rows + 1 and r.xcls.numel() == r.rows and r.xcls.dtype == torch.uint8
        p = r.ptr.long()
        assert int(p[0]) == 0 and bool((p[1:] >= p[:-1]).all()) and int(p[-1]) <= r.idx.numel()
        ent = r.idx[:int(p[-1])].long()
        if r.src == 'ones':
            rows_in = r.rows
        elif r.src == 'stacked':
            assert r.n_rows == r.rows and r.table_own is None and r.own.numel() == r.rows
            assert int(r.own.min()) >= 0 and int(r.own.max()) < avail
            rows_in = r.rows + avail
        else:
            assert r.src == 'prev'
            rows_in = avail
        if r.table_own is not None:
            assert r.table_own.numel() == r.rows and r.table_own.dtype == torch.int32 and r.n_rows is None
            assert int(r.table_own.min()) >= 0 and int(r.table_own.max()) < rows_in
            if r.tagged:            # entry = node | table row << 24: the node names the row whose own state it is, the tag a table row
                assert plan.tagged_fits(rows_in)
                node, row = ent & 0xFFFFFF, ent >> 24
                assert bool((node < r.rows).all()) and bool((row < rows_in).all()) and bool((ent >= 0).all())
                assert torch.equal(row, r.table_own.long()[node])
                ent = row
        elif r.src != 'stacked':
            assert rows_in == r.rows          # own rows are read in place
        if ent.numel():
            assert int(ent.min()) >= 0 and int(ent.max()) < rows_in, k
        if r.heavy is not None:
            deg = p[1:] - p[:-1]
            assert r.heavy[0] == r.heavy[1].numel() and r.heavy[1].long().tolist() == torch.nonzero(deg > GraphPlan.HEAVY_ROW).reshape(-1).tolist()
        avail = r.rows
        if r.expand is not None:
            assert r.expand.numel() == N and r.expand.dtype == torch.int32 and int(r.expand.min()) >= 0 and int(r.expand.max()) < r.rows
            avail = N
    assert not sched or avail == N


def _per_node(plan, xcls, r, k):
    p, i = plan.csr(r.rev)
    return (r.rows == plan.N and r.ptr is p and r.idx is i and r.xcls is xcls and r.heavy == plan.heavy(r.rev) and r.table_own is None
            and r.n_rows is None and r.tagged and r.src == ('ones' if k == 0 else 'prev') and r.expand is None and r.grad == 'rows')


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('rounds', [1, 2])
@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_per_node_schedule(name, rounds, mode):
    plan, xcls, _, _ = _plan(name)
    x3, H = MODES[mode]
    for first, quot in ((None, None), (None, [])):
        sched = ops.half_round_schedule(plan, xcls, rounds, H, x3, first, quot)
        assert len(sched) == 2 * rounds and all(_per_node(plan, xcls, r, k) for k, r in enumerate(sched))
        _check_lists(plan, sched)
    if name == 'hub':
        assert sched[1].heavy[0] == 1 and sched[0].heavy[0] == 0


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('rounds', [1, 2])
@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_table_schedule(name, rounds, mode):
    """Stage 0 on the pair rows; bf16x3 at H = 64 reads the table in place through tagged entries (no expansion), every other
    mode expands it behind stage 0."""
    plan, xcls, first, _ = _plan(name)
    x3, H = MODES[mode]
    cid, C = first[0], first[1]
    sched = ops.half_round_schedule(plan, xcls, rounds, H, x3, first, None)
    assert len(sched) == 2 * rounds
    _check_lists(plan, sched)
    r0, r1 = sched[0], sched[1]
    assert r0.rows == C and (r0.ptr, r0.idx, r0.xcls) == tuple(first[2:]) and r0.src == 'ones' and r0.heavy is None
    assert r0.table_own is None and r0.n_rows is None and r0.tagged
    assert r0.grad == 'pairs' and r0.gsrc[0] is cid and (r0.gsrc[1], r0.gsrc[2]) == plan.csr(False)
    table_mode = x3 and H == 64
    if table_mode:
        assert r0.expand is None
        assert r1.rows == plan.N and r1.table_own is cid and r1.tagged and r1.idx is plan.tagged_idx(True, cid) and r1.ptr is plan.csr(True)[0]
        assert r1.src == 'prev' and r1.grad == 'rows' and r1.heavy == plan.heavy(True) and r1.expand is None and r1.xcls is xcls
    else:
        assert r0.expand is cid
    assert sum(r.expand is not None for r in sched) == (0 if table_mode else 1)
    assert all(_per_node(plan, xcls, r, k) for k, r in enumerate(sched) if k >= (2 if table_mode else 1))


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('rounds,stages', [(1, 2), (2, 2), (2, 4), (2, 3)])
@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_quotient_schedule(name, rounds, stages, mode):
    """Stages 0..q-1 on colours, one expansion behind stage q-1 (also when q = 2R), the rest per node; the pair table is not used."""
    plan, xcls, first, quot = _plan(name)
    x3, H = MODES[mode]
    quot = quot[:stages]
    q = len(quot)
    sched = ops.half_round_schedule(plan, xcls, rounds, H, x3, first, quot)
    assert len(sched) == 2 * rounds and q <= 2 * rounds
    _check_lists(plan, sched)
    for k, (r, st) in enumerate(zip(sched, quot)):
        assert r.rows == st['C'] and r.ptr is st['ptr'] and r.xcls is st['xcls'] and r.heavy is st['heavy']
        if x3:
            assert r.src == 'prev' and r.idx is st['ent_idx'] and r.table_own is st['own32'] and not r.tagged and r.n_rows is None
        else:
            assert r.src == 'stacked' and r.idx is st['idx'] and r.own is st['own'] and r.n_rows == st['C'] and r.table_own is None
        if k + 1 < q:
            nx = quot[k + 1]
            assert r.expand is None and r.grad == 'above'
            assert all(a is b for a, b in zip(r.gsrc, (nx['own_levels'], nx['own_rows'], nx['ent_levels'], nx['ent_rows'])))
        else:
            assert r.expand is st['cid'] and r.grad == 'sum_levels' and r.gsrc[0] is st.get('sum_levels')
            assert (r.gsrc[1], r.gsrc[2]) == plan.csr(r.rev)
    assert sum(r.expand is not None for r in sched) == 1
    assert all(_per_node(plan, xcls, r, k) for k, r in enumerate(sched) if k >= q)
    if name == 'hub':
        assert any(r.heavy is not None and r.heavy[0] >= 1 for r in sched)


def test_more_stages_than_half_rounds_are_not_scheduled():
    plan, xcls, _, quot = _plan('trees')
    sched = ops.half_round_schedule(plan, xcls, 1, 64, True, None, quot)
    assert [r.rows for r in sched] == [3, 5] and sched[1].expand is quot[1]['cid'] and sched[1].grad == 'sum_levels'
    assert ops.half_round_schedule(plan, xcls, 0, 64, True, None, quot) == []
