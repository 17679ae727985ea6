"""mgv_seg_sum_entries (per-colour row sums over a flat entry list) against mgv_seg_sum on the same tables, BIT FOR BIT, the entry-list
builder (mgv_seg_entries, GraphPlan.seg_entries) against a numpy restatement of the encoding, and both through the product
(StructEncoderFn with ops.SEG_LISTS on and off: every parameter gradient bit-identical).

The encoding (include/mgvae_hip.h): in member order, per member position m of `items`, the entry items[m] (>= 0: that row of `direct`,
starts a new member), then ~nbr_idx[e] over items[m]'s list (< 0: that row of `agg`, continues the member); segment pointers count
entries.  The additions are mgv_seg_sum's in its order, so the two kernels must agree in every bit; rows of mixed magnitudes
(1e-3 .. 1e3) make any other association show.

Shapes are the smallest at which the kernel can go wrong: a lane group takes 8 entries per batch (4 at H = 16), so the designed
lists cross one and two batch boundaries, a member's entries straddle one, colours of 64 and 65 members bring a partial row and a
second level, and the grid has more than one workgroup (H = 128: 8 segments per workgroup).  One size has to be large: a lane group
walks more than one segment only above the launch's grid cap, 4096 * 1024 / H segments (test_many_segments_per_lane_group)."""
import numpy as np
import pytest
import torch

import test_half_round_schedule as HRS

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128)
BATCH = 8               # entries per lane group and batch (min(H / 4, 8)): every designed length below crosses both 4 and 8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def entries_ref(order, ptr, idx, seg_ptr):
    """The encoding, restated: (entries, segment pointers in entry positions)."""
    ent, off = [], [0]
    for m in order:
        ent.append(int(m))
        ent += [~int(j) for j in idx[ptr[m]:ptr[m + 1]]]
        off.append(len(ent))
    return np.array(ent, dtype=np.int32), np.array([off[s] for s in seg_ptr], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ designed tables
# node -> in-list length.  Node 0: an empty list (and a colour of its own); 1..4: lists of 2 in one colour (entries 3 + 3 + 3 + 3: the
# second member straddles position 4, the third position 8); 5: 9 entries (more than one batch); 6: 20 (more than two); 7: 40.
DESIGNED_DEG = {0: 0, 1: 2, 2: 2, 3: 2, 4: 2, 5: 9, 6: 20, 7: 40}
N_NODES = 330


def _designed(dev, big):
    """(plan, cid, C): colour 0 nobody carries, 1 = {node 0}, 2 = {1, 2, 3, 4}, 3 = {5, 6}, 4 = {7}, 5 = 64 members, 6 = 65 members
    (`big`; else 64 again: then every colour is one segment and level 1 writes row s without an out_row table), the rest random
    colours of a few members."""
    from deepgate.graph_plan import GraphPlan
    rng = np.random.Generator(np.random.PCG64(17))
    deg = rng.integers(0, 4, N_NODES)
    for v, d in DESIGNED_DEG.items():
        deg[v] = d
    src = np.concatenate([rng.choice(N_NODES, size=d, replace=False) for d in deg]).astype(np.int64)
    dst = np.repeat(np.arange(N_NODES), deg).astype(np.int64)
    cid = np.zeros(N_NODES, dtype=np.int64)
    cid[0], cid[1:5], cid[5:7], cid[7] = 1, 2, 3, 4
    cid[8:72] = 5
    n6 = 65 if big else 64
    cid[72:72 + n6] = 6
    rest = np.arange(72 + n6, N_NODES)
    cid[rest] = 7 + rng.integers(0, 40, rest.size)
    C = 47
    plan = GraphPlan(torch.from_numpy(np.stack([src, dst])).to(dev), N_NODES)
    assert plan.hip
    return plan, torch.from_numpy(cid).to(dev), C


def _rows(n, H, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, H, generator=g) * torch.pow(10.0, torch.rand(n, H, generator=g) * 6 - 3)).to(dev)


def _levels_old(H, tables, items, direct, agg, p, i, buf):
    from deepgate import _hip
    from deepgate._hip import ptr
    for li, (n_seg, seg_ptr, out_row, src_row) in enumerate(tables['levels']):
        if li == 0:
            _hip.call('mgv_seg_sum', H, n_seg, ptr(seg_ptr), ptr(items), ptr(direct), ptr(agg), ptr(p if agg is not None else None),
                      ptr(i if agg is not None else None), ptr(out_row), ptr(buf))
        else:
            _hip.call('mgv_seg_sum', H, n_seg, ptr(seg_ptr), None, ptr(buf[src_row:]), None, None, None, ptr(out_row), ptr(buf))


def _levels_new(H, tables, entries, seg_ptr0, direct, agg, buf):
    from deepgate import _hip
    from deepgate._hip import ptr
    for li, (n_seg, seg_ptr, out_row, src_row) in enumerate(tables['levels']):
        if li == 0:
            _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(seg_ptr0), ptr(entries), ptr(direct), ptr(agg), ptr(out_row), ptr(buf))
        else:       # the identity list
            _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(seg_ptr), None, ptr(buf[src_row:]), None, ptr(out_row), ptr(buf))


_TABLES = {}


def _case(dev, big):
    """Tables, the flat list and its restatement, built once per colouring and shared."""
    if big not in _TABLES:
        plan, cid, C = _designed(dev, big)
        order, tables = plan.class_sum_levels(cid, C)
        p, i = plan.csr(False)
        entries, esp = plan.seg_entries(False, order, tables)
        want = entries_ref(order.cpu().numpy(), p.cpu().numpy(), i.cpu().numpy(), tables['levels'][0][1].cpu().numpy())
        _TABLES[big] = (plan, order, tables, p, i, entries, esp, want)
    return _TABLES[big]


@pytest.mark.parametrize('big', [True, False], ids=['second-level', 'one-level'])
def test_the_designed_tables_are_the_ones_described(big):
    dev = _dev()
    plan, order, tables, p, i, entries, esp, want = _case(dev, big)
    levels = tables['levels']
    counts = tables['counts'].cpu().numpy()
    assert counts[0] == 0 and counts[1] == 1 and counts[5] == 64 and counts[6] == (65 if big else 64)
    if big:
        assert len(levels) == 2 and levels[0][2] is not None and tables['rows'] == tables['C'] + 2      # two partial rows, summed by level 2
    else:
        assert len(levels) == 1 and levels[0][2] is None                                                 # segment s writes row s
    # the builder: exactly the encoding, and every node once + every list once
    assert entries.dtype == torch.int32 and esp.dtype == torch.int32
    assert np.array_equal(entries.cpu().numpy(), want[0]) and np.array_equal(esp.cpu().numpy(), want[1])
    assert entries.numel() == plan.N + plan.E and int(esp[-1]) == plan.N + plan.E
    assert plan.seg_entries(False, order, tables)[0] is entries                                          # cached on the plan
    # the lengths the kernel's batches are tested by: members of 10, 21 and 41 entries, an empty list, a straddling member
    e = want[0]
    runs = np.diff(np.concatenate([np.nonzero(e >= 0)[0], [e.size]]))
    assert {1, 3, 10, 21, 41} <= set(runs.tolist()) and 2 * BATCH < 21 and BATCH < 10
    # colours 0..4 are one segment each, so colour 2 is segment 2: its members start at entry offsets 0, 3, 6, 9 — the second one's
    # entries lie across offset 4, the third one's across offset 8
    assert np.array_equal(np.nonzero(e[want[1][2]:want[1][3]] >= 0)[0], [0, 3, 6, 9])
    assert want[1][1] == want[1][0] and want[1][2] - want[1][1] == 1       # the empty segment; the member with an empty list


@pytest.mark.parametrize('H', WIDTHS)
@pytest.mark.parametrize('big', [True, False], ids=['second-level', 'one-level'])
def test_entry_sums_equal_seg_sum_bit_for_bit(big, H):
    """Every level of the designed tables through both kernels into buffers with the same fill: the raw buffers (final rows, partial
    rows, and guard rows behind them) must hold the same bits.  Covers: the empty segment (a zero row), the member with an empty
    list, lists longer than one and two batches, the straddling member, 64 and 65 members (partial rows + an identity upper level),
    out_row NULL (one-level) and non-NULL (second-level)."""
    dev = _dev()
    plan, order, tables, p, i, entries, esp, _ = _case(dev, big)
    direct, agg = _rows(plan.N, H, 100 + H, dev), _rows(plan.N, H, 200 + H, dev)
    rows, guard = tables['rows'], 4
    old = torch.full((rows + guard, H), 7.5, device=dev)
    new = torch.full((rows + guard, H), 7.5, device=dev)
    _levels_old(H, tables, order, direct, agg, p, i, old)
    _levels_new(H, tables, entries, esp, direct, agg, new)
    torch.cuda.synchronize()
    assert torch.equal(_bits(old), _bits(new))
    assert bool((new[rows:] == 7.5).all()), 'wrote behind its output'
    assert float(new[0].abs().max()) == 0.0                              # the colour nobody carries
    # against float64, so that "equal" is not "equally wrong": a sum of n terms added one by one in fp32 is within
    # (n - 1) * 2^-24 * sum |term| of the exact one (first order; 1 % on top covers the rest), n = the colour's entries
    dy = direct.double().clone()
    dy.index_add_(0, plan.in_dst.long(), agg.double()[plan.in_src.long()])
    cid = torch.empty(plan.N, dtype=torch.int64, device=dev)
    cid[order.long()] = torch.repeat_interleave(torch.arange(tables['C'], device=dev), tables['counts'].long())
    ref = torch.zeros(tables['C'], H, dtype=torch.float64, device=dev).index_add_(0, cid, dy)
    mag = torch.zeros(tables['C'], H, dtype=torch.float64, device=dev).index_add_(
        0, cid, direct.double().abs() + torch.zeros_like(dy).index_add_(0, plan.in_dst.long(), agg.double().abs()[plan.in_src.long()]))
    terms = torch.zeros(tables['C'], dtype=torch.float64, device=dev).index_add_(0, cid, 1.0 + (p[1:] - p[:-1]).double())
    assert bool(((new[:tables['C']].double() - ref).abs() <= 1.01 * 2.0 ** -24 * terms[:, None] * mag).all())


@pytest.mark.parametrize('H', WIDTHS)
def test_items_only_table_and_no_segments(H):
    """An items-only table is an entry list as it stands (every entry its own member, agg NULL); n_seg = 0 launches nothing."""
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import ptr
    plan, order, tables, p, i, entries, esp, _ = _case(dev, True)
    direct = _rows(plan.N, H, 300 + H, dev)
    rows = tables['rows']
    old, new = torch.full((rows, H), -3.25, device=dev), torch.full((rows, H), -3.25, device=dev)
    _levels_old(H, tables, order, direct, None, None, None, old)
    _levels_new(H, tables, order, tables['levels'][0][1], direct, None, new)
    torch.cuda.synchronize()
    assert torch.equal(_bits(old), _bits(new))
    untouched = new.clone()
    _hip.call('mgv_seg_sum_entries', H, 0, ptr(esp), ptr(entries), ptr(direct), None, None, ptr(new))
    torch.cuda.synchronize()
    assert torch.equal(_bits(untouched), _bits(new))


@pytest.mark.parametrize('H', WIDTHS)
def test_seg_sums_route_switch(H):
    """ops._seg_sums with the flat list, without one, and with ops.SEG_LISTS off: the same bits (what StructEncoderFn.backward calls)."""
    dev = _dev()
    from deepgate import ops
    plan, order, tables, p, i, entries, esp, _ = _case(dev, True)
    direct, agg = _rows(plan.N, H, 400 + H, dev), _rows(plan.N, H, 500 + H, dev)
    old = ops.SEG_LISTS
    try:
        ops.SEG_LISTS = True
        a = ops._seg_sums(H, tables, order, direct, agg, p, i, entries=(entries, esp))
        b = ops._seg_sums(H, tables, order, direct, agg, p, i)
        c = ops._seg_sums(H, tables, order, direct)
        ops.SEG_LISTS = False
        a0 = ops._seg_sums(H, tables, order, direct, agg, p, i, entries=(entries, esp))
        c0 = ops._seg_sums(H, tables, order, direct)
    finally:
        ops.SEG_LISTS = old
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(a0)) and torch.equal(_bits(c), _bits(c0))


# ------------------------------------------------------------------------------------------------ the plans of the schedule tests
_PLANS = {}


def _plan(dev, name):
    from deepgate.graph_plan import GraphPlan
    if name not in _PLANS:
        ei, n, xc = {'aig': lambda: HRS._netlist(False), 'hub': lambda: HRS._netlist(True), 'trees': HRS._trees}[name]()
        plan, xcls = GraphPlan(torch.from_numpy(ei).to(dev), n), torch.from_numpy(xc).to(dev)
        assert plan.hip
        _PLANS[name] = (plan, xcls, {k: plan.quotient(xcls, k, force=True) for k in (2, 3, 4)})
    return _PLANS[name]


@pytest.mark.parametrize('stages', [2, 3, 4])
@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_builder_on_the_schedule_plans(name, stages):
    """GraphPlan.seg_entries for the last colour stage's sum_levels (over the CSR that stage gathers) on the aig / hub / trees plans:
    entries and entry-segment pointers exactly the restated encoding; the hub's list of 80 is one run of negative entries."""
    dev = _dev()
    plan, xcls, quot = _plan(dev, name)
    st = quot[stages][-1]
    assert len(quot[stages]) == stages and 'sum_levels' in st and st['rev'] == (stages % 2 == 0)
    order, tables = st['sum_levels']
    p, i = plan.csr(st['rev'])
    entries, esp = plan.seg_entries(st['rev'], order, tables)
    want = entries_ref(order.cpu().numpy(), p.cpu().numpy(), i.cpu().numpy(), tables['levels'][0][1].cpu().numpy())
    assert np.array_equal(entries.cpu().numpy(), want[0]) and np.array_equal(esp.cpu().numpy(), want[1])
    assert entries.numel() == plan.N + plan.E
    e = want[0]
    longest = int(np.diff(np.concatenate([np.nonzero(e >= 0)[0], [e.size]])).max()) - 1
    pn = p.cpu().numpy()
    assert longest == int((pn[1:] - pn[:-1]).max())
    if name == 'hub' and st['rev']:
        assert longest >= 80


@pytest.mark.parametrize('stages', [2, 3])
@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_parameter_gradients_do_not_depend_on_the_route(name, stages):
    """One MultiGCNEncoder (H = 64: every parameter gradient of its backward is summed in a fixed order), two rounds, the first
    `stages` half rounds on colours and the rest per node, so the boundary's per-colour sums pull the per-node gradient over the
    flat list: forward and backward with ops.SEG_LISTS on and off — the output and every parameter gradient bit-identical."""
    dev = _dev()
    import deepgate
    from deepgate import ops
    plan, xcls, quot = _plan(dev, name)
    plan.cache.put('quotient', 4, quot[stages], held=(xcls,))       # what the encoder's request for 2R = 4 stages finds
    H = 64
    torch.manual_seed(23)
    enc = deepgate.digae_layer.MultiGCNEncoder(2, H, 6, True, True).to(dev)
    rows = torch.eye(6, device=dev)
    gy = _rows(plan.N, H, 77, dev)
    res, old = {}, ops.SEG_LISTS
    try:
        for flag in (True, False):
            ops.SEG_LISTS = flag
            plan.cache.drop('seg_entries')
            enc.zero_grad(set_to_none=True)
            out = enc(None, None, plan=plan, classes=(rows, xcls))
            (out * gy).sum().backward()
            res[flag] = [out.detach()] + [q.grad.detach().clone() for q in enc.parameters()]
            assert ('seg_entries' in plan.cache) == flag     # the list is built when, and only when, the route reads it
    finally:
        ops.SEG_LISTS = old
        plan.cache.put('quotient', 4, quot[4], held=(xcls,))
    names = ['out'] + [k for k, _ in enc.named_parameters()]
    assert all(float(g.abs().max()) > 0 for g in res[True][1:])
    for nm, a, b in zip(names, res[True], res[False]):
        assert torch.equal(_bits(a), _bits(b)), nm


# ------------------------------------------------------------------------------------------------ more segments than lane groups
# The launch caps its grid at 4,096 workgroups (csrc/mgv_common.h grid_for(tiles, 16)) of 256 / (H / 4) lane groups: above
# STRIDE(H) = 4096 * 1024 / H segments a lane group walks several, s, s + STRIDE, s + 2 STRIDE, ..., and hands over between them — the
# next segment's first batch fetched beside the last rows of this one, pointers and output row of the segment after the next fetched
# two ahead, empty ranges behind the last.  None of the tables above reaches that.
def _stride(H):
    return 4096 * (256 // (H // 4))


_MANY = {}


def _many(dev, H):
    """2.5 STRIDE + 77 segments (every lane group walks two, half of them and a few more a third) of 0 .. 2 members with lists of
    0 .. 2 entries, so most segments are 0 .. 4 entries; every 997th row carries a list of 19 (a segment of three batches in between the
    tiny ones).  Members name any of R rows, rows repeat; ~22 % of the segments are empty.  CSR form for mgv_seg_sum, the flat list
    restated in numpy for mgv_seg_sum_entries."""
    if H not in _MANY:
        n_seg = 2 * _stride(H) + _stride(H) // 2 + 77
        rng = np.random.Generator(np.random.PCG64(1000 + H))
        R = 5000
        rdeg = rng.integers(0, 3, R)
        rdeg[::997] = 19
        rptr = np.concatenate([[0], np.cumsum(rdeg)]).astype(np.int64)
        ridx = rng.integers(0, R, rptr[-1])
        nmem = rng.choice(3, size=n_seg, p=[0.22, 0.48, 0.30])
        nmem[-1] = 0 if H in (16, 64) else 2                 # the very last segment empty / not
        seg_ptr = np.concatenate([[0], np.cumsum(nmem)]).astype(np.int64)
        M = int(seg_ptr[-1])
        items = rng.integers(0, R, M)
        d = rdeg[items]
        off = np.concatenate([[0], np.cumsum(1 + d)]).astype(np.int64)
        ent = np.empty(off[-1], dtype=np.int64)
        ent[off[:-1]] = items
        member = np.repeat(np.arange(M), d)
        k = np.arange(member.size) - np.repeat(off[:-1] - np.arange(M), d)
        ent[off[member] + 1 + k] = ~ridx[rptr[items[member]] + k]
        esp = off[seg_ptr]
        assert int((esp[1:] == esp[:-1]).sum()) > n_seg // 6 and int((esp[1:] - esp[:-1]).max()) >= 20
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        _MANY[H] = dict(n_seg=n_seg, R=R, M=M, seg_ptr=i32(seg_ptr), items=i32(items), rptr=i32(rptr), ridx=i32(ridx), ent=i32(ent), esp=i32(esp),
                        out_row=i32(rng.permutation(n_seg)))
    return _MANY[H]


@pytest.mark.parametrize('with_out_row', [True, False], ids=['out_row', 'row-s'])
@pytest.mark.parametrize('H', WIDTHS)
def test_many_segments_per_lane_group(H, with_out_row):
    """More than twice the grid stride of tiny segments: the flat list (negative entries) and the identity list against mgv_seg_sum,
    bit for bit, with and without an out_row table; and the list builder on the same tables (its three-launch scan, members that
    repeat rows) against the numpy restatement."""
    dev = _dev()
    from deepgate import _hip
    from deepgate._hip import ptr
    c = _many(dev, H)
    n_seg = c['n_seg']
    assert n_seg > 2 * _stride(H)
    direct, agg = _rows(c['R'], H, 600 + H, dev), _rows(c['R'], H, 700 + H, dev)
    out_row = c['out_row'] if with_out_row else None
    old, new = torch.full((n_seg + 2, H), 7.5, device=dev), torch.full((n_seg + 2, H), 7.5, device=dev)
    _hip.call('mgv_seg_sum', H, n_seg, ptr(c['seg_ptr']), ptr(c['items']), ptr(direct), ptr(agg), ptr(c['rptr']), ptr(c['ridx']), ptr(out_row), ptr(old))
    _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(c['esp']), ptr(c['ent']), ptr(direct), ptr(agg), ptr(out_row), ptr(new))
    torch.cuda.synchronize()
    assert torch.equal(_bits(old), _bits(new))
    assert bool((new[n_seg:] == 7.5).all()), 'wrote behind its output'
    del old, new
    # the identity list: segment s sums rows [seg_ptr[s], seg_ptr[s + 1]) of a table of M rows
    table = _rows(c['M'], H, 800 + H, dev)
    old, new = torch.full((n_seg + 2, H), -1.5, device=dev), torch.full((n_seg + 2, H), -1.5, device=dev)
    _hip.call('mgv_seg_sum', H, n_seg, ptr(c['seg_ptr']), None, ptr(table), None, None, None, ptr(out_row), ptr(old))
    _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(c['seg_ptr']), None, ptr(table), None, ptr(out_row), ptr(new))
    torch.cuda.synchronize()
    assert torch.equal(_bits(old), _bits(new))
    assert bool((new[n_seg:] == -1.5).all()), 'wrote behind its output'
    if with_out_row:
        return
    # the builder on these tables
    i32 = dict(dtype=torch.int32, device=dev)
    cap = int(c['ent'].numel())
    entries, esp = torch.full((cap + 8,), -7, **i32), torch.zeros(n_seg + 1, **i32)
    n_s = _hip.call_value('mgv_seg_entries_scratch_ints', c['M'])
    scratch = torch.empty(n_s, **i32)
    _hip.call('mgv_seg_entries', c['M'], ptr(c['items']), ptr(c['rptr']), ptr(c['ridx']), n_seg, ptr(c['seg_ptr']), cap, ptr(entries), ptr(esp),
              ptr(scratch), n_s)
    torch.cuda.synchronize()
    assert torch.equal(entries[:cap], c['ent']) and torch.equal(esp, c['esp']) and bool((entries[cap:] == -7).all())
