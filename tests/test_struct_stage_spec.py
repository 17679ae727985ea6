"""CPU checks behind tests/test_hip_struct_stage_reference.py: the float64 restatement of one struct-stage half round
(tests/struct_stage_ref.py) is pinned to the reference project's own numbers (fixture g3_ops) and to oracle/ref_cpu.py, the case
builders are shown to reach every row path, tile order and index form the device tests rely on, every defect of the kinds those
tests are there to catch is shown to be at least 10x outside their bound when planted in the restatement, and the bf16x3 emulation
is shown to emulate split precision."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import struct_stage_ref as SR  # noqa: E402
from conftest import load_golden  # noqa: E402

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
FLOOR = {'f32': 2.0 ** -23, 'x3': 2.0 ** -17}


def _compose(raw, aggr, gru, H, rows):
    """The kernels' folded parameters from the module's: Wc = W_ih[:, :H] Wm, bc = W_ih[:, :H] bm, xtab = rows W_ih[:, H:]^T + b_ih."""
    w_ih = raw[gru + '.weight_ih_l0']
    return [rows @ w_ih[:, H:].t() + raw[gru + '.bias_ih_l0'], w_ih[:, :H] @ raw[aggr + '.msg.weight'], w_ih[:, :H] @ raw[aggr + '.msg.bias'],
            raw[gru + '.weight_hh_l0'], raw[gru + '.bias_hh_l0']]


def _chain(h0, csrs, xcls, comps, lw, lb, up):
    """Half rounds k = 0.. over csrs[k % 2] with parameters comps[k % 2] in float64: every state, then the backward with the
    g_agg -> gy_agg hand-over between opposite CSRs.  Returns (states, g_direct and g_agg of stage 0, per-parity gradient sums)."""
    det = lambda ts: [None if t is None else t.detach() for t in ts]      # noqa: E731
    states = [h0]
    K = len(csrs)
    for k in range(K):
        c = SR.plain_case(states[-1], *csrs[k], xcls, *det(comps[k % 2]), *det((lw, lb)), torch.zeros_like(h0), None)
        states.append(SR.half_round(c)['h_out'])
    gd, ga = up, None
    acc = [dict(), dict()]
    for k in range(K - 1, -1, -1):
        c = SR.plain_case(states[k], *csrs[k], xcls, *det(comps[k % 2]), *det((lw, lb)), gd, ga)
        r = SR.half_round(c)
        gd, ga = r['g_direct'], r['g_agg']
        for name in SR.PARAM_OUT:
            if name in r:
                acc[k % 2][name] = acc[k % 2].get(name, 0) + r[name]
    return states, gd, ga, acc


def test_restatement_reproduces_the_reference_fixture():
    """g3_ops: enc_h0 -> enc_h1 -> enc_h2, enc_grad_h0, LayerNorm and raw-parameter gradients of the reference project's own run, composed
    as tests/test_hip_encoder.py composes them.  The fixture was COMPUTED in float32 by the reference (not merely stored in it), so it is
    float32-limited throughout; bounds from the count of float32 roundings behind an entry, each at most 2^-24 of the running magnitude:
    a state entry sits behind two 64-term and one 6-term dot product, the gates and LayerNorm (< 256 roundings: 256 * 2^-24 = 1.5e-5 of
    the tensor's scale); a gradient entry behind two stages of 192-term products and a sum over the 96 rows or 186 edges (< 1024:
    6.1e-5).  (tests/test_hip_encoder.py allows the device 2e-4 on the same fixture.)"""
    z = load_golden('g3_ops')
    H = 64
    raw = {k[len('enc_param_'):]: torch.tensor(z[k], dtype=F64, requires_grad=True) for k in z.files if k.startswith('enc_param_')}
    ei = torch.tensor(z['enc_edge_index'])
    N = z['enc_x'].shape[0]
    xcls = torch.tensor(z['enc_x']).argmax(1).to(torch.uint8)
    rows = torch.eye(6, dtype=F64)
    cf, cr = _compose(raw, 'aggr', 'update', H, rows), _compose(raw, 'aggr_r', 'update_r', H, rows)
    csrs = [SR.csr(ei[1], ei[0], N), SR.csr(ei[0], ei[1], N)]
    states, gd0, ga0, acc = _chain(torch.tensor(z['enc_h0'], dtype=F64), csrs, xcls, (cf, cr), raw['ln.weight'], raw['ln.bias'],
                                   torch.tensor(z['enc_up'], dtype=F64))
    g_h0 = gd0.clone().index_add_(0, ei[0], ga0[ei[1]])
    order = ('dxtab', 'dWc', 'dbc', 'dWhh', 'dbhh')
    torch.autograd.backward(cf + cr, [acc[0][k] for k in order] + [acc[1][k] for k in order])
    got = {'enc_h1': states[1], 'enc_h2': states[2], 'enc_grad_h0': g_h0, 'enc_grad_ln.weight': acc[0]['dln_w'] + acc[1]['dln_w'],
           'enc_grad_ln.bias': acc[0]['dln_b'] + acc[1]['dln_b']}
    got.update({'enc_grad_' + k: v.grad for k, v in raw.items() if not k.startswith('ln.')})
    for k, v in got.items():
        ref = torch.tensor(z[k], dtype=F64)
        bound = (256 if k in ('enc_h1', 'enc_h2') else 1024) * U24
        err = float((v.detach() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        print('%-40s %.3g of scale (bound %.3g)' % (k, err, bound))
        assert err <= bound, k


def test_restatement_composes_to_the_oracle_encoder():
    """Two rounds = four half rounds with the g_agg -> gy_agg hand-over between opposite CSRs, against oracle/ref_cpu.struct_encoder
    run in float64 on a small synthetic batch: states and every parameter gradient to 1e-9 of scale (float64 against float64 in
    another operation order)."""
    from deepgate import synthetic as syn
    from oracle import ref_cpu as R
    H, rounds = 32, 2
    arrays = syn.collate([syn.make_graph('aig', 148, 8, 21 + i, n_inputs=20) for i in range(2)])
    N = arrays['num_nodes']
    ei = torch.from_numpy(arrays['edge_index'])
    g = torch.Generator().manual_seed(5)
    xcls = torch.randint(0, 6, (N,), generator=g).to(torch.uint8)
    x = torch.eye(6, dtype=F64)[xcls.long()]
    raw = {}
    for conv in ('source_conv', 'target_conv'):
        for a, u in (('aggr', 'update'), ('aggr_r', 'update_r')):
            raw['enc.%s.%s.msg.weight' % (conv, a)] = 0.3 * torch.randn(H, H, generator=g, dtype=F64)
            raw['enc.%s.%s.msg.bias' % (conv, a)] = 0.1 * torch.randn(H, generator=g, dtype=F64)
            raw['enc.%s.%s.weight_ih_l0' % (conv, u)] = 0.2 * torch.randn(3 * H, H + 6, generator=g, dtype=F64)
            raw['enc.%s.%s.weight_hh_l0' % (conv, u)] = 0.2 * torch.randn(3 * H, H, generator=g, dtype=F64)
            raw['enc.%s.%s.bias_ih_l0' % (conv, u)] = 0.1 * torch.randn(3 * H, generator=g, dtype=F64)
            raw['enc.%s.%s.bias_hh_l0' % (conv, u)] = 0.1 * torch.randn(3 * H, generator=g, dtype=F64)
        raw['enc.%s.ln.weight' % conv] = 1 + 0.2 * torch.randn(H, generator=g, dtype=F64)
        raw['enc.%s.ln.bias' % conv] = 0.1 * torch.randn(H, generator=g, dtype=F64)
    po = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    so, to = R.struct_encoder(po, 'enc', x, ei, rounds, rounds, layernorm=True)
    ups = [1.3 * torch.randn(N, H, generator=g, dtype=F64) for _ in range(2)]
    ((so * ups[0]).sum() + (to * ups[1]).sum()).backward()
    csrs = [SR.csr(ei[1], ei[0], N), SR.csr(ei[0], ei[1], N)] * rounds
    worst = 0.0
    for conv, ref_out, up in (('source_conv', so, ups[0]), ('target_conv', to, ups[1])):
        pre = 'enc.%s.' % conv
        mine = {k[len(pre):]: v.clone().requires_grad_(True) for k, v in raw.items() if k.startswith(pre)}
        cf, cr = _compose(mine, 'aggr', 'update', H, torch.eye(6, dtype=F64)), _compose(mine, 'aggr_r', 'update_r', H, torch.eye(6, dtype=F64))
        states, _, _, acc = _chain(torch.ones(N, H, dtype=F64), csrs, xcls, (cf, cr), mine['ln.weight'], mine['ln.bias'], up)
        order = ('dxtab', 'dWc', 'dbc', 'dWhh', 'dbhh')
        torch.autograd.backward(cf + cr, [acc[0][k] for k in order] + [acc[1][k] for k in order])
        pairs = [('state', states[-1], ref_out.detach()), ('ln.weight', acc[0]['dln_w'] + acc[1]['dln_w'], po[pre + 'ln.weight'].grad),
                 ('ln.bias', acc[0]['dln_b'] + acc[1]['dln_b'], po[pre + 'ln.bias'].grad)]
        pairs += [(k, v.grad, po[pre + k].grad) for k, v in mine.items() if not k.startswith('ln.')]
        for k, a, b in pairs:
            err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            worst = max(worst, err)
            assert err <= 1e-9, (conv, k, err)
    print('four chained half rounds against the oracle encoder: worst %.3g of scale' % worst)


# ------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize('size', list(SR.SIZES))
def test_builder_places_every_row_path(size):
    N = SR.SIZES[size]
    full = N // SR.TILE
    c = SR.case(64, size, 'empty')
    assert c['E'] == 0 and c['idx'].numel() == 1 and int(c['ptr'].abs().sum()) == 0 and c['heavy'][0] == 0
    c = SR.case(64, size, 'small')
    p = SR.paths(c)
    assert all(t['chunked'] == t['full'] for t in p['tiles']) and len(p['heavy']) == 0
    if full >= 2:
        assert p['tiles'][1]['total'] == 0 and p['tiles'][1]['chunked']                      # a chunked tile of empty lists
        assert set(range(8)) <= set(int(d) for d in p['tiles'][0]['degs'])                   # 0..7: below, at and above D = 2, 3 and 2 D
    c = SR.case(64, size, 'designed')
    p = SR.paths(c)
    deg = (c['ptr'][1:] - c['ptr'][:-1]).numpy()
    n_h, nodes = c['heavy']
    assert nodes.tolist() == sorted(np.nonzero(deg > SR.HEAVY_ROW)[0].tolist()) and n_h == nodes.numel() and n_h >= 1
    assert deg.max() <= SR.HUB and nodes[0] == 0 and nodes[-1] == N - 1                      # heavy rows as node 0 and as node N - 1
    if N >= 2:
        assert deg[0] == SR.HUB and deg[N - 1] == SR.LAST_ROW
    if N % SR.TILE:
        assert p['tiles'][-1]['reason'] == 'partial' and N - 1 in p['heavy_generic']         # a heavy row inside the partial last tile
    if N >= 8:
        assert set(SR.LADDER) <= set(deg.tolist())
    if full >= 6:
        t = p['tiles']
        assert (t[0]['reason'], t[0]['dmax']) == ('cap', SR.HUB)
        assert (t[2]['total'], t[2]['reason']) == (504, '') and (t[3]['total'], t[3]['reason']) == (505, 'cap')
        assert (t[4]['total'], t[4]['reason'], t[4]['dmax']) == (504, '', SR.ON_CHUNKED) and p['heavy_chunked'][0] == 4 * SR.TILE + 10
        assert t[5]['reason'] == 'cap' and set(SR.LADDER) <= set(int(d) for d in t[5]['degs'])
        assert 64 in t[5]['degs'] and 5 * SR.TILE + 3 not in nodes.tolist() and 5 * SR.TILE + 4 in nodes.tolist()     # 64 is not heavy, 65 is
        assert all(x['chunked'] for x in t[6:full])
        if N % SR.TILE == 0:
            assert N - 1 in p['heavy_chunked']
    if N >= 64:
        ptr, idx = c['ptr'].long(), c['idx'].long()
        has = deg >= 2
        assert bool((idx[ptr[:-1][has]] == idx[ptr[:-1][has] + 1]).any())                   # a repeated entry
        assert bool((idx[ptr[:-1][deg >= 1]] == torch.arange(N)[deg >= 1]).any())           # a self entry


@pytest.mark.parametrize('size', ['n1', 'n65', 't9', 't257'])
def test_builder_index_forms(size):
    N = SR.SIZES[size]
    c = SR.case(64, size, mode='tagged')
    ent = c['idx'][:c['E']]
    neg = float((ent < 0).float().mean())
    tag, node = (ent.long() & 0xffffffff) >> 24, ent.long() & 0xffffff
    assert c['h_in'].shape[0] == 256 and int(node.max()) < N and c['gy_agg'].shape[0] == N and c['own_idx'].numel() == N
    assert int(tag.max()) >= 128 and (N < 64 or 0.3 < neg < 0.7), neg                       # rows >= 128: negative as int32
    if N >= 64:
        assert int(tag.max()) > 250 and int(tag.min()) < 5 and int(c['own_idx'].max()) >= 128
        assert bool((node[c['ptr'].long()[:-1][(c['ptr'][1:] > c['ptr'][:-1])]] == torch.arange(N)[(c['ptr'][1:] > c['ptr'][:-1])]).any())
    few, more, nr = SR.case(64, size, mode='own_few'), SR.case(64, size, mode='own_more'), SR.case(64, size, mode='n_rows')
    assert few['h_in'].shape[0] < N or N == 1
    assert more['h_in'].shape[0] > N and nr['h_in'].shape[0] > N and nr['own_idx'] is None
    for q in (few, more, nr):
        assert int(q['idx'].max()) < q['R'] and q['gy_agg'].shape[0] == q['R'] and not q['tagged']
    if N >= 64:
        assert int(more['idx'].max()) >= N and int(more['own_idx'].max()) >= N and int(nr['idx'].max()) >= N
        assert bool((few['own_idx'].long() != torch.arange(N)).any())
    for C in (1, 6, 8):
        q = SR.case(64, size, C=C)
        cls = q['xcls'].long()
        assert int(cls.max()) < C and q['xtab'].shape == (C, 192)
        if C > 1:
            assert q['absent'] == C - 2 and not bool((cls == q['absent']).any())
            if N >= 64:
                assert set(cls.tolist()) == set(range(C)) - {q['absent']}


def test_tile_order_visits_every_tile_once():
    """grid_for / tile_seq restated: every tile exactly once at every named size and every co-residency the launchers use; the XCD
    order at grids that are multiples of 8 and round-robin otherwise; at 257 tiles the grid is capped at 256, some workgroups take
    two tiles and some of the last eighth none; at 513 tiles a workgroup takes up to three."""
    seen_kind = set()
    for size, N in SR.SIZES.items():
        nt = (N + SR.TILE - 1) // SR.TILE
        for per_cu in (1, 2, 3, 4):
            grid = SR.grid_for(nt, per_cu)
            seqs = [SR.tile_seq(nt, grid, b) for b in range(grid)]
            assert sorted(t for s in seqs for t in s) == list(range(nt)), (size, per_cu)
            if per_cu == 1:
                seen_kind.add((size, 'xcd' if grid % 8 == 0 else 'rr', max(len(s) for s in seqs), sum(1 for s in seqs if not s)))
    kinds = {k[0]: k[1:] for k in seen_kind}
    assert [kinds[s][0] for s in ('t7', 't8', 't9', 't16', 't17', 't20')] == ['rr', 'xcd', 'rr', 'xcd', 'rr', 'rr']
    assert kinds['t256'] == ('xcd', 1, 0)
    assert kinds['t257'][0] == 'xcd' and kinds['t257'][1] == 2 and kinds['t257'][2] > 0
    idle = [b for b in range(256) if not SR.tile_seq(257, 256, b)]
    assert idle and all(b & 7 == 7 for b in idle)                                            # idle workgroups: the last eighth's only
    assert kinds['t300'][1] == 2 and kinds['t513'][1] == 3 and kinds['m260'][1] == 2
    assert SR.SIZES['m260'] % SR.TILE == 0 and SR.SIZES['m260'] // SR.TILE > SR.GRID_CAP
    assert SR.SIZES['t513'] <= 33000


# ------------------------------------------------------------------------------------------------ sensitivity
@functools.lru_cache(maxsize=None)
def _clean(H, size, mode, mm):
    c = SR.case(H, size, mode=mode)
    r64 = SR.half_round(c)
    r = SR.ratios(SR.half_round(c, F32, 'x3' if mm == 'x3' else 'exact'), r64)
    return c, r64, {k: 8 * max(v, FLOOR[mm]) for k, v in r.items()}, r


def _excess(c, r64, tau, mm, mutate):
    got = SR.ratios(SR.half_round(c, F32, 'x3' if mm == 'x3' else 'exact', mutate=mutate), r64)
    return {k: v / tau[k] for k, v in got.items()}


FWD = ('h_out', 'mean', 'rstd')
MUTATIONS = [
    ('last entry of the 600-entry list lost', 't9', 'plain', ('drop_entry', 0, -1)),
    ('last entry of a 129-entry list lost (the pre-pass tail)', 't9', 'plain', ('drop_entry', 5 * 64 + 7, -1)),
    ('entry D + 1 of a row lost, D = 2', 't9', 'plain', ('drop_entry', 6 * 64 + 11, 2)),
    ('entry D + 1 of a row lost, D = 3', 't9', 'tagged', ('drop_entry', 6 * 64 + 11, 3)),
    ('own row read instead of own_idx (table)', 't9', 'tagged', ('own_identity',)),
    ('own row read instead of own_idx (quotient form)', 't9', 'own_few', ('own_identity',)),
    ('deg * bc forgotten', 't9', 'plain', ('no_deg_bc',)),
    ('tag used where the node id belongs', 't9', 'tagged', ('tag_for_node',)),
    ('another row\'s {mean, rstd} reused', 't9', 'plain', ('stale_stats', 300, 299)),
    ('one tile\'s share of dbhh skipped at 257 tiles', 't257', 'plain', ('skip_tile_dbhh', 200)),
]


@pytest.mark.parametrize('mm', ['f32', 'x3'])
@pytest.mark.parametrize('what,size,mode,mutate', MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_planted_defect_is_far_outside_the_device_bound(what, size, mode, mutate, mm):
    """Each defect, planted in the float32 / bf16x3 restatement, exceeds tau S (tau = 8 max(r, floor) per output, as the device tests
    assert it) by at least 10x on some output; a lost list entry on the forward outputs alone as well (the forward kernels return
    nothing else) and on the backward outputs alone."""
    c, r64, tau, _ = _clean(64, size, mode, mm)
    if mutate[0] == 'drop_entry':
        assert int(c['ptr'][mutate[1] + 1] - c['ptr'][mutate[1]]) > (mutate[2] if mutate[2] >= 0 else 0)
    ex = _excess(c, r64, tau, mm, mutate)
    worst = max(ex, key=ex.get)
    print('%s [%s]: %.3g x the bound on %s' % (what, mm, ex[worst], worst))
    assert ex[worst] >= 10
    if mutate[0] in ('drop_entry', 'own_identity', 'no_deg_bc'):
        assert max(ex[k] for k in FWD) >= 10, {k: ex[k] for k in FWD}
        assert max(v for k, v in ex.items() if k not in FWD) >= 10
    if mutate[0] == 'skip_tile_dbhh':
        assert worst == 'dbhh'


@pytest.mark.parametrize('H', [32, 64])
def test_x3_emulation_is_split_precision(H):
    """The emulation's own error against float64 is larger than float32's (it is not exact) and below 2^-14 of scale on every output
    (plain bf16 operands would be at 2^-9)."""
    for size, mode in (('t20', 'plain'), ('t20', 'tagged')):
        _, _, _, r3 = _clean(H, size, mode, 'x3')
        _, _, _, r32 = _clean(H, size, mode, 'f32')
        print(H, size, mode, {k: '%.2g / %.2g' % (r3[k], r32[k]) for k in r3})
        for k in ('h_out', 'g_direct', 'g_agg', 'dWc', 'dWhh'):
            assert r3[k] > r32[k], k
        assert max(r3.values()) < 2.0 ** -14


# ------------------------------------------------------------------------------------------------ host-side refusals
_STAGE_ENTRIES = {'fwd': 64, 'bwd': 64, 'rows_fwd': 64, 'rows_bwd': 64, 'fwd_x3': 64, 'bwd_x3': 32, 'bwd2_x3': 64}      # mgv_struct_stage_<entry>: H of its valid call
OK, E, U, D = 0, -1, -2, 'dummy'        # MGV_OK, MGV_EINVAL, MGV_EUNSUPPORTED; D: a non-NULL pointer where the valid call has NULL
# (overrides of the valid call, return code).  The valid call: H as above, N = 65, C = 6, every pointer non-NULL but heavy_nodes / heavy_ws /
# table_own_idx (heavy_n = 0, nbr_tagged = 0), workspace_floats = mgv_struct_stage_bwd2_ws_floats(64, 65) (written as an offset from it).
# Every code is what the library of the commit before the first backward lost H = 64 returned for the row (the table was run against
# that build through MGV_LIB); the one row that differs by design is the last of bwd_x3.  The rows behind "N=0, nbr_idx=None" pin the
# order of each entry: argument check, N == 0, nbr_idx, width (bwd2: width in front of N == 0, heavy and tagged lists behind nbr_idx).
_STAGE_REFUSALS = {
    'fwd': [
        (dict(H=48), U), (dict(C=0), E), (dict(C=9), E), (dict(C=9, H=48), E), (dict(ln_w=None), E), (dict(ln_b=None), E), (dict(h_in=None), E),
        (dict(nbr_ptr=None), E), (dict(xcls=None), E), (dict(xtab=None), E), (dict(Wc=None), E), (dict(bc=None), E), (dict(Whh=None), E),
        (dict(bhh=None), E), (dict(h_out=None), E), (dict(N=-1), E), (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK), (dict(H=48, N=0), OK),
        (dict(H=48, nbr_idx=None), E)
    ],
    'bwd': [
        (dict(H=128), U), (dict(C=0), E), (dict(C=9), E), (dict(C=9, H=128), E), (dict(ln_w=None), E), (dict(ln_b=None), E),
        (dict(g_direct_out=None), E), (dict(g_agg_out=None), E), (dict(h_in=None), E), (dict(nbr_ptr=None), E), (dict(xcls=None), E),
        (dict(xtab=None), E), (dict(Wc=None), E), (dict(WcT=None), E), (dict(bc=None), E), (dict(Whh=None), E), (dict(WhhT=None), E),
        (dict(bhh=None), E), (dict(gy_direct=None), E), (dict(dWc=None), E), (dict(dbc=None), E), (dict(dWhh=None), E), (dict(dbhh=None), E),
        (dict(dxtab=None), E), (dict(dln_w=None), E), (dict(dln_b=None), E), (dict(N=-1), E), (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK)
    ],
    'rows_fwd': [
        (dict(H=48), U), (dict(ln_w=None), E), (dict(ln_b=None), E), (dict(h_in=None), E), (dict(nbr_ptr=None), E), (dict(xrow=None), E),
        (dict(Wc=None), E), (dict(bc=None), E), (dict(Whh=None), E), (dict(bhh=None), E), (dict(h_out=None), E), (dict(N=-1), E),
        (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK)
    ],
    'rows_bwd': [
        (dict(H=128), U), (dict(ln_w=None), E), (dict(ln_b=None), E), (dict(g_direct_out=None), E), (dict(g_agg_out=None), E), (dict(h_in=None), E),
        (dict(nbr_ptr=None), E), (dict(xrow=None), E), (dict(Wc=None), E), (dict(WcT=None), E), (dict(bc=None), E), (dict(Whh=None), E),
        (dict(WhhT=None), E), (dict(bhh=None), E), (dict(gy_direct=None), E), (dict(dWc=None), E), (dict(dbc=None), E), (dict(dWhh=None), E),
        (dict(dbhh=None), E), (dict(d_xrow=None), E), (dict(dln_w=None), E), (dict(dln_b=None), E), (dict(N=-1), E), (dict(nbr_idx=None), E),
        (dict(N=0, nbr_idx=None), OK), (dict(H=128, N=0), OK), (dict(H=128, nbr_idx=None), E)
    ],
    'fwd_x3': [
        (dict(H=16), U), (dict(C=0), E), (dict(C=9), E), (dict(C=9, H=16), E), (dict(ln_w=None), E), (dict(ln_b=None), E), (dict(h_in=None), E),
        (dict(nbr_ptr=None), E), (dict(xcls=None), E), (dict(xtab=None), E), (dict(wpack_bf16=None), E), (dict(bc=None), E), (dict(bhh=None), E),
        (dict(h_out=None), E), (dict(N=-1), E), (dict(heavy_n=-1), E), (dict(heavy_n=1, heavy_ws=D), E), (dict(heavy_n=1, heavy_nodes=D), E),
        (dict(N=1 << 24, table_own_idx=D, nbr_tagged=1), E), (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK), (dict(H=16, N=0), OK),
        (dict(N=0, heavy_n=-1), E), (dict(H=16, nbr_idx=None), E)
    ],
    'bwd_x3': [
        (dict(H=16), U), (dict(C=0), E), (dict(C=9), E), (dict(C=9, H=16), E), (dict(ln_w=None), E), (dict(ln_b=None), E),
        (dict(g_direct_out=None), E), (dict(g_agg_out=None), E), (dict(h_in=None), E), (dict(nbr_ptr=None), E), (dict(xcls=None), E),
        (dict(xtab=None), E), (dict(wpack_bf16=None), E), (dict(bc=None), E), (dict(bhh=None), E), (dict(gy_direct=None), E), (dict(dWc=None), E),
        (dict(dbc=None), E), (dict(dWhh=None), E), (dict(dbhh=None), E), (dict(dxtab=None), E), (dict(dln_w=None), E), (dict(dln_b=None), E),
        (dict(N=-1), E), (dict(heavy_n=-1), E), (dict(heavy_n=1, heavy_ws=D), E), (dict(heavy_n=1, heavy_nodes=D), E),
        (dict(N=1 << 24, table_own_idx=D, nbr_tagged=1), E), (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK), (dict(H=16, N=0), OK),
        (dict(N=0, heavy_n=-1), E), (dict(H=16, nbr_idx=None), E)
    ],
    'bwd2_x3': [
        (dict(H=16), U), (dict(H=32), U), (dict(C=0), E), (dict(C=9), E), (dict(C=9, H=16), E), (dict(ln_w=None), E), (dict(ln_b=None), E),
        (dict(g_direct_out=None), E), (dict(g_agg_out=None), E), (dict(h_in=None), E), (dict(nbr_ptr=None), E), (dict(xcls=None), E),
        (dict(xtab=None), E), (dict(wpack_bf16=None), E), (dict(bc=None), E), (dict(bhh=None), E), (dict(gy_direct=None), E), (dict(dWc=None), E),
        (dict(dbc=None), E), (dict(dWhh=None), E), (dict(dbhh=None), E), (dict(dxtab=None), E), (dict(dln_w=None), E), (dict(dln_b=None), E),
        (dict(N=-1), E), (dict(heavy_n=-1), E), (dict(heavy_n=1, heavy_ws=D), E), (dict(heavy_n=1, heavy_nodes=D), E),
        (dict(N=1 << 24, table_own_idx=D, nbr_tagged=1), E), (dict(workspace_floats=-1), E), (dict(nbr_idx=None), E), (dict(N=0, nbr_idx=None), OK),
        (dict(H=16, N=0), U), (dict(N=0, heavy_n=-1), OK), (dict(H=16, heavy_n=-1), U), (dict(H=16, nbr_idx=None), U)
    ],
}
_STAGE_REFUSALS['bwd_x3'].append((dict(H=64), U))       # every argument valid: the first backward serves H = 32 only


def test_stage_entries_refuse_on_the_host_before_any_launch():
    """All seven struct-stage entries over rows that return before anything is launched or any pointer is read: an unserved width, C
    outside 1 .. 8, half a LayerNorm, half an input gradient, every checked pointer NULL in turn, N = -1, a bad heavy list, the tagged
    form at N = 2^24, bwd2 one float short of workspace, N > 0 without nbr_idx, N = 0 without it (accepted), and which of two faults
    wins.  The pointers are dummies, so this runs only where no device could be reached through them; the same rows with real buffers
    that must come back untouched: tests/test_hip_struct_stage_reference.py::test_refusals_are_return_codes."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host only')
    import ctypes
    import re
    from deepgate import _hip
    lib, sigs = _hip.load(), _hip.parse_header()
    with open(_hip.HEADER_PATH) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    dummy = ctypes.c_void_p(64)
    N = 65
    nws = lib.mgv_struct_stage_bwd2_ws_floats(64, N)
    assert nws == 2 * 28800
    n = 0
    for entry, H in _STAGE_ENTRIES.items():
        name = 'mgv_struct_stage_' + entry
        decl = re.search(r'\bint\s+%s\s*\(([^;{]*?)\)\s*;' % name, header, flags=re.S).group(1)
        names = [re.search(r'(\w+)\s*$', a).group(1) for a in decl.split(',')]
        assert len(names) == len(sigs[name])
        valid = dict(H=H, N=N, C=6, ln_eps=1e-5, heavy_n=0, heavy_nodes=None, heavy_ws=None, table_own_idx=None, nbr_tagged=0,
                     workspace_floats=0, stream=None)
        for over, code in _STAGE_REFUSALS[entry]:
            assert set(over) <= set(names), (entry, over)
            args = dict({k: dummy for k in names}, **{k: v for k, v in valid.items() if k in names})
            args.update({k: dummy if v is D else v for k, v in over.items()})
            if 'workspace_floats' in args:
                args['workspace_floats'] += nws
            assert getattr(lib, name)(*[args[k] for k in names]) == code, (entry, over)
            n += 1
    assert n == 184
