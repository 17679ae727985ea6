"""CPU checks of tests/sweep_ref.py, the float64 restatement the device tests of the level-sweep and attention-pool kernels
(tests/test_hip_sweep_reference.py) compare with:

  * pins: the reference project's own fixture g3_ops (lvl_*: one level of TFMlpAggr + GRU from a non-zero state, outputs and every
    gradient), oracle/ref_cpu.py's tf_mlp_aggr + gru_cell in float64 with random module weights, and a 6-level graph with three
    gate types against oracle/ref_cpu.model_forward's plain level loop;
  * the properties of the case builders the device tests rely on;
  * planted defects: each one, run in the float32 restatement (and the bf16x3 one where it applies), is at least 10 times outside
    the bound the device tests assert for the output it hits.  The table is in NOTEBOOK.md (2026-10-18)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as W  # noqa: E402
from conftest import load_golden  # noqa: E402

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ pins
def _compose(p, a, g, H):
    """The kernels' per-slot tensors from a TFMlpAggr `a` and a GRU `g` by the header's formulas (include/mgvae_hip.h):
    attn_u = Wk^T w_attn[H:], Wvc = W_ih Wv, bvc = W_ih bv, bih."""
    w_ih = p[g + '.weight_ih_l0']
    return (p[a + '.msg_k.weight'].t() @ p[a + '.attn_lin.weight'][0, H:], w_ih @ p[a + '.msg_v.weight'], w_ih @ p[a + '.msg_v.bias'], p[g + '.bias_ih_l0'])


def _one_level(z, p, state):
    """The fixture's level as a sweep case in float64: 16 gates (nodes 20 .. 35, fan-in 1 .. 5 from nodes 0 .. 19) on level 1, three
    unrelated edges into nodes nobody updates.  The sources' functional rows are not zero in the fixture, so the level is run in the
    rounds >= 2 form: `state` [N, H] holds the sources' hf rows and the gates' own previous states, gh = W_hh state + b_hh.
    Returns (case, composed tensors, gh, the state leaf)."""
    H = 64
    ns = torch.tensor(z['lvl_node_state'], dtype=F64)
    nodes = z['lvl_nodes']
    N = ns.shape[0]
    gate, level = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    gate[nodes], level[nodes] = 1, 1
    comp = _compose(p, 'a', 'g', H)
    hp = state.clone().requires_grad_(True)
    gh = hp @ p['g.weight_hh_l0'].t() + p['g.bias_hh_l0']
    c = {'H': H, 'N': N, 'T': 1, 'gate_ids': [1], 'ei': z['lvl_edge_index'].astype(np.int64), 'gate': gate, 'level': level, 'hs': ns[:, :H].clone(),
         'attn_u': comp[0].detach()[None], 'Wvc': comp[1].detach()[None], 'bvc': comp[2].detach()[None], 'bih': comp[3].detach()[None],
         'bhh': torch.zeros(1, 3 * H, dtype=F64), 'ghf': torch.zeros(N, H, dtype=F64), 'h_prev': state.clone(), 'gh': gh.detach()}
    c['ghf'][nodes] = torch.tensor(z['lvl_up'], dtype=F64)
    return c, comp, gh, hp


def _fixture_sweep(z, p, with_state):
    """Run the restatement on the fixture's level and push its gradients through the composition to the module's parameters."""
    H = 64
    ns = torch.tensor(z['lvl_node_state'], dtype=F64)
    nodes = torch.tensor(z['lvl_nodes'])
    state = ns[:, H:].clone()
    state[nodes] = torch.tensor(z['lvl_hprev'], dtype=F64)[nodes] if with_state else 0.0        # lvl0_*: the gates themselves start from zero
    c, comp, gh, hp = _one_level(z, p, state)
    r = W.sweep(c)
    torch.autograd.backward(list(comp) + [gh], [r['d_attn_u'][0], r['dWvc'][0], r['dbvc'][0], r['dbih'][0], r['d_gh']])
    return c, r, hp


def _raw(z, dtype=F64):
    p = {'a.' + k[len('lvl_aggr_'):]: torch.tensor(z[k], dtype=dtype, requires_grad=True) for k in z.files if k.startswith('lvl_aggr_')}
    p.update({'g.' + k[len('lvl_gru_'):]: torch.tensor(z[k], dtype=dtype, requires_grad=True) for k in z.files if k.startswith('lvl_gru_')})
    return p


def test_restatement_reproduces_the_reference_fixture():
    """g3_ops lvl_* (from a non-zero state: the rounds >= 2 form) and lvl0_* (the gates' own states zero): the new rows, the gradient of
    the hs half of node_state, of hprev and of every module parameter.  The fixture was COMPUTED in float32 by the reference, so bounds
    come from the count of float32 roundings behind an entry, each at most 2^-24 of the running magnitude: a state entry sits behind
    two 128-term dot products per in-edge (k, v), the softmax, a 64-term and a 128-term product and the gates (< 512 roundings: 3.1e-5
    of the tensor's scale); a gradient entry behind the same chain backwards and a sum over 16 rows or 48 edges (< 1024: 6.1e-5)."""
    z = load_golden('g3_ops')
    H = 64
    nodes = torch.tensor(z['lvl_nodes'])
    for tag, with_state in (('lvl', True), ('lvl0', False)):
        p = _raw(z)
        c, r, hp = _fixture_sweep(z, p, with_state)
        got = {tag + '_hnew': r['hf'][nodes], tag + '_grad_node_state': r['ghs']}
        if with_state:
            got['lvl_grad_hprev'] = (r['g_hprev'] + hp.grad)[nodes]
        for k, v in p.items():
            name = tag + '_grad_' + ('aggr_' if k.startswith('a.') else 'gru_') + k[2:]
            if name in z.files and v.grad is not None:
                got[name] = v.grad
        for k, v in got.items():
            ref = torch.tensor(z[k], dtype=F64)
            if k.endswith('grad_node_state'):
                ref = ref[:, :H]
            if k == 'lvl_grad_hprev':
                ref = ref[nodes]
            if k.endswith('attn_lin.weight'):
                v, ref = v[:, H:], ref[:, H:]            # (the q half cancels inside a softmax segment: the restatement has no such parameter)
            bound = (512 if k.endswith('hnew') else 1024) * U24
            err = float((v.detach() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
            print('%-44s %.3g of scale (bound %.3g)' % (k, err, bound))
            assert err <= bound, k
        assert len(got) >= (11 if with_state else 9), sorted(got)


def test_restatement_matches_the_oracle_aggregator_and_gru_in_float64():
    """oracle/ref_cpu.tf_mlp_aggr + gru_cell in float64 with random module weights on the fixture's graph: every output and gradient to
    1e-9 of scale (float64 against float64 in another operation order, with the q term and the message bias restated away)."""
    from oracle import ref_cpu as R
    z = load_golden('g3_ops')
    H = 64
    g = torch.Generator().manual_seed(3)
    p = {k: (0.3 * torch.randn(v.shape, generator=g, dtype=F64)).requires_grad_(True) for k, v in _raw(z).items()}
    ns = torch.tensor(z['lvl_node_state'], dtype=F64)
    nodes = torch.tensor(z['lvl_nodes'])
    state = ns[:, H:].clone()
    state[nodes] = torch.randn(nodes.numel(), H, generator=g, dtype=F64)
    ei = torch.tensor(z['lvl_edge_index'])
    keep = torch.isin(ei[1], nodes)
    src, dst = ei[0][keep], ei[1][keep]
    order = torch.sort(dst, stable=True).indices
    src, dst = src[order], dst[order]
    po = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    hs_o, hp_o = ns[:, :H].clone().requires_grad_(True), state.clone().requires_grad_(True)
    x = torch.cat([hs_o, state], 1)
    msg = R.tf_mlp_aggr(po, 'a', x[src], x[dst], torch.searchsorted(nodes, dst), nodes.numel())
    hn = R.gru_cell(po, 'g', msg, hp_o[nodes])
    up = torch.tensor(z['lvl_up'], dtype=F64)
    (hn * up).sum().backward()
    c, comp, gh, hp = _one_level(z, p, state)
    r = W.sweep(c)
    torch.autograd.backward(list(comp) + [gh], [r['d_attn_u'][0], r['dWvc'][0], r['dbvc'][0], r['dbih'][0], r['d_gh']])
    pairs = [('hf', r['hf'][nodes], hn.detach()), ('ghs', r['ghs'], hs_o.grad), ('h_prev', (r['g_hprev'] + hp.grad)[nodes], hp_o.grad[nodes])]
    for k, v in p.items():
        if k.startswith('a.msg_q') or k in ('a.attn_lin.bias', 'a.msg_k.bias'):
            assert po[k].grad is None or float(po[k].grad.abs().max()) <= 1e-12, k       # they cancel in the oracle too
            continue
        a, b = v.grad, po[k].grad
        if k == 'a.attn_lin.weight':
            a, b = a[:, H:], b[:, H:]
        pairs.append((k, a, b))
    for k, a, b in pairs:
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        assert err <= 1e-9, (k, err)


def test_restatement_matches_the_oracle_level_loop_on_six_levels():
    """Six levels, three gate types (xag): hf and the gradient of hs against oracle/ref_cpu.model_forward's plain level loop in float64,
    to 1e-9 of scale."""
    import deepgate
    from deepgate import synthetic as syn
    from oracle import ref_cpu as R
    H, ctype = 32, 'xag'
    torch.manual_seed(4)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = getattr(deepgate, 'dg_ae_model_' + ctype).Model(struct_encoder=enc, dim_hidden=H)
    p = {k: (v.to(F64) if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    arrays = syn.collate([syn.make_graph(ctype, 158, 6, 40 + i, n_inputs=14) for i in range(2)])
    batch = R.batch_from_arrays(lambda k: arrays[k])
    hs, hf, _, _ = R.model_forward(p, ctype, batch, 1, 1)
    hs = hs.detach().requires_grad_(True)

    def level_loop(hs_in):          # model_forward's level loop from a given hs (it forms hs itself: re-run the loop on a leaf)
        plan = R.LevelPlan(ctype, batch['edge_index'], batch['gate'], batch['forward_level'])
        h = torch.zeros_like(hs_in)
        for lv in range(1, plan.num_levels):
            writes = []
            for level, gname, nodes, esrc, seg in plan.groups:
                if level != lv:
                    continue
                x_src = torch.cat([hs_in[esrc], h[esrc]], 1)
                dn = nodes[seg]
                msg = R.tf_mlp_aggr(p, 'aggr_%s_func' % gname, x_src, torch.cat([hs_in[dn], h[dn]], 1), seg, nodes.numel())
                writes.append((nodes, R.gru_cell(p, 'update_%s_func' % gname, msg, h[nodes])))
            for nd, val in writes:
                h = h.index_put((nd,), val)
        return h
    hf_loop = level_loop(hs)
    assert float((hf_loop.detach() - hf.detach()).abs().max()) <= 1e-12      # the re-run loop IS model_forward's
    N = hs.shape[0]
    up = torch.randn(N, H, dtype=F64)
    ghs_ref, = torch.autograd.grad((hf_loop * up).sum(), hs)
    gates = R.GATES[ctype]
    comps = [_compose(p, 'aggr_%s_func' % n, 'update_%s_func' % n, H) for _, n in gates]
    c = {'H': H, 'N': N, 'T': len(gates), 'gate_ids': [g for g, _ in gates], 'ei': np.asarray(arrays['edge_index']).astype(np.int64),
         'gate': np.asarray(arrays['gate']).reshape(-1).astype(np.int64), 'level': np.asarray(arrays['forward_level']).astype(np.int64),
         'hs': hs.detach(), 'attn_u': torch.stack([q[0] for q in comps]), 'Wvc': torch.stack([q[1] for q in comps]), 'bvc': torch.stack([q[2] for q in comps]),
         'bih': torch.stack([q[3] for q in comps]), 'bhh': torch.stack([p['update_%s_func.bias_hh_l0' % n] for _, n in gates]), 'ghf': up, 'h_prev': None, 'gh': None}
    assert int(c['level'].max()) >= 5
    r = W.sweep(c)
    for k, a, b in (('hf', r['hf'], hf.detach()), ('ghs', r['ghs'], ghs_ref)):
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print('%s against the oracle level loop: %.3g of scale' % (k, err))
        assert err <= 1e-9, (k, err)


# ------------------------------------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def _shallow(H, T, seed=0, rounds2=False, fanout=True):
    return W.shallow(H, T, seed, rounds2, fanout)


def _degrees(c):
    plan = W.plan_of(c)
    return (plan.in_ptr[1:] - plan.in_ptr[:-1]).numpy(), (plan.out_ptr[1:] - plan.out_ptr[:-1]).numpy(), plan


@pytest.mark.parametrize('T', [1, 2, 5, 6])
def test_shallow_places_every_degree_slot_and_list(T):
    c = _shallow(32, T)
    ind, outd, plan = _degrees(c)
    gs = plan.gslot.numpy()
    lv = plan.level.numpy()
    assert plan.num_levels == 3
    upd = gs != W.NO_GATE
    assert set(W.FANINS) <= set(ind[upd & (lv == 1)].tolist()), 'every fan-in on an updated level-1 gate'
    assert [int(outd[v]) for v in c['pi_f']] == list(W.FANOUTS) and not upd[c['pi_f']].any()
    assert [int(outd[v]) for v in c['l1_f']] == list(W.FANOUTS) and upd[c['l1_f']].all() and (lv[c['l1_f']] == 1).all()
    # the heavy lists on both kinds of node, by GraphPlan.heavy_segments' own rule: 65 -> 1 segment, 513 -> 2, 1100 -> 3
    for kw, owners in (({'inactive_only': True}, c['pi_f']), ({'active_by_level': True}, c['l1_f'])):
        hv = plan.heavy_segments(True, **kw)
        nodes = hv['nodes'].tolist()
        nsp = hv['node_seg_ptr'].tolist()
        segs = {v: nsp[i + 1] - nsp[i] for i, v in enumerate(nodes)}
        assert [segs[owners[W.FANOUTS.index(f)]] for f in (65, 513, 1100)] == [1, 2, 3]
        assert owners[W.FANOUTS.index(64)] not in segs, '64 consumers are not heavy'
    # slots: the last one absent from the graph, slot T - 2 absent from level 1 (T >= 3); level-1 group sizes
    present1, present2 = set(gs[upd & (lv == 1)].tolist()), set(gs[upd & (lv == 2)].tolist())
    if T >= 2:
        assert T - 1 not in present1 | present2
    if T >= 3:
        assert T - 2 not in present1 and T - 2 in present2
    for s_, nodes in c['groups'].items():
        assert len(nodes) == W.GROUPS[s_ % len(W.GROUPS)]
    # never-updated sources on level 1 and never-updated consumers (nobody writes their alpha / dsc / dzb)
    assert all(gs[v] == W.NO_GATE and lv[v] == 1 and outd[v] > 0 for v in c['nev1'])
    src, dst = c['ei']
    never_cons = (gs[dst] == W.NO_GATE) & (lv[dst] >= 1)
    assert never_cons.sum() > 50 and upd[src[never_cons]].any() and (~upd[src[never_cons]]).any()
    # a repeated edge and a row of equal scores
    pairs = src * c['N'] + dst
    assert len(np.unique(pairs)) < len(pairs)
    r64 = W.sweep(c)
    e0 = int(plan.in_ptr[c['equal_row']])
    assert ind[c['equal_row']] == 3 and torch.allclose(r64['alpha'][e0:e0 + 3], torch.full((3,), 1 / 3, dtype=F64), atol=1e-12)


@pytest.mark.parametrize('rounds2', [False, True])
def test_spread_rows_are_spread_in_both_orders_and_finite(rounds2):
    c = _shallow(32, 5, rounds2=rounds2)
    plan = W.plan_of(c)
    r64 = W.sweep(c)
    x = torch.cat([c['hs'], c['h_prev'] if rounds2 else torch.zeros_like(c['hs'])], 1).to(F64)
    for row, first_largest in zip(c['spread_rows'], (True, False)):
        e0, e1 = int(plan.in_ptr[row]), int(plan.in_ptr[row + 1])
        sc = x[plan.in_src[e0:e1].long()] @ c['attn_u'][0].to(F64)
        assert float(sc.max() - sc.min()) > 100 and (int(sc.argmax()) == 0) == first_largest and (int(sc.argmax()) == e1 - e0 - 1) != first_largest
        al = r64['alpha'][e0:e1]
        assert bool(torch.isfinite(al).all()) and float(al.min()) > 0 and abs(float(al.sum()) - 1) < 1e-12
    for k, v in r64.items():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()), k


def test_tile_counts_of_the_widest_level_and_the_257_tile_slot():
    """The small-gradient slabs are summed over the tiles of the widest level, four at a time with a tail: 1, 3, 4 and 5 tiles."""
    got = {}
    for T, seed in ((1, 4), (1, 0), (5, 1), (6, 1)):
        ltp = W.plan_of(_shallow(32, T, seed, False, False)).level_tile_ptr
        got[(T, seed)] = max(ltp[i + 1] - ltp[i] for i in range(1, len(ltp) - 1))
    assert got == {(1, 4): 1, (1, 0): 3, (5, 1): 4, (6, 1): 5}, got
    for H in (32, 64):
        c = W.wide(H)
        plan = W.plan_of(c)
        assert plan.slot_tile_ptr == [0, W.WGRAD_GRID + 1] and int(plan.tile_count[-1]) == W.WIDE_LAST
        # mgv_common.h grid_for(tiles, 8) = min(max(tiles, 1), 256 * 8); rows_per_block = kThreads / (H / 4)
        rpb = W.THREADS // (H // 4)
        assert W.grid_for((c['N'] + rpb - 1) // rpb, 8) == 2048 and c['N'] == 2048 * rpb + 1
    d = W.deep(32)
    assert W.plan_of(d).num_levels == 40 and all(5 <= int((d['level'] == lv).sum()) <= 70 for lv in range(1, 40))


def test_pool_case_lists():
    c = W.pool_case(64, 20)
    deg = (c['ptr'][1:] - c['ptr'][:-1]).tolist()
    assert set(W.POOL_LISTS) <= set(deg) and deg[0] == 0
    r = W.attn_pool(c)
    assert float(r['inv'][0]) == 1e16 and float(r['mstat'][0]) == 0 and float(r['zbar'][0].abs().max()) == 0
    assert all(bool(torch.isfinite(v).all()) for k, v in r.items() if torch.is_tensor(v))
    assert W.pool_case(32, 1)['E'] == 0 and W.pool_case(32, 2)['E'] == 1


# ------------------------------------------------------------------------------------------------ planted defects
@functools.lru_cache(maxsize=None)
def _bounds(maker, mm):
    c = maker()
    r64 = W.sweep(c)
    rk = W.sweep(c, F32, 'x3' if mm == 'x3' else 'exact')
    return c, r64, W.device_taus(c, r64, rk, mm)


def _partial_tile_last_row(c, slot=None):
    plan = W.plan_of(c)
    for t in range(plan.num_tiles):
        if 1 < int(plan.tile_count[t]) < W.TILE and (slot is None or int(plan.tile_slot[t]) == slot):
            return int(W.tile_nodes(plan, t)[-1])
    raise AssertionError('no partial tile')


def _tile_of_slot(c, slot, level=1, which=0):
    plan = W.plan_of(c)
    ltp = plan.level_tile_ptr
    return [t for t in range(ltp[level], ltp[level + 1]) if int(plan.tile_slot[t]) == slot][which]


S5 = functools.partial(_shallow, 32, 5)
S5R = functools.partial(_shallow, 32, 5, 0, True)
S6N = functools.partial(_shallow, 32, 6, 1, False, False)
WIDE = functools.lru_cache(maxsize=None)(functools.partial(W.wide, 32))
COH = functools.lru_cache(maxsize=None)(functools.partial(W.coherent, 32))

DEFECTS = [
    ('the 4th in-edge lost', S5, lambda c: ('drop_in', 3), 'hf', ('f32', 'x3')),
    ('the 5th in-edge lost', S5, lambda c: ('drop_in', 4), 'hf', ('f32', 'x3')),
    ('the 3rd consumer lost', S5, lambda c: ('drop_consumer', 2), 'ghs', ('f32', 'x3')),
    ('the 9th consumer lost', S5, lambda c: ('drop_consumer', 8), 'ghs', ('f32', 'x3')),
    ('the 17th consumer lost', S5, lambda c: ('drop_consumer', 16), 'ghs', ('f32', 'x3')),
    ('the last entry of a heavy segment lost', S5, lambda c: ('drop_seg_last',), 'ghs', ('x3',)),
    ('the second segment lost', S5, lambda c: ('drop_seg', 1), 'ghs', ('x3',)),
    ('a consumer of gate id 9 pulled', S5, lambda c: ('pull_never',), 'ghs', ('f32', 'x3')),
    ('sa = 1 for a fan-in-0 gate', S5, lambda c: ('sa_one',), 'hf', ('f32', 'x3')),
    ('the hf half of u ignored', S5R, lambda c: ('u_hs_only',), 'hf', ('f32', 'x3')),
    ('the last row of a partial tile lost in hf', S5, lambda c: ('row_lost', 'hf', _partial_tile_last_row(c)), 'hf', ('f32', 'x3')),
    ('the last row of a partial tile lost in dWvc', S6N, lambda c: ('row_lost', 'dWvc', _partial_tile_last_row(c, 1)), 'dWvc', ('f32', 'x3')),
    ('the last row of a partial tile lost in dbih', S6N, lambda c: ('row_lost', 'dbih', _partial_tile_last_row(c, 1)), 'dbih', ('f32', 'x3')),
    ('a tile of slot 1 on slot 0\'s weights', S5, lambda c: ('slot_swap', _tile_of_slot(c, 1)), 'hf', ('f32', 'x3')),
    ('bhh_n outside the r product', S5, lambda c: ('bhh_n_outside',), 'hf', ('f32', 'x3')),
    ('z h_prev missing', S5R, lambda c: ('no_z_hprev',), 'hf', ('f32', 'x3')),
    ('g_hprev including the gh path', S5R, lambda c: ('ghprev_gh',), 'g_hprev', ('f32', 'x3')),
    ('one tile\'s share missing from dbvc at 5 tiles', S6N, lambda c: ('tile_lost', 'dbvc', W.plan_of(c).level_tile_ptr[1] + 4), 'dbvc', ('x3',)),
    ('the 257th tile missing from dWvc', WIDE, lambda c: ('tile_lost', 'dWvc', W.WGRAD_GRID), 'dWvc', ('x3',)),
    ('the softmax without the running-max rescale', S5, lambda c: ('no_rescale',), 'hf', ('f32', 'x3')),
    ('hi.lo dropped', COH, lambda c: ('drop_hilo',), 'ghs', ('x3',)),
]


@pytest.mark.parametrize('name,maker,mut,out,mms', DEFECTS, ids=[d[0].replace(' ', '_') for d in DEFECTS])
def test_planted_defect_is_ten_times_outside_the_device_bound(name, maker, mut, out, mms):
    """tau = 8 max(r, floor) per output is what tests/test_hip_sweep_reference.py asserts; the defect's ratio on the output it hits
    must be at least 10 tau in every arithmetic it can occur in (the heavy pre-passes, the slab sums and the deferred weight gradient
    exist in the bf16x3 design only)."""
    for mm in mms:
        c, r64, tau = _bounds(maker, mm)
        bad = W.sweep(c, F32, 'x3' if mm == 'x3' else 'exact', mutate=mut(c))
        ratio = W.ratio(bad[out], r64[out], r64['S'][out])
        over = W.share(bad[out], r64[out], r64['S'][out], tau[out])       # (the fp32 ghs has one bound per row: each row against its own)
        print('DEFECT %-48s %-3s %-8s ratio %.3g  tau %.3g  ratio/tau %.3g' % (name, mm, out, ratio, W.tau_max(tau[out]), over))
        assert over >= 10, (name, mm, ratio, W.tau_max(tau[out]), over)


def test_five_tile_level_is_the_one_the_dbvc_defect_uses():
    c = S6N()
    ltp = W.plan_of(c).level_tile_ptr
    assert ltp[2] - ltp[1] == 5


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_unserved_widths_are_refused_on_the_host_before_anything_divides():
    """W / 4 and H / 4 divide kThreads on the host: the pool entries did so before they looked at W, the sweep backwards behind a level
    loop that never sees H when no level has a tile, so a width in 0 .. 3 was an integer division by zero in the host process (and the
    forward entries returned MGV_OK for any H on such a sweep).  The width is now the first thing every entry looks at: no pointer is
    read and nothing is launched, so this runs without a GPU (the pointers are dummies).  The same on the device, with valid buffers
    that must come back untouched: tests/test_hip_sweep_reference.py."""
    import ctypes
    from deepgate import _hip
    lib, sigs = _hip.load(), _hip.parse_header()
    dummy = ctypes.c_void_p(64)
    served = {'mgv_attn_pool_fwd': (32, 64, 128), 'mgv_attn_pool_bwd': (32, 64, 128), 'mgv_func_sweep_fwd': (16, 32, 64), 'mgv_func_sweep_bwd': (16, 32, 64),
              'mgv_func_sweep_fwd_x3': (32, 64), 'mgv_func_sweep_bwd_x3': (32, 64)}
    for name, ok in served.items():
        for width in (0, 1, 2, 3, 4, 8, 16, 24, 48, 96, 128, 256, -4):
            if width in ok:
                continue
            args = [dummy if t is ctypes.c_void_p else 1 for t in sigs[name]]
            args[0], args[-1] = width, None
            assert getattr(lib, name)(*args) == -2, (name, width)


def test_chain_length_bounds_a_float32_model_of_the_fp32_backwards_accumulation():
    """dbih of `wide` (257 tiles) as the fp32 backward forms it, in float32 on the CPU: each tile's rows added one after another, then
    the tiles' shares added one after another (the worst order the atomics can arrive in is still a chain of that length): the error
    stays inside L 2^-24 of the entry's scale, L = 64 + 257."""
    c = WIDE()
    r64 = W.sweep(c)
    plan = W.plan_of(c)
    dG = r64['aux']['dGi'].to(F32)
    acc = torch.zeros(3 * c['H'], dtype=F32)
    for t in range(plan.num_tiles):
        rows = dG[W.tile_nodes(plan, t)]
        part = torch.zeros(3 * c['H'], dtype=F32)
        for i in range(rows.shape[0]):
            part = part + rows[i]
        acc = acc + part
    L = W.chain_length(c, 'dbih')
    assert L == W.TILE + W.WGRAD_GRID + 1
    r = W.ratio(acc[None], r64['dbih'], r64['S']['dbih'])
    print('float32 chain model of dbih at 257 tiles: %.3g of scale, L 2^-24 = %.3g' % (r, L * U24))
    assert r <= L * U24


def _dot_as_the_kernels(a, b, H):
    """sum_k a_k b_k over 2H columns in float32 the way the level kernels add it up (mgv_common.h): dot4 over a lane's four columns of
    the hs half, dot4 over those of the hf half, their sum, then the butterfly over the row's H / 4 lanes."""
    p = a * b
    assert p.dtype == F32
    lanes = p.reshape(-1, 2, H // 4, 4)
    d4 = ((lanes[..., 0] + lanes[..., 1]) + lanes[..., 2]) + lanes[..., 3]
    v = d4[:, 0] + d4[:, 1]
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


@pytest.mark.parametrize('H,T', [(16, 7), (64, 5)])
def test_derived_ghs_bound_holds_for_a_float32_model_of_the_kernels_attention_backward(H, T):
    """alpha, dsc and the pull of ghs for `shallow` as k_level_bwd forms them, in float32 on the CPU: the scores, t = dzb . x and
    ci = dzb . zbar as dot4 + dot4 and the butterfly add them up, the online softmax in list order with its running-max rescale
    (S and zbar), __expf(a) as exp2(a * log2 e) in float32, inv = 1 / (S + 1e-16), alpha = __expf(sc - m) inv, dsc = alpha (t - ci),
    the pull in list order.  The sources' hf rows and dzb are the float64 run's, rounded: this is alpha's and dsc's own error, the one
    sweep_ref.alpha_error and aux['ghs_own'] bound (a weight below 2^-126 is flushed: the spread rows' e^-120).  The middle source of
    the spread rows (scores 60 below the maximum) is where it is largest, and where 8 x the float32 floor does not hold it."""
    c = _shallow(H, T)
    r64 = W.sweep(c)
    plan = W.plan_of(c)
    gslot, in_ptr, in_src = plan.gslot.long(), plan.in_ptr.long(), plan.in_src.long()
    N = c['N']
    dst = torch.repeat_interleave(torch.arange(N), in_ptr[1:] - in_ptr[:-1])
    live, rho = r64['aux']['live'], r64['aux']['rho']
    dl = dst[live]
    x = torch.cat([c['hs'], r64['hf'].to(F32)], 1)[in_src[live]]
    u = c['attn_u'][gslot[dl]]
    sc = _dot_as_the_kernels(u, x, H)
    expf = lambda a: torch.exp2(a * torch.tensor(1.4426950408889634, dtype=F32))      # noqa: E731
    m, S, zb = torch.full((N,), float('-inf'), dtype=F32), torch.zeros(N, dtype=F32), torch.zeros(N, 2 * H, dtype=F32)
    pos = live - in_ptr[dl]
    for k in range(int(pos.max()) + 1):
        sel = torch.nonzero(pos == k).reshape(-1)
        v = dl[sel]
        mn = torch.maximum(m[v], sc[sel])
        corr, w = expf(m[v] - mn), expf(sc[sel] - mn)
        S[v] = S[v] * corr + w
        zb[v] = w[:, None] * x[sel] + corr[:, None] * zb[v]
        m[v] = mn
    inv = 1.0 / (S + torch.tensor(1e-16, dtype=F32))
    zb = zb * inv[:, None]
    alpha = expf(sc - m[dl]) * inv[dl]
    assert alpha.dtype == F32
    a64 = r64['alpha'][live]
    err = (alpha.to(F64) - a64).abs()
    q = err / (rho * a64 + 2.0 ** -126)
    mid = torch.nonzero(in_src[live] == c['spread_src'][1]).reshape(-1)
    assert mid.numel() == 2 and bool((a64[mid] < 1e-25).all())
    print('float32 model H=%d T=%d: alpha worst err / (rho alpha) %.3g; the spread rows\' middle source: relative error %.3g, rho %.3g'
          % (H, T, float(q.max()), float((err[mid] / a64[mid]).max()), float(rho[mid].max())))
    assert float(q.max()) <= 1
    assert float(rho[mid].min()) > 8 * W.FLOOR['f32']
    dz = r64['dzb'].to(F32)
    ds = alpha * (_dot_as_the_kernels(dz[dl], x, H) - _dot_as_the_kernels(dz, zb, H)[dl])
    ghs = torch.zeros(N, H, dtype=F32)
    term = alpha[:, None] * dz[dl, :H] + ds[:, None] * u[:, :H]
    for e in range(term.shape[0]):                          # (in-CSR order: a float32 sum in SOME list order)
        ghs[in_src[live[e]]] += term[e]
    own = r64['aux']['ghs_own']
    Sg = r64['S']['ghs']
    floor = 8 * W.FLOOR['f32']
    v = c['spread_src'][1]
    r_mid = W.ratio(ghs[v:v + 1], r64['ghs'][v:v + 1], Sg[v:v + 1])
    sh = W.share(ghs, r64['ghs'], Sg, own.clamp(min=floor))
    print('float32 model H=%d T=%d: ghs worst share of max(8 floor, own) %.3g; the middle source\'s row %.3g of scale, own %.3g'
          % (H, T, sh, r_mid, float(own[v])))
    assert sh <= 1
