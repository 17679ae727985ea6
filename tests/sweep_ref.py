"""Plain restatement of the levelised functional sweep (csrc/func_level.hip, func_level_x3.hip: per-gate-type attention aggregation
and a GRU update of hf, level by level) and of the stand-alone attention pooling (csrc/attn_pool.hip) under torch autograd, from
exactly what the C ABI takes (include/mgvae_hip.h), plus the builders of the cases tests/test_hip_sweep_reference.py runs on the
device.  CPU only; pinned to the reference project's fixture and to oracle/ref_cpu.py by tests/test_sweep_spec.py, which also
asserts the builders' properties and shows that the planted defects (`mutate=`) are far outside the device tests' bounds.

sweep(case, dtype, mm):  for levels 1 .. L-1 in order, every node v with gslot[v] = g != 255, sources j in in-CSR order, x_j = [hs_j, hf_j]:
  sc_j = u_g . x_j,  alpha_j = exp(sc_j - max) / (sum exp + 1e-16),  zbar = sum alpha_j x_j,  sa = [deg > 0],
  gi = Wvc_g zbar + sa bvc_g + bih_g,  gh_v = bhh_g (round 1) or gh[v] (rounds >= 2, bhh zero),
  r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n),  hf[v] = (1 - z) n + z h_prev[v]  (h_prev = 0 in round 1).
  Never-updated rows keep 0 (round 1) or h_prev[v] (rounds >= 2) and are constants: no gradient reaches their h_prev / gh rows.
  The tables (gslot, level, in-CSR, tiles) are the product's own: GraphPlan(ei, N).set_levels(gate, level, gate_ids), never hand-built.
  mm = 'x3' (float32 only): the three matrix products (zbar Wvc^T, dG Wvc, dG^T zbar) on bf16 planes (struct_stage_ref.mm3).

Scales S (float64 only), one per entry or row: the sums of the magnitudes of the terms behind an entry
  hf row         max(1, max |row|)                                ghs row      max_col sum_consumers (alpha |dzb| + |dsc| |u|)
  d_attn_u[g]    sum_edges |dsc| |x_j|                            dWvc[g]      |dGi|^T |zbar| over the slot's rows
  dbvc           sum sa |dGi|      dbih  sum |dGi|                dbhh         sum |dGh|
  d_gh row       max |dGh row|                                    g_hprev      |dh| z per entry
Where S = 0 the device must return the reference's value exactly (struct_stage_ref.ratio's rule).
Bounds: taus (8 max(r, floor) per output) and device_taus (with the derived terms: chain_length for the fp32 backward's float atomics,
alpha_error / aux['ghs_own'] / aux['dx_alpha'] for what a float32 softmax weight and dsc are good to, row by row).

attn_pool(case, dtype): zbar, mstat (0 for an empty list), inv (1 / (S + 1e-16)), dx, du of mgv_attn_pool_fwd / _bwd, with scales
  zbar  sum alpha |x_j| per entry    mstat  max_j sum_k |u_k x_jk|    inv  inv (relative)
  dx[j] sum over the edges out of j of alpha |dz_i| + D |u|           du   sum_edges D |x_j|
  with D_e = alpha_e (|dz_i| . |x_e| + sum_k alpha_k |dz_i| . |x_k|), the terms of d(score_e) = alpha_e (t_e - sum_k alpha_k t_k).
"""
import numpy as np
import torch

import struct_stage_ref as SR
from struct_stage_ref import F32, F64, grid_for, mm3, ratio  # noqa: F401  (re-exported: the device tests use them from here)

NO_GATE = 255
TILE = 64                   # csrc/mgv_common.h kTileRows
THREADS = 256               # csrc/mgv_common.h kThreads
IN_REGS, IN_CAP = 3, 4      # csrc/func_level_x3_common.h kInRegs, kInCap
OUT_CHUNK, ROW_OUT, OUT_CAP = 2, 8, 16      # kOutChunk, kRowOut, kOutCap
HEAVY_ROW, HEAVY_SEG = 64, 512              # GraphPlan.HEAVY_ROW / HEAVY_SEG (struct_stage_x3_common.h kHeavyRow)
MAX_SLOTS = 6               # kMaxSlots
WGRAD_GRID = 256            # kWgradGrid
WIDE_LAST = 40              # rows of the 257th tile of `wide`
NEVER = 9                   # a gate id no model updates
FANOUTS = (0, 1, 2, 3, 8, 9, 16, 17, 33, 64, 65, 513, 1100)
FANINS = (0, 1, 2, 3, 4, 5, 7, 40)
GROUPS = (129, 65, 64, 63, 1)               # level-1 group sizes, rotated over the slots by the seed
SPREAD = 60.0               # the spread rows' scores are -SPREAD .. +SPREAD

# workgroups per CU handed to grid_for and the rows a workgroup takes per visit, with the source line restated (as dense_ref.GEOMETRY)
GEOMETRY = {
    'pull_inactive': (8, lambda H: THREADS // (H // 4), 'func_level.hip / func_level_x3.hip: grid_for(ceil(N / rows_per_block), 8), rows_per_block = kThreads / (H / 4)'),
    'attn_pool': (8, lambda W: THREADS // (W // 4), 'attn_pool.hip: grid_for(ceil(N / rows_per_block), 8), rows_per_block = kThreads / (W / 4)'),
}


def cap_rows(kernel, width):
    """The largest row count at which every workgroup visits one row per lane group; from cap_rows + 1 on workgroup 0 comes round
    a second time (mgv_common.h grid_for: min(max(tiles, 1), 256 * per_cu))."""
    per_cu, unit, _ = GEOMETRY[kernel]
    return SR.GRID_CAP * per_cu * unit(width)


# ------------------------------------------------------------------------------------------------ the sweep
def plan_of(c, device=None):
    """The product's own tables for case c (cached per device)."""
    from deepgate.graph_plan import GraphPlan
    key = '_plan_%s' % (device or 'cpu')
    if key not in c:
        ei = torch.from_numpy(c['ei'])
        if device is not None:
            ei = ei.to(device)
        c[key] = GraphPlan(ei, c['N'], device=device).set_levels(torch.from_numpy(c['gate']), torch.from_numpy(c['level']), c['gate_ids'])
    return c[key]


class _Lin3Drop(torch.autograd.Function):
    """_Lin3 with the hi.lo product dropped from every matrix product (hi.hi + lo.hi only): the defect of the coherent case."""
    @staticmethod
    def _mm(a, b):
        ah, al = SR._split(a)
        bh, _ = SR._split(b)
        return ah @ bh + al @ bh

    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return _Lin3Drop._mm(x, W.t())

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        return _Lin3Drop._mm(g, W), _Lin3Drop._mm(g.t(), x)


def _under(S):
    """A float32 term below 2^-126 is flushed (the spread rows' alpha is exp(-120) = 8e-53, finite in float64 only): an absolute error
    of up to 2^-126 per term, which a scale made of such terms alone cannot carry.  Where S > 0 it gains 2^-100 = 2^-126 / 2^-26, so that
    tau S >= 8 * 2^-23 * 2^-100 = 2^-120 covers 64 flushed terms; an entry nothing contributes to keeps S = 0."""
    return torch.where(S > 0, S + 2.0 ** -100, S)


def tile_nodes(plan, t):
    s, n = int(plan.tile_start[t]), int(plan.tile_count[t])
    return plan.order[s:s + n].long().cpu()


def sweep(c, dtype=F64, mm='exact', mutate=None):
    """See the module docstring.  `mutate` = (kind, ...) plants ONE defect:
      ('drop_in', k)         in-edge k (0-based position in its list) of every node is never read
      ('drop_consumer', k)   consumer k of every node's out-list is left out of the node's pull
      ('drop_seg_last',)     the last entry of every segment of a heavy (> 64 consumers) out-list is left out of the pull
      ('drop_seg', s)        segment s of every heavy out-list is left out
      ('pull_never',)        a never-updated consumer is pulled (its alpha / dsc / dzb are nobody's: 1 stands for what lies there)
      ('sa_one',)            sa = 1 for a gate without in-edges            ('u_hs_only',)  the hf half of u ignored
      ('row_lost', out, v)   node v (the last row of a partial tile) missing from out in ('hf', 'dWvc', 'dbih')
      ('slot_swap', t)       tile t runs on slot 0's parameters            ('bhh_n_outside',)  b_hh_n outside the r . product
      ('no_z_hprev',)        z h_prev missing                              ('ghprev_gh',)  g_hprev also carries the r block of d_gh
      ('tile_lost', out, t)  tile t's share missing from out in ('dbvc', 'dWvc')
      ('no_rescale',)        the online softmax without its running-max rescale
      ('drop_hilo',)         x3: the hi.lo product dropped
    Scales come with float64 and no defect only."""
    assert mm == 'exact' or dtype == F32
    plan = plan_of(c)
    H, N, T = c['H'], c['N'], c['T']
    kind = mutate[0] if mutate else None
    gslot, level = plan.gslot.long(), plan.level.long()
    in_ptr, in_src = plan.in_ptr.long(), plan.in_src.long()
    out_ptr, out_slot = plan.out_ptr.long(), plan.out_slot.long()
    E = int(in_src.numel())
    deg, odeg = in_ptr[1:] - in_ptr[:-1], out_ptr[1:] - out_ptr[:-1]
    ar = torch.arange(N)
    dst_of = torch.repeat_interleave(ar, deg)
    pos_in = torch.arange(E) - in_ptr[dst_of]
    pos_out = torch.zeros(E, dtype=torch.long)
    pos_out[out_slot] = torch.arange(E) - out_ptr[torch.repeat_interleave(ar, odeg)]
    keep = torch.ones(E, dtype=torch.bool)
    lost = torch.zeros(E, dtype=torch.bool)                 # edges whose gradient never reaches the source's rows
    heavy_e = odeg[in_src] > HEAVY_ROW
    if kind == 'drop_in':
        keep = pos_in != mutate[1]
    if kind == 'drop_consumer':
        lost = pos_out == mutate[1]
    if kind == 'drop_seg_last':
        lost = heavy_e & ((pos_out % HEAVY_SEG == HEAVY_SEG - 1) | (pos_out == odeg[in_src] - 1))
    if kind == 'drop_seg':
        lost = heavy_e & (pos_out // HEAVY_SEG == mutate[1])
    rounds2 = c.get('h_prev') is not None
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)       # noqa: E731
    hs, u_all, Wvc, bvc, bih, bhh = (leaf(c[k]) for k in ('hs', 'attn_u', 'Wvc', 'bvc', 'bih', 'bhh'))
    h_prev = leaf(c['h_prev']) if rounds2 else None
    gh = leaf(c['gh']) if rounds2 else None
    lin = {'exact': lambda x, W: x @ W.t(), 'x3': SR._Lin3.apply}[mm]
    if kind == 'drop_hilo':
        assert mm == 'x3'
        lin = _Lin3Drop.apply
    geff = gslot.clone()
    if kind == 'slot_swap':
        geff[tile_nodes(plan, mutate[1])] = 0
    hf = h_prev.detach().clone() if rounds2 else torch.zeros(N, H, dtype=dtype)
    kept = []
    for lv in range(1, int(plan.num_levels)):
        nodes = torch.nonzero((level == lv) & (gslot != NO_GATE)).reshape(-1)
        n = int(nodes.numel())
        if n == 0:
            continue
        g = geff[nodes]
        loc = torch.full((N,), -1, dtype=torch.long)
        loc[nodes] = torch.arange(n)
        e = torch.nonzero((loc[dst_of] >= 0) & keep).reshape(-1)
        seg, src = loc[dst_of[e]], in_src[e]
        x = torch.cat([hs[src], hf[src]], 1)
        x = torch.where(lost[e][:, None], x.detach(), x)
        ue = u_all[g][seg]
        sc = (x[:, :H] * ue[:, :H]).sum(1) if kind == 'u_hs_only' else (x * ue).sum(1)
        sc.retain_grad()
        if kind == 'no_rescale':            # w_k = exp(sc_k - running max at k), never corrected when the maximum moves on
            w = torch.zeros_like(sc)
            run = torch.full((n,), float('-inf'), dtype=dtype)
            pe = pos_in[e]
            for k in range(int(pe.max()) + 1 if e.numel() else 0):
                sel = torch.nonzero(pe == k).reshape(-1)
                run = run.index_put((seg[sel],), torch.maximum(run[seg[sel]], sc.detach()[sel]))
                w = w.index_put((sel,), torch.exp(sc[sel] - run[seg[sel]]))
        else:
            m = torch.full((n,), float('-inf'), dtype=dtype).scatter_reduce(0, seg, sc.detach(), 'amax')
            w = torch.exp(sc - m[seg])
        Ssum = torch.zeros(n, dtype=dtype).index_add(0, seg, w)
        alpha = w / (Ssum[seg] + 1e-16)
        zbar = torch.zeros(n, 2 * H, dtype=dtype).index_add(0, seg, alpha[:, None] * x)
        zbar.retain_grad()
        sa = (torch.zeros(n, dtype=dtype).index_add(0, seg, torch.ones(e.numel(), dtype=dtype)) > 0).to(dtype)
        if kind == 'sa_one':
            sa = torch.ones_like(sa)
        gi = torch.zeros(n, 3 * H, dtype=dtype)
        for s_ in torch.unique(g).tolist():
            rows = torch.nonzero(g == s_).reshape(-1)
            gi = gi.index_put((rows,), lin(zbar[rows], Wvc[s_]) + sa[rows, None] * bvc[s_] + bih[s_])
        gi.retain_grad()
        ghv = bhh[g] + (gh[nodes] if rounds2 else 0)
        ghv.retain_grad()
        r = torch.sigmoid(gi[:, :H] + ghv[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + ghv[:, H:2 * H])
        if kind == 'bhh_n_outside':
            bn = bhh[g][:, 2 * H:]
            nn = torch.tanh(gi[:, 2 * H:] + bn + r * (ghv[:, 2 * H:] - bn))
        else:
            nn = torch.tanh(gi[:, 2 * H:] + r * ghv[:, 2 * H:])
        hnew = (1 - z) * nn
        if rounds2 and kind != 'no_z_hprev':
            hnew = hnew + z * h_prev[nodes]
        hnew.retain_grad()
        wr = torch.ones(n, dtype=torch.bool)
        if kind == 'row_lost' and mutate[1] == 'hf':
            wr = nodes != mutate[2]
        hf = hf.index_put((nodes[wr],), hnew[wr])
        kept.append((nodes, e, sc, alpha, zbar, gi, ghv, hnew, sa, z, (x.detach() * ue.detach()).abs().sum(1)))
    hf.backward(c['ghf'].to(dtype))
    Z = lambda *s: torch.zeros(*s, dtype=dtype)       # noqa: E731
    al_e, ds_e, dzb, zb, dGi, dGh, dh, zz, sa_n = Z(max(E, 1)), Z(max(E, 1)), Z(N, 2 * H), Z(N, 2 * H), Z(N, 3 * H), Z(N, 3 * H), Z(N, H), Z(N, H), Z(N)
    sc_e, A_e = Z(max(E, 1)), Z(max(E, 1))
    for nodes, e, sc, alpha, zbar, gi, ghv, hnew, sa, z, A in kept:
        sc_e[e], A_e[e] = sc.detach(), A
        al_e[e], ds_e[e] = alpha.detach(), sc.grad
        dzb[nodes], zb[nodes], dGi[nodes], dGh[nodes], dh[nodes], zz[nodes], sa_n[nodes] = zbar.grad, zbar.detach(), gi.grad, ghv.grad, hnew.grad, z.detach(), sa
    res = {'hf': hf.detach(), 'ghs': hs.grad if hs.grad is not None else Z(N, H), 'd_attn_u': u_all.grad, 'dWvc': Wvc.grad, 'dbvc': bvc.grad, 'dbih': bih.grad,
           'dbhh': bhh.grad, 'alpha': al_e, 'dsc': ds_e, 'dzb': dzb}
    for k in ('d_attn_u', 'dWvc', 'dbvc', 'dbih', 'dbhh'):
        if res[k] is None:
            res[k] = torch.zeros_like(c[{'d_attn_u': 'attn_u', 'dWvc': 'Wvc', 'dbvc': 'bvc', 'dbih': 'bih', 'dbhh': 'bhh'}[k]], dtype=dtype)
        res[k] = res[k].clone()
    if rounds2:
        res['d_gh'] = gh.grad if gh.grad is not None else Z(N, 3 * H)
        res['g_hprev'] = h_prev.grad if h_prev.grad is not None else Z(N, H)
        del res['dbhh']                     # "receives nothing meaningful" in rounds >= 2 (include/mgvae_hip.h)
        if kind == 'ghprev_gh':
            res['g_hprev'] = res['g_hprev'] + dGh[:, :H]
    if kind == 'pull_never':
        bad = torch.nonzero((gslot[dst_of] == NO_GATE) & (level[dst_of] >= 1)).reshape(-1)
        res['ghs'] = res['ghs'].index_add(0, in_src[bad], torch.ones(bad.numel(), H, dtype=dtype))
    if kind == 'row_lost' and mutate[1] in ('dWvc', 'dbih'):
        v = mutate[2]
        if mutate[1] == 'dWvc':
            res['dWvc'][gslot[v]] -= torch.outer(dGi[v], zb[v])
        else:
            res['dbih'][gslot[v]] -= dGi[v]
    if kind == 'tile_lost':
        tn = tile_nodes(plan, mutate[2])
        gt = int(gslot[tn[0]])
        if mutate[1] == 'dWvc':
            res['dWvc'][gt] -= dGi[tn].t() @ zb[tn]
        else:
            res['dbvc'][gt] -= (sa_n[tn, None] * dGi[tn]).sum(0)
    res = {k: v.detach().to(F64) for k, v in res.items()}
    if dtype == F64 and mutate is None:
        aG, aH, azb, au = dGi.abs(), dGh.abs(), zb.abs(), u_all.detach().abs()
        upd = gslot != NO_GATE
        S = {'hf': res['hf'].abs().amax(1).clamp(min=1.0)}
        live = torch.nonzero(upd[dst_of]).reshape(-1) if E else torch.zeros(0, dtype=torch.long)
        gd = gslot[dst_of[live]]
        term = al_e[live, None] * dzb[dst_of[live], :H].abs() + ds_e[live, None].abs() * au[gd][:, :H]
        S['ghs'] = _under(Z(N, H).index_add(0, in_src[live], term).amax(1))
        xe = torch.cat([hs.detach()[in_src[live]], res['hf'][in_src[live]]], 1).abs()
        S['d_attn_u'] = _under(Z(T, 2 * H).index_add(0, gd, ds_e[live, None].abs() * xe))
        S['dWvc'], S['dbvc'], S['dbih'], S['dbhh'] = Z(T, 3 * H, 2 * H), Z(T, 3 * H), Z(T, 3 * H), Z(T, 3 * H)
        for s_ in range(T):
            rows = torch.nonzero(gslot == s_).reshape(-1)
            S['dWvc'][s_] = aG[rows].t() @ azb[rows]
            S['dbvc'][s_], S['dbih'][s_], S['dbhh'][s_] = (sa_n[rows, None] * aG[rows]).sum(0), aG[rows].sum(0), aH[rows].sum(0)
        if rounds2:
            del S['dbhh']
            S['d_gh'], S['g_hprev'] = aH.amax(1), dh.abs() * zz
        res['S'] = S
        res['aux'] = {'dGi': dGi, 'dh': dh, 'zbar': zb, 'sa': sa_n}
        # The float32 error of alpha and dsc themselves pushed through the terms of ghs, as a share of the row's scale.  alpha_e: rho_e
        # (alpha_error).  dsc_e = alpha_e (t_e - ci), t_e = dzb . x_e, ci = dzb . zbar: the scale has |dsc|, but t_e - ci is a
        # difference of two sums of 2H products, each good to depth 2^-24 of ITS terms' magnitudes T_e = sum_k |dzb_k x_ek| and
        # sum_k |dzb_k zbar_k| <= Q = sum_j alpha_j T_j, and zbar carries the weights' errors, sum_j rho_j alpha_j T_j, and the deg
        # additions behind an entry of it.
        depth = SCORE_DEPTH['sweep'](H)
        dl = dst_of[live]
        al, adz = al_e[live], dzb.abs()
        rho = alpha_error(depth, sc_e[live], A_e[live], al, dl, N)
        Te = (adz[dl] * xe).sum(1)
        Q, R = Z(N).index_add(0, dl, al * Te), Z(N).index_add(0, dl, rho * al * Te)
        e_dsc = al * (depth * U24 * (Te + Q[dl]) + R[dl] + (deg[dl] + 2) * U24 * Q[dl]) + (rho + 2 * U24) * ds_e[live].abs()
        d = Z(N, H).index_add(0, in_src[live], (rho * al)[:, None] * adz[dl, :H] + e_dsc[:, None] * au[gd][:, :H]).amax(1)
        res['aux']['ghs_own'] = torch.where(S['ghs'] > 0, d / S['ghs'].clamp(min=1e-300), Z(N))
        res['aux']['live'], res['aux']['rho'] = live, rho
    return res


# additions and roundings behind one term of a score as the kernels form it (mgv_common.h dot4 and group_sum): the product, the three
# additions of dot4, in the sweep the addition of the hs and the hf half, then one addition per butterfly step over the H / 4 lanes
SCORE_DEPTH = {'sweep': lambda H: 5 + (H // 4).bit_length() - 1, 'pool': lambda W: 4 + (W // 4).bit_length() - 1}


def alpha_error(depth, sc, A, alpha, seg, n):
    """First-order bound on the relative error of a float32 softmax weight alpha_e = exp(sc_e - m) / (sum_k exp(sc_k - m) + 1e-16) as
    the level and pool kernels form it; per edge, from float64 quantities only (sc the scores, A_e = sum_k |u_k x_ek|, seg the
    edge's destination among n).  alpha does not change when every score of a list moves by the same amount, so the error of the
    maximum cancels and what is left is each score's own:
      own_e = depth 2^-24 A_e        the score: a sum in which every term passes `depth` roundings (SCORE_DEPTH)
            + 3 2^-24 |sc_e - m|     exp of it: __expf(a) is exp2(a log2 e) on v_exp_f32; the subtraction, the rounded constant and the
                                     rounded product each move the argument by 2^-24 |a|, i.e. the result by that much of itself
            + 2^-23                  v_exp_f32 itself: 1 ulp
      rho_e = own_e + sum_k alpha_k own_k + (deg + 3) 2^-24      the normalisation: the sum of deg weights, + 1e-16, 1 / S, alpha = w inv
    exp turns an ABSOLUTE error of its argument into a relative one of its value: a list whose scores spread by 60 with terms of one
    sign (the spread rows) has weights e^-60 that are good to 60 * 10 * 2^-24 = 4e-5 only, in any float32 implementation; which way the
    roundings fall there differs between one correct implementation and the next, so no single float32 run bounds another."""
    m = torch.full((n,), float('-inf'), dtype=F64).scatter_reduce(0, seg, sc, 'amax')
    deg = torch.zeros(n, dtype=F64).index_add(0, seg, torch.ones_like(sc))
    own = (depth * A + 3 * (m[seg] - sc) + 2) * U24
    return own + torch.zeros(n, dtype=F64).index_add(0, seg, alpha * own)[seg] + (deg[seg] + 3) * U24


OUTPUTS = ('hf', 'ghs', 'd_attn_u', 'dWvc', 'dbvc', 'dbih', 'dbhh', 'd_gh', 'g_hprev')
ACCS = ('d_attn_u', 'dWvc', 'dbvc', 'dbih', 'dbhh')


def ratios(got, ref):
    return {k: ratio(got[k], ref[k], S) for k, S in ref['S'].items() if k in got}


def taus(r64, rk, mm):
    """tau = 8 max(r, floor) per output, r the worst ratio of the CPU restatement in the kernel's arithmetic against float64."""
    return {k: 8 * max(v, FLOOR[mm]) for k, v in ratios(rk, r64).items()}


FLOOR = {'f32': 2.0 ** -23, 'x3': 2.0 ** -17}          # as struct_stage / dense_ref state them
U24 = 2.0 ** -24


def chain_length(c, output):
    """L: the longest chain of sequential float32 additions the FP32 backward's design makes for one entry of an accumulator (every
    addition counted as sequential, as dense_ref.chain_length does).  k_level_bwd is one workgroup per tile: an entry of dWvc / dbvc /
    dbih / dbhh takes the tile's 64 rows (MFMA accumulation, per-lane sums, shuffles, LDS atomics: at most one addition per row) and
    is then added to the accumulator with ONE float atomic per tile, in arrival order: L = 64 + (tiles of the slot with the most
    tiles).  An entry of d_attn_u takes every in-edge of the tile (per lane group in list order, LDS atomics across groups) before
    that atomic: L = (most in-edges of one tile) + tiles.  Stated because a correct kernel was measured outside tau there on an
    MI355X (NOTEBOOK.md, 2026-10-18): 3.2e-6 of scale at 257 tiles against tau = 9.5e-7; 321 * 2^-24 = 1.9e-5."""
    plan = plan_of(c)
    stp = plan.slot_tile_ptr
    tiles = max([stp[i + 1] - stp[i] for i in range(len(stp) - 1)] + [0])
    if output == 'd_attn_u':
        deg = (plan.in_ptr[1:] - plan.in_ptr[:-1]).long()
        edges = max([int(deg[tile_nodes(plan, t)].sum()) for t in range(plan.num_tiles)] + [0])
        return edges + tiles
    if output in ('dWvc', 'dbvc', 'dbih', 'dbhh'):
        return TILE + tiles
    raise KeyError(output)


def device_taus(c, r64, rk, mm):
    """The bound the device tests use: tau, or max(tau, L 2^-24) for the fp32 backward's accumulators (chain_length); for the fp32
    backward's ghs one bound per row, max(tau, the float32 error of alpha and dsc themselves pushed through the row's terms) (sweep:
    aux['ghs_own'], alpha_error).  The row of the spread rows' middle source is two weights e^-60 times dzb and dsc and nothing else:
    a correct kernel was measured at 1.8e-5 of its scale there on an MI355X (alpha off by 5.6e-6 of itself, dsc by 4e-5), and the
    float32 restatement gives 7.5e-7 or 2.4e-6 on that row depending on the machine it runs on, so it bounds nothing there
    (NOTEBOOK.md, 2026-10-18).  The bf16x3 bound is 8 * 2^-17 = 6.1e-5 at the least and stays as it is.
    A value is a float, or a tensor of the shape of the output's scale; `share` takes both."""
    t = taus(r64, rk, mm)
    if mm == 'f32':
        for k in ACCS:
            if k in t:
                t[k] = max(t[k], chain_length(c, k) * U24)
        t['ghs'] = r64['aux']['ghs_own'].clamp(min=t['ghs'])
    return t


def share(got, ref, S, tau):
    """max |got - ref| / (tau S): at most 1 inside the bound; tau a float or one value per entry of S."""
    return ratio(got, ref, S * tau)


def tau_max(tau):
    return float(tau.max()) if torch.is_tensor(tau) else tau


# ------------------------------------------------------------------------------------------------ cases
def _params(g, H, T, c):
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    c.update(attn_u=0.25 * f(T, 2 * H), Wvc=0.15 * f(T, 3 * H, 2 * H), bvc=0.1 * f(T, 3 * H), bih=0.1 * f(T, 3 * H), bhh=0.1 * f(T, 3 * H))
    return f


def _finish(c, g, f, rounds2):
    N, H = c['N'], c['H']
    c['hs'] = f(N, H) if 'hs' not in c else c['hs']
    c['ghf'] = f(N, H)
    c['h_prev'] = c['gh'] = None
    if rounds2:                              # rounds >= 2: random previous states (the inputs' rows too) and hidden halves; b_hh rides in gh
        c['h_prev'], c['gh'] = 0.7 * f(N, H), 0.5 * f(N, 3 * H)
        c['bhh'] = torch.zeros_like(c['bhh'])
    return c


def shallow(H, T, seed=0, rounds2=False, fanout=True):
    """A 3-level graph (inputs, level 1, level 2): a level's error does not compound.  Slot s is gate id s + 1, id 0 an input, id 9
    a type nobody updates.  With T >= 2 the last slot is absent from the whole graph, with T >= 3 slot T - 2 is absent from level 1.
    Level 1: per present slot one group of GROUPS[(slot + seed) % 5] nodes whose fan-ins cycle through FANINS from a pool of 48
    quiet inputs, and on slot 0 the designed rows: two spread rows (scores +SPREAD, 0, -SPREAD, largest first and largest last), a
    row of three equal scores (the same input three times: a repeated edge), a row [a, a, b], then one gate per FANOUTS entry and
    three gates of id 9.  Level 2 (fanout=True): a pool of 1100 consumers, every eleventh of id 9; one input and one level-1 gate
    per FANOUTS entry f feed f distinct pool nodes (1, 2 and 3 heavy segments: 65, 513 and 1100 consumers), the id-9 gates of
    level 1 feed the first pool nodes.  fanout=False: 30 level-2 consumers fed by the level-1 gates, no long out-list: the widest
    level then has 1, 3, 4, 5, ... tiles (the small-gradient slab sum's unroll of four and its tail) depending on (T, seed)."""
    g = np.random.Generator(np.random.PCG64([seed, H, T, int(rounds2), int(fanout)]))
    c = {'H': H, 'T': T, 'gate_ids': list(range(1, T + 1)), 'name': 'shallow T=%d seed=%d%s%s' % (T, seed, ' r2' if rounds2 else '', '' if fanout else ' nofan')}
    present = list(range(T - 1)) if T >= 2 else [0]
    lvl1 = present[:-1] if T >= 3 else present
    gate, level, src, dst = [], [], [], []

    def add(gid, lv, k=1):
        first = len(gate)
        gate.extend([gid] * k)
        level.extend([lv] * k)
        return list(range(first, first + k))

    pool = add(0, 0, 48)
    sp_hi, sp_mid, sp_lo = add(0, 0)[0], add(0, 0)[0], add(0, 0)[0]
    pi_f = add(0, 0, len(FANOUTS))
    groups = {}
    for s_ in lvl1:
        groups[s_] = add(s_ + 1, 1, GROUPS[(s_ + seed) % len(GROUPS)])
        for i, v in enumerate(groups[s_]):
            k = FANINS[(i + s_) % len(FANINS)]
            for j in g.choice(len(pool), size=k, replace=k > len(pool)):
                src.append(pool[j]); dst.append(v)
    rows = add(1, 1, 4)
    for j in (sp_hi, sp_mid, sp_lo):
        src.append(j); dst.append(rows[0])
    for j in (sp_lo, sp_mid, sp_hi):
        src.append(j); dst.append(rows[1])
    for j in (pool[3], pool[3], pool[3]):
        src.append(j); dst.append(rows[2])
    for j in (pool[5], pool[5], pool[7]):
        src.append(j); dst.append(rows[3])
    l1_f = add(1, 1, len(FANOUTS))
    for v in l1_f:
        for j in g.choice(len(pool), size=2, replace=False):
            src.append(pool[j]); dst.append(v)
    nev1 = add(NEVER, 1, 3)
    for v in nev1:
        src.append(pool[0]); dst.append(v)
    l2slots = present
    if fanout:
        M = 1100
        cons = []
        for i in range(M):
            cons += add(NEVER if i % 11 == 10 else l2slots[i % len(l2slots)] + 1, 2)
        for kind_nodes, off in ((pi_f, 0), (l1_f, 370)):
            for q, f_ in enumerate(FANOUTS):
                for i in range(f_):
                    src.append(kind_nodes[q]); dst.append(cons[(off + 97 * q + i) % M])
        for q, v in enumerate(nev1):
            for i in range(4):
                src.append(v); dst.append(cons[(5 * q + i) % M])
    else:
        cons = []
        for i in range(30):
            cons += add(NEVER if i % 11 == 10 else l2slots[i % len(l2slots)] + 1, 2)
        feeders = l1_f + nev1 + [v for s_ in lvl1 for v in groups[s_][:9]]
        for i, v in enumerate(cons):
            for j in g.choice(len(feeders), size=1 + (i // len(l2slots)) % 4, replace=False):      # (every slot gets every fan-in 1 .. 4)
                src.append(feeders[j]); dst.append(v)
    N = len(gate)
    c.update(N=N, ei=np.array([src, dst], dtype=np.int64), gate=np.array(gate, dtype=np.int64), level=np.array(level, dtype=np.int64))
    f = _params(g, H, T, c)
    hs = f(N, H)
    u0 = c['attn_u'][0, :H]
    for j, s_ in ((sp_hi, SPREAD), (sp_mid, 0.0), (sp_lo, -SPREAD)):
        hs[j] = s_ * u0 / float(u0 @ u0)
    c['hs'] = hs
    c.update(spread_rows=rows[:2], equal_row=rows[2], repeat_row=rows[3], spread_src=(sp_hi, sp_mid, sp_lo), pi_f=pi_f, l1_f=l1_f, nev1=nev1, cons=cons,
             groups=groups, lvl1_slots=lvl1, present=present)
    _finish(c, g, f, rounds2)
    if rounds2:
        for j in (sp_hi, sp_mid, sp_lo):
            c['h_prev'][j] = 0                # (their scores stay exactly +-SPREAD and 0)
    return c


def deep(H, rounds2=False, T=3):
    """40 levels of 5 to 70 nodes on three slots, fan-in 1 to 3 from any lower level: errors compound along the levels."""
    g = np.random.Generator(np.random.PCG64([11, H, int(rounds2)]))
    c = {'H': H, 'T': T, 'gate_ids': list(range(1, T + 1)), 'name': 'deep%s' % (' r2' if rounds2 else '')}
    gate, level, src, dst = [0] * 24, [0] * 24, [], []
    for lv in range(1, 40):
        k = int(g.integers(5, 71))
        first = len(gate)
        prev = [i for i in range(first) if level[i] == lv - 1]
        for i in range(k):
            v = first + i
            gate.append(int(g.integers(1, T + 1)) if i % 13 != 12 else NEVER)
            level.append(lv)
            src.append(prev[int(g.integers(0, len(prev)))]); dst.append(v)      # one source on the level below: the level is ASAP
            for j in g.integers(0, first, size=int(g.integers(0, 3))):
                src.append(int(j)); dst.append(v)
    N = len(gate)
    c.update(N=N, ei=np.array([src, dst], dtype=np.int64), gate=np.array(gate, dtype=np.int64), level=np.array(level, dtype=np.int64))
    return _finish(c, g, _params(g, H, T, c), rounds2)


def wide(H):
    """One slot with 257 tiles in level 1 (256 full ones and a tile of WIDE_LAST rows: the weight-gradient kernel's 256 workgroups take a
    second tile from workgroup 0 on) fed by never-updated inputs, and N = cap_rows('pull_inactive', H) + 1: workgroup 0 of the
    inactive pull comes round a second time (GEOMETRY)."""
    g = np.random.Generator(np.random.PCG64([12, H]))
    T = 1
    c = {'H': H, 'T': T, 'gate_ids': [1], 'name': 'wide'}
    n_act = TILE * WGRAD_GRID + WIDE_LAST
    N = cap_rows('pull_inactive', H) + 1
    assert N > n_act + 64
    n_in = N - n_act
    gate = np.zeros(N, dtype=np.int64)
    level = np.zeros(N, dtype=np.int64)
    gate[n_in:], level[n_in:] = 1, 1
    dst = np.repeat(np.arange(n_in, N), 2)
    src = g.integers(0, n_in, size=dst.size)
    src[-2:] = n_in - 1, 0                   # the last input row and the first are read
    c.update(N=N, ei=np.stack([src, dst]).astype(np.int64), gate=gate, level=level)
    return _finish(c, g, _params(g, H, T, c), False)


def coherent(H):
    """hs >= 0 (so hf >= 0) and every weight (1 + 2^-9) 2^j: a bf16 split puts 2^j into hi and 2^(j-9) into lo, every hi.lo
    product has the same sign, and dropping that product moves an entry by 2^-9 of its magnitude."""
    g = np.random.Generator(np.random.PCG64([13, H]))
    T = 2
    c = {'H': H, 'T': T, 'gate_ids': [1, 2], 'name': 'coherent'}
    gate = [0] * 16 + [1 + i % 2 for i in range(70)] + [1 + i % 2 for i in range(40)]
    level = [0] * 16 + [1] * 70 + [2] * 40
    src, dst = [], []
    for v in range(16, 86):
        for j in g.choice(16, size=1 + v % 3, replace=False):
            src.append(int(j)); dst.append(v)
    for v in range(86, 126):
        for j in g.choice(70, size=1 + v % 3, replace=False):
            src.append(16 + int(j)); dst.append(v)
    N = len(gate)
    c.update(N=N, ei=np.array([src, dst], dtype=np.int64), gate=np.array(gate, dtype=np.int64), level=np.array(level, dtype=np.int64))
    f = _params(g, H, T, c)
    pw = lambda *s: torch.from_numpy(((1 + 2.0 ** -9) * 2.0 ** g.integers(-8, -5, size=s)).astype(np.float32))      # noqa: E731
    c.update(attn_u=pw(T, 2 * H), Wvc=pw(T, 3 * H, 2 * H), bvc=pw(T, 3 * H), bih=pw(T, 3 * H), bhh=pw(T, 3 * H), hs=f(N, H).abs())
    c['Wvc'][:, H:2 * H] *= 2.0 ** -6          # a quiet z block: its gate gradients are the ones of the other sign (daz = -dh n z (1 - z) <= 0)
    _finish(c, g, f, False)
    c['ghf'] = c['ghf'].abs()                   # dh >= 0: the r and n blocks of dG are >= 0, so dG Wvc is a same-sign sum as well
    return c


# ------------------------------------------------------------------------------------------------ attention pooling
POOL_LISTS = (0, 1, 2, 3, 64, 65, 3000)


def pool_case(W, N, seed=0):
    """Rows x [R, W] (R = max(N, 70) source rows), lists by destination: node i < 14 has POOL_LISTS[i % 7] entries (node 0 none), the
    others 0 to 3; where there are ten or more nodes, node 7 reads the same source three times and nodes 8 / 9 are the spread rows
    (scores +SPREAD, 0, -SPREAD in both orders)."""
    g = np.random.Generator(np.random.PCG64([21, W, N, seed]))
    R = max(N, 70)
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    x, u = f(R, W), 0.25 * f(W)
    deg = g.integers(0, 4, size=N)
    k = min(N, 14)
    deg[:k] = [POOL_LISTS[i % len(POOL_LISTS)] for i in range(k)]
    if N >= 10:
        deg[7:10] = 3
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=ptr[1:])
    E = int(ptr[-1])
    idx = g.integers(3, R, size=max(E, 1)).astype(np.int32)
    if N >= 10:
        for j, s_ in ((0, SPREAD), (1, 0.0), (2, -SPREAD)):
            x[j] = s_ * u / float(u @ u)
        idx[ptr[7]:ptr[8]] = 5
        idx[ptr[8]:ptr[9]] = [0, 1, 2]
        idx[ptr[9]:ptr[10]] = [2, 1, 0]
    return {'W': W, 'N': N, 'R': R, 'E': E, 'x': x, 'u': u, 'dz': f(N, W), 'ptr': torch.from_numpy(ptr.astype(np.int32)), 'idx': torch.from_numpy(idx)}


def attn_pool(c, dtype=F64):
    N, W, E = c['N'], c['W'], c['E']
    ptr = c['ptr'].long()
    deg = ptr[1:] - ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(N), deg)
    src = c['idx'][:E].long()
    x = c['x'].to(dtype).clone().requires_grad_(True)
    u = c['u'].to(dtype).clone().requires_grad_(True)
    xe = x[src]
    sc = xe @ u
    sc.retain_grad()
    m = torch.full((N,), float('-inf'), dtype=dtype).scatter_reduce(0, seg, sc.detach(), 'amax')
    w = torch.exp(sc - m[seg])
    Ssum = torch.zeros(N, dtype=dtype).index_add(0, seg, w)
    alpha = w / (Ssum[seg] + 1e-16)
    zbar = torch.zeros(N, W, dtype=dtype).index_add(0, seg, alpha[:, None] * xe)
    zbar.backward(c['dz'].to(dtype))
    Z = lambda *s: torch.zeros(*s, dtype=dtype)       # noqa: E731
    res = {'zbar': zbar, 'mstat': torch.where(deg > 0, m, torch.zeros_like(m)), 'inv': 1.0 / (Ssum + 1e-16),
           'dx': x.grad if x.grad is not None else Z(*x.shape), 'du': u.grad if u.grad is not None else Z(W)}
    res = {k: v.detach().to(F64) for k, v in res.items()}
    if dtype == F64:
        a = alpha.detach()
        ax, au, adz = xe.detach().abs(), u.detach().abs(), c['dz'].to(dtype).abs()
        # d(score_e) = alpha_e (t_e - sum_k alpha_k t_k), t = dz . x, is itself a difference: its magnitude is taken from ITS terms
        t_abs = (adz[seg] * ax).sum(1)
        dsc = a * (t_abs + Z(N).index_add(0, seg, a * t_abs)[seg])
        tdx = a[:, None] * adz[seg] + dsc[:, None] * au
        res['S'] = {'zbar': _under(Z(N, W).index_add(0, seg, a[:, None] * ax)),
                    'mstat': Z(N).scatter_reduce(0, seg, ax @ au, 'amax'), 'inv': res['inv'].clone(),
                    'dx': _under(Z(*x.shape).index_add(0, src, tdx)), 'du': _under((dsc[:, None] * ax).sum(0))}
        # alpha's own float32 error pushed through the terms of dx, as a share of the entry's scale (the spread rows' middle source)
        rho = alpha_error(SCORE_DEPTH['pool'](W), sc.detach(), ax @ au, a, seg, N)
        Sdx = res['S']['dx']
        res['aux'] = {'dx_alpha': torch.where(Sdx > 0, Z(*x.shape).index_add(0, src, rho[:, None] * tdx) / Sdx.clamp(min=1e-300), Z(*x.shape))}
    return res
