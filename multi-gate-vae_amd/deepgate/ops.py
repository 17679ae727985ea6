"""Host-side operators of the DG_AE hot path: thin checked wrappers over the C ABI
(include/mgvae_hip.h) and the torch.autograd.Functions that stitch the hand-written forward and
backward kernels into the reference's Python operator surface.  PyTorch supplies device memory,
streams and the autograd tape; all arithmetic on [N,*] data happens in libmgvae_hip.so.
"""
from collections import namedtuple
import math
import os

import torch

from . import _hip
from ._hip import F32, I32, U8, HipLibraryError, check, edge_rows, ptr

LN_EPS = 1e-5

# Arithmetic of the dense products: 'x3' = bf16x3 split-precision MFMA (hi/lo bf16 planes, three
# products, fp32 accumulation; ~1e-5 relative per product, 3/16 of the fp32-MFMA cost), 'f32' = exact
# fp32 MFMA.  Hidden widths the x3 kernels do not cover (H=16) always run in fp32.
PRECISION = os.environ.get('MGV_PRECISION', 'x3')
# first half round of an encoder from one kernel row per (degree, class) pair ('table') or over all nodes ('full')
FIRST_STAGE_TABLE = True          # first half round per (degree, class) pair / quotient stages (tests switch it off to compare with the per-node launch)


def use_x3(H):
    return PRECISION == 'x3' and H in (32, 64)          # csrc/mgv_launch.h X3Widths


def split_bf16(w):
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def frag_order(w):
    """[R, K] (k contiguous) -> MFMA 16x16x32 fragment order: blocks (row tile, k-step) of 512 elements in
    which lane l = 16*q + r holds w[16*rt + r, 32*ks + 8*q : +8] at offset 8*l (one coalesced 1 KiB load)."""
    R, K = w.shape
    return w.reshape(R // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def _pack_into(out, off, W, transpose):
    """bf16 hi/lo fragment-order planes of W (or W^T) at out[off : off + 2 * W.numel()] (one launch)."""
    R, K = (W.shape[1], W.shape[0]) if transpose else W.shape
    n = W.numel()
    if W.dtype != F32 or not W.is_cuda or W.stride(1) != 1:
        raise HipLibraryError('weight must be an fp32 GPU matrix with contiguous rows')
    base = out.data_ptr() + 2 * off
    _hip.call('mgv_wpack_bf16x3', ptr(W), R, K, W.stride(0), int(transpose), _hip.ctypes.c_void_p(base),
              _hip.ctypes.c_void_p(base + 2 * n))
    return off + 2 * n


def stage_wpack(Wc, Whh):
    """bf16 weight pack of mgv_struct_stage_*_x3: [Wc_hi, Wc_lo, Whh_hi, Whh_lo, WcT_hi, WcT_lo, WhhT_hi, WhhT_lo],
    each block in fragment order."""
    out = torch.empty(4 * (Wc.numel() + Whh.numel()), dtype=torch.bfloat16, device=Wc.device)
    off = 0
    for w, tr in ((Wc, False), (Whh, False), (Wc, True), (Whh, True)):
        off = _pack_into(out, off, w, tr)
    return out


def sweep_wpack(Wvc):
    """bf16 weight pack of mgv_func_sweep_*_x3 from Wvc [T, 3H, 2H]: per slot [Wvc_hi, Wvc_lo, WvcT_hi, WvcT_lo],
    each block in fragment order."""
    out = torch.empty(4 * Wvc.numel(), dtype=torch.bfloat16, device=Wvc.device)
    off = 0
    for g in range(Wvc.shape[0]):
        off = _pack_into(out, off, Wvc[g], False)
        off = _pack_into(out, off, Wvc[g], True)
    return out


def linear_wpack(W):
    out = torch.empty(2 * W.numel(), dtype=torch.bfloat16, device=W.device)
    _pack_into(out, 0, W, False)
    return out


def _zeros_like_params(*ts):
    return [torch.zeros_like(t) for t in ts]


# ------------------------------------------------------------------------------------------------
# structural encoder half round (digae_layer.py:267-275)
# ------------------------------------------------------------------------------------------------
def _heavy_args(heavy, H, device):
    """(heavy_n, heavy_nodes, heavy_ws) of a stage launch; `heavy` = GraphPlan.heavy(reverse) or None."""
    if heavy is None or heavy[0] == 0:
        return 0, None, None
    n, nodes = heavy
    return n, ptr(nodes), ptr(workspace(2 * n * H, device, tag='heavy'))     # (its own buffer: the bwd2 slab is live in the same launch)


def struct_stage_fwd(h_in, nbr_ptr, nbr_idx, xcls, xtab, Wc, bc, Whh, bhh, ln_w, ln_b, out=None, wpack=None, heavy=None, table_own=None, n_rows=None,
                     stats_out=None, tagged=True):
    """`table_own` (int32 [N]): table mode — h_in is the (degree, class) table, nbr_idx entries are tagged (GraphPlan.tagged_idx);
    with `tagged=False` the entries are plain rows of h_in and only the own rows go through table_own (quotient stages: h_in is the
    previous stage's colour table).
    `n_rows`: only the first n_rows rows of h_in are stage rows, the rest are rows their neighbour lists point at (quotient stages).
    `stats_out` [N, 2] (bf16x3 kernels): receives {mean, rstd} of every row's pre-LayerNorm state, for struct_stage_bwd(stats=...)."""
    N, H = h_in.shape
    if n_rows is not None:
        N = int(n_rows)
    if table_own is not None:
        N = table_own.numel()
    check(h_in, F32, 'h_in'); check(nbr_ptr, I32, 'nbr_ptr'); check(nbr_idx, I32, 'nbr_idx'); check(xcls, U8, 'xcls')
    for n, t in (('xtab', xtab), ('Wc', Wc), ('bc', bc), ('Whh', Whh), ('bhh', bhh)):
        check(t, F32, n)
    check(ln_w, F32, 'ln_w'); check(ln_b, F32, 'ln_b')
    assert nbr_ptr.numel() == N + 1 and xcls.numel() == N
    assert Wc.shape == (3 * H, H) and Whh.shape == (3 * H, H) and xtab.shape[1] == 3 * H
    h_out = (torch.empty(N, H, dtype=F32, device=h_in.device) if out is None else out)
    if use_x3(H):
        wpack = stage_wpack(Wc, Whh) if wpack is None else wpack
        _hip.call('mgv_struct_stage_fwd_x3', H, N, ptr(h_in), ptr(nbr_ptr), ptr(nbr_idx), ptr(xcls), ptr(xtab),
                  xtab.shape[0], ptr(wpack), ptr(bc), ptr(bhh), ptr(ln_w), ptr(ln_b), LN_EPS, ptr(h_out), *_heavy_args(heavy, H, h_in.device), ptr(table_own),
                  int(bool(tagged)), ptr(stats_out))
        return h_out
    assert table_own is None, 'table mode needs the bf16x3 kernels'
    _hip.call('mgv_struct_stage_fwd', H, N, ptr(h_in), ptr(nbr_ptr), ptr(nbr_idx), ptr(xcls), ptr(xtab),
              xtab.shape[0], ptr(Wc), ptr(bc), ptr(Whh), ptr(bhh), ptr(ln_w), ptr(ln_b), LN_EPS, ptr(h_out))
    return h_out


# The bf16x3 half-round backward at H = 64 is struct_stage_bwd2_x3.hip (register-resident recompute weights, transposed products,
# slab-reduced deterministic parameter gradients); the first kernel (struct_stage_x3.hip, mgv_struct_stage_bwd_x3) serves H = 32 only
# and refuses H = 64 with MGV_EUNSUPPORTED.
QUOTIENT = os.environ.get('MGV_QUOTIENT', '1') != '0'         # early half rounds on one row per colour (GraphPlan.quotient)
_WS = {}


def workspace(nfloats, device, dtype=F32, tag=None):
    """Scratch for the deterministic cross-workgroup sums (per-workgroup partial rows, csrc/mgv_slab.h): one growing buffer
    per (device, stream, dtype, tag); launches on a stream are ordered, so consecutive users may share it.  Scratch that one
    launch uses next to the untagged buffer (heavy-row sums) asks for a buffer of its own by `tag`."""
    key = (str(device), _hip.stream().value if torch.device(device).type == 'cuda' else 0, dtype, tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = _WS[key] = torch.empty(max(int(nfloats), 1), dtype=dtype, device=device)
    return buf


def sum_ws(device):
    """Double workspace of the small-sum launchers (mgv_sum_workspace_doubles), per (device, stream)."""
    return workspace(_hip.call_value('mgv_sum_workspace_doubles'), device, torch.float64)


def _sw(device):
    ws = sum_ws(device)
    return ptr(ws), ws.numel()


def _stage_ws(H, N, device):
    """Scratch slab of mgv_struct_stage_bwd2_x3 (one per device, grown on demand; contents are never read across calls)."""
    return workspace(_hip.call_value('mgv_struct_stage_bwd2_ws_floats', H, N), device)


def struct_stage_bwd(h_in, nbr_ptr, nbr_idx, xcls, xtab, Wc, bc, Whh, bhh, ln_w, ln_b, gy_direct, gy_agg,
                     grads, need_input_grad=True, wpack=None, heavy=None, table_own=None, n_rows=None, stats=None, tagged=True):
    """`grads` = dict of fp32 accumulators (dWc, dbc, dWhh, dbhh, dxtab, dln_w, dln_b), added to."""
    N, H = h_in.shape
    if n_rows is not None:
        N = int(n_rows)
    if table_own is not None:
        N = table_own.numel()
    check(gy_direct, F32, 'gy_direct'); check(gy_agg, F32, 'gy_agg')
    x3, dev = use_x3(H), h_in.device
    assert x3 or table_own is None, 'own rows through an index need the bf16x3 kernels'
    assert (x3 and H == 64) or table_own is None or not tagged, 'table mode needs the H = 64 bf16x3 backward'
    g_direct = torch.empty(N, H, dtype=F32, device=dev) if need_input_grad else None
    g_agg = torch.empty(N, H, dtype=F32, device=dev) if need_input_grad else None
    if x3:
        wpack = stage_wpack(Wc, Whh) if wpack is None else wpack
        weights = (ptr(wpack), ptr(bc), ptr(bhh))
    else:
        weights = (ptr(Wc), ptr(Wc.t().contiguous()), ptr(bc), ptr(Whh), ptr(Whh.t().contiguous()), ptr(bhh))
    head = (H, N, ptr(h_in), ptr(nbr_ptr), ptr(nbr_idx), ptr(xcls), ptr(xtab), xtab.shape[0], *weights, ptr(ln_w), ptr(ln_b), LN_EPS,
            ptr(gy_direct), ptr(gy_agg), ptr(g_direct), ptr(g_agg), ptr(grads['dWc']), ptr(grads['dbc']), ptr(grads['dWhh']),
            ptr(grads['dbhh']), ptr(grads['dxtab']), ptr(grads.get('dln_w')), ptr(grads.get('dln_b')))
    if x3 and H == 64:
        ws = _stage_ws(H, N, dev)
        _hip.call('mgv_struct_stage_bwd2_x3', *head, ptr(ws), ws.numel(), *_heavy_args(heavy, H, dev), ptr(table_own), int(bool(tagged)), ptr(stats))
    elif x3:
        _hip.call('mgv_struct_stage_bwd_x3', *head, *_heavy_args(heavy, H, dev), ptr(table_own), 0)
    else:
        _hip.call('mgv_struct_stage_bwd', *head)
    return g_direct, g_agg


# MGV_SEG_LISTS=0 keeps the per-colour gradient sums on mgv_seg_sum (items -> nbr_ptr -> nbr_idx resolved per call) for a same-process
# A/B; default: mgv_seg_sum_entries over flat entry lists (bit-identical sums).  Tests flip this flag.
SEG_LISTS = os.environ.get('MGV_SEG_LISTS', '1') != '0'


def _seg_sums(H, tables, items, direct, agg=None, nbr_ptr=None, nbr_idx=None, entries=None):
    """Per-group row sums through the segment tables of GraphPlan.class_sum_levels: level 1 reads rows `items` of `direct` (+ the
    neighbour pull of `agg`), every further level the partial rows the one before left behind the C final rows of the same buffer.
    `entries` = GraphPlan.seg_entries(...) of the same tables and lists: (flat entry list, level-1 segment pointers in entry positions),
    what mgv_seg_sum_entries reads for a level 1 with a pull; a level without a pull needs none (its items are an entry list as they
    stand, the upper levels read the identity list).  A level 1 with a pull and no list runs on mgv_seg_sum."""
    buf = torch.empty(tables['rows'], H, dtype=F32, device=direct.device)
    for li, (n_seg, seg_ptr, out_row, src_row) in enumerate(tables['levels']):
        if li > 0:
            if SEG_LISTS:
                _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(seg_ptr), None, ptr(buf[src_row:]), None, ptr(out_row), ptr(buf))
            else:
                _hip.call('mgv_seg_sum', H, n_seg, ptr(seg_ptr), None, ptr(buf[src_row:]), None, None, None, ptr(out_row), ptr(buf))
        elif SEG_LISTS and agg is None:
            _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(seg_ptr), ptr(items), ptr(direct), None, ptr(out_row), ptr(buf))
        elif SEG_LISTS and entries is not None:
            _hip.call('mgv_seg_sum_entries', H, n_seg, ptr(entries[1]), ptr(entries[0]), ptr(direct), ptr(agg), ptr(out_row), ptr(buf))
        else:
            _hip.call('mgv_seg_sum', H, n_seg, ptr(seg_ptr), ptr(items), ptr(direct), ptr(agg), ptr(nbr_ptr), ptr(nbr_idx), ptr(out_row), ptr(buf))
    return buf[:tables['C']]


# One half round of StructEncoderFn, as half_round_schedule lays it out:
#   rev, rows            direction (True: over the out-CSR), and how many rows the stage computes
#   ptr, idx, xcls       the neighbour lists and class bytes of those rows;  heavy: (count, rows with long lists) or None
#   table_own, tagged, n_rows   as struct_stage_fwd takes them
#   src                  its input: 'ones' [rows, H] | 'prev' the previous output, read in place | 'stacked' [own rows | previous
#                        output], own rows = previous output rows `own` (colour stages on the fp32 kernels)
#   expand               class ids [N] by which its output table is expanded to N rows behind it, or None
#   grad, gsrc           how the gradient reaches it on the way back: 'rows' per node, as the stage after it left it | 'pairs'
#                        summed per (degree, class) pair (cid, per-node lists) | 'sum_levels' summed per colour over the per-node
#                        lists (the last colour stage: (order, levels), per-node lists) | 'above' from the colour stage after it,
#                        summed over the representatives that own a colour and the list entries that name it
HalfRound = namedtuple('HalfRound', 'rev rows ptr idx xcls heavy table_own tagged n_rows src own expand grad gsrc',
                       defaults=(None, True, None, 'prev', None, None, 'rows', None))


def half_round_schedule(plan, xcls, rounds, H, x3, first, quot):
    """The 2R half rounds of one MultiGCNEncoder as HalfRound records: forward walks them, backward walks them in reverse.
    `first` = plan.first_stage_classes(xcls) or None, `quot` = plan.quotient(xcls, 2R) or empty, `x3`: the bf16x3 kernels serve H.
    node_state = ones (digae_layer.py:260), so the first half round sees identical rows: one kernel row per (degree, class) pair
    does for all nodes of the pair (`first`), and while the rows of a half round are few distinct ones it runs on one
    representative row per colour (`quot`: stages 0..q-1, the table of the last one expanded to N rows).  The rest runs per node."""
    N, quot = plan.N, list(quot or [])[:2 * rounds]
    q = len(quot)
    # table mode for the half round after the pair one: bf16x3 H = 64 kernels read the pair table through tagged entries, it is never expanded
    table_mode = not q and first is not None and x3 and H == 64 and plan.tagged_fits(first[1])
    out = []
    for k in range(2 * rounds):
        rev = k % 2 == 1
        p, i = plan.csr(rev)
        if k < q:
            st = quot[k]
            if k + 1 < q:
                grad, gsrc = 'above', tuple(quot[k + 1][f] for f in ('own_levels', 'own_rows', 'ent_levels', 'ent_rows'))
            else:
                grad, gsrc = 'sum_levels', (st.get('sum_levels'), p, i)
            # the bf16x3 kernels read the previous table in place: own rows through own32, lists name its rows
            lists = (dict(idx=st['ent_idx'], table_own=st['own32'], tagged=False) if x3 else
                     dict(idx=st['idx'], n_rows=st['C'], src='stacked', own=st['own']))
            out.append(HalfRound(rev, st['C'], st['ptr'], xcls=st['xcls'], heavy=st['heavy'], expand=st['cid'] if k + 1 == q else None,
                                 grad=grad, gsrc=gsrc, **lists))
        elif k == 0 and first is not None:
            cid, C, tp, ti, tx = first
            out.append(HalfRound(rev, C, tp, ti, tx, None, src='ones', expand=None if table_mode else cid, grad='pairs', gsrc=(cid, p, i)))
        elif k == 1 and table_mode:
            out.append(HalfRound(rev, N, p, plan.tagged_idx(rev, first[0]), xcls, plan.heavy(rev), table_own=first[0]))
        else:
            out.append(HalfRound(rev, N, p, i, xcls, plan.heavy(rev), src='ones' if k == 0 else 'prev'))
    return out


class StructEncoderFn(torch.autograd.Function):
    """All 2R half rounds of one MultiGCNEncoder (digae_layer.py:257-277) as one autograd node.

    Forward keeps the input state of every half round (per-node stages: 2R x [N,H]); backward walks them in reverse
    and hands each stage's aggregate gradient to the previous stage's gather (consecutive half
    rounds use opposite CSRs), so no scatter pass exists.
    Inputs: the composed per-direction weights (forward half: *_f, reversed half: *_r) and the shared
    LayerNorm affine (None, None = no LayerNorm)."""

    @staticmethod
    def forward(ctx, plan, xcls, rounds, xtab_f, Wc_f, bc_f, Whh_f, bhh_f, xtab_r, Wc_r, bc_r, Whh_r, bhh_r, ln_w, ln_b):
        N = plan.N
        H = Whh_f.shape[1]
        dev = Whh_f.device
        par = [t.detach().contiguous() for t in (xtab_f, Wc_f, bc_f, Whh_f, bhh_f, xtab_r, Wc_r, bc_r, Whh_r, bhh_r)]
        lw = ln_w.detach().contiguous() if ln_w is not None else None
        lb = ln_b.detach().contiguous() if ln_b is not None else None
        packs = (stage_wpack(par[1], par[3]), stage_wpack(par[6], par[8])) if use_x3(H) else (None, None)
        quot = plan.quotient(xcls, 2 * rounds) if (QUOTIENT and FIRST_STAGE_TABLE and rounds > 0 and N > 0 and Whh_f.is_cuda) else []
        first = plan.first_stage_classes(xcls) if (not quot and FIRST_STAGE_TABLE and rounds > 0 and N > 0) else None
        sched = half_round_schedule(plan, xcls, rounds, H, use_x3(H), first, quot)
        keep_stats = lw is not None and use_x3(H) and H == 64      # LayerNorm statistics kept for the bwd2 kernel
        states, stats = [], []
        h = torch.ones(1, H, dtype=F32, device=dev) if quot else None      # the table the first colour stage reads
        for r in sched:
            if r.src == 'ones':
                h = torch.ones(r.rows, H, dtype=F32, device=dev)
            elif r.src == 'stacked':
                h = torch.cat([h.index_select(0, r.own), h])
            states.append(None if r.grad == 'pairs' else h)      # (a few rows of ones: backward makes them again)
            stats.append(torch.empty(r.rows, 2, dtype=F32, device=dev) if keep_stats else None)
            h = struct_stage_fwd(h, r.ptr, r.idx, r.xcls, *(par[5:] if r.rev else par[:5]), lw, lb, wpack=packs[int(r.rev)], heavy=r.heavy,
                                 table_own=r.table_own, n_rows=r.n_rows, stats_out=stats[-1], tagged=r.tagged)
            if r.expand is not None:
                table, h = h, torch.empty(N, H, dtype=F32, device=dev)
                _hip.call('mgv_class_expand', H, N, ptr(table), ptr(r.expand), ptr(h))
        if not sched:
            h = torch.ones(N, H, dtype=F32, device=dev)
        ctx.plan, ctx.packs, ctx.sched = plan, packs, sched
        ctx.par, ctx.lw, ctx.lb, ctx.states, ctx.stats = par, lw, lb, states, stats
        return h

    @staticmethod
    def backward(ctx, gy):
        plan, par, lw, lb = ctx.plan, ctx.par, ctx.lw, ctx.lb
        H, dev = gy.shape[1], gy.device
        dlw = torch.zeros_like(lw) if lw is not None else None
        dlb = torch.zeros_like(lb) if lb is not None else None
        acc = [dict(zip(('dxtab', 'dWc', 'dbc', 'dWhh', 'dbhh', 'dln_w', 'dln_b'), _zeros_like_params(*w) + [dlw, dlb])) for w in (par[:5], par[5:])]
        g_direct, g_agg = gy.contiguous(), None
        for k in range(len(ctx.sched) - 1, -1, -1):
            r, h_in = ctx.sched[k], ctx.states[k]
            if r.grad == 'pairs':
                # parameter gradients are linear in the incoming gradient: sum it per (degree, class) pair,
                # then one backward row per pair
                cid, p, i = r.gsrc
                gsum = torch.zeros(r.rows, H, dtype=F32, device=dev)
                ws = workspace(_hip.call_value('mgv_class_pull_sum_ws_floats', H, plan.N, r.rows), dev)
                _hip.call('mgv_class_pull_sum', H, plan.N, ptr(g_direct), ptr(g_agg), ptr(p), ptr(i), ptr(cid), r.rows, ptr(gsum), ptr(ws), ws.numel())
                g_direct, g_agg, h_in = gsum, None, torch.ones(r.rows, H, dtype=F32, device=dev)
            elif r.grad == 'sum_levels':
                # the last colour stage: per-colour sums of the per-node gradient (g_direct + the pull of g_agg over this stage's
                # lists), colour runs cut into segments, partial rows summed level by level (_seg_sums: mgv_seg_sum_entries over the plan's flat entry list; list order, no atomics)
                (order, levels), p, i = r.gsrc
                flat = plan.seg_entries(r.rev, order, levels) if (SEG_LISTS and g_agg is not None) else None      # (once per plan, beside the stage tables)
                g_direct, g_agg = _seg_sums(H, levels, order, g_direct, g_agg, p, i, entries=flat), None
            elif r.grad == 'above':
                # a colour collects the own-row gradients of the representatives above that own it and the aggregate gradients
                # of those that list it (deterministic gathers over the colour-level lists)
                own_levels, own_rows, ent_levels, ent_rows = r.gsrc
                g_direct, g_agg = _seg_sums(H, own_levels, own_rows, g_direct) + _seg_sums(H, ent_levels, ent_rows, g_agg), None
            g_direct, g_agg = struct_stage_bwd(h_in, r.ptr, r.idx, r.xcls, *(par[5:] if r.rev else par[:5]), lw, lb, g_direct, g_agg, acc[int(r.rev)],
                                               need_input_grad=(k > 0), wpack=ctx.packs[int(r.rev)], heavy=r.heavy, table_own=r.table_own,
                                               n_rows=r.n_rows, stats=ctx.stats[k], tagged=r.tagged)
        ctx.states = ctx.stats = None
        f, r = acc
        return (None, None, None, f['dxtab'], f['dWc'], f['dbc'], f['dWhh'], f['dbhh'],
                r['dxtab'], r['dWc'], r['dbc'], r['dWhh'], r['dbhh'], dlw, dlb)


class StructEncoderRowsFn(torch.autograd.Function):
    """MultiGCNEncoder (digae_layer.py:257-277) for GENERAL node features: x has more distinct rows than the class table holds, so
    the GRU's feature term enters per node — xrow_f / xrow_r [N, 3H] = x W_ih[:, H:]^T + b_ih of the forward / reversed half, formed
    by the caller with ops.linear (autograd carries their gradients to W_ih, b_ih and x through the linear kernels).  Every half
    round runs per node on the exact-fp32 stage kernels (mgv_struct_stage_rows_fwd / _bwd): rows differ node by node, so neither
    the (degree, class) table nor the colour quotient applies.  The reference's Models never reach this path (they feed one-hot
    rows, dg_ae_model_aig.py:59); it completes the encoder's surface."""

    @staticmethod
    def forward(ctx, plan, rounds, xrow_f, Wc_f, bc_f, Whh_f, bhh_f, xrow_r, Wc_r, bc_r, Whh_r, bhh_r, ln_w, ln_b):
        N, H, dev = plan.N, Whh_f.shape[1], Whh_f.device
        par = [check(t.detach().contiguous(), F32, 'encoder parameter') for t in (xrow_f, Wc_f, bc_f, Whh_f, bhh_f, xrow_r, Wc_r, bc_r, Whh_r, bhh_r)]
        lw = ln_w.detach().contiguous() if ln_w is not None else None
        lb = ln_b.detach().contiguous() if ln_b is not None else None
        assert par[0].shape == (N, 3 * H) and par[5].shape == (N, 3 * H)
        h = torch.ones(N, H, dtype=F32, device=dev)
        states = []
        for _ in range(rounds):
            for rev in (False, True):
                p, i = plan.csr(rev)
                w = par[5:] if rev else par[:5]
                states.append(h)
                out = torch.empty(N, H, dtype=F32, device=dev)
                _hip.call('mgv_struct_stage_rows_fwd', H, N, ptr(h), ptr(p), ptr(i), ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(w[4]),
                          ptr(lw), ptr(lb), LN_EPS, ptr(out))
                h = out
        ctx.plan, ctx.rounds, ctx.par, ctx.lw, ctx.lb, ctx.states = plan, rounds, par, lw, lb, states
        return h

    @staticmethod
    def backward(ctx, gy):
        plan, par, lw, lb = ctx.plan, ctx.par, ctx.lw, ctx.lb
        N, H, dev = plan.N, gy.shape[1], gy.device
        acc = {}
        for tag, w in (('f', par[:5]), ('r', par[5:])):
            acc[tag] = [torch.zeros_like(t) for t in w]          # d_xrow, dWc, dbc, dWhh, dbhh
            acc[tag] += [w[1].t().contiguous(), w[3].t().contiguous()]
        dlw = torch.zeros_like(lw) if lw is not None else None
        dlb = torch.zeros_like(lb) if lb is not None else None
        g_direct, g_agg = gy.contiguous(), None
        k = len(ctx.states) - 1
        for _ in range(ctx.rounds):
            for rev in (True, False):
                p, i = plan.csr(rev)
                w = par[5:] if rev else par[:5]
                g = acc['r' if rev else 'f']
                gd = torch.empty(N, H, dtype=F32, device=dev) if k > 0 else None
                ga = torch.empty(N, H, dtype=F32, device=dev) if k > 0 else None
                _hip.call('mgv_struct_stage_rows_bwd', H, N, ptr(ctx.states[k]), ptr(p), ptr(i), ptr(w[0]), ptr(w[1]), ptr(g[5]), ptr(w[2]),
                          ptr(w[3]), ptr(g[6]), ptr(w[4]), ptr(lw), ptr(lb), LN_EPS, ptr(g_direct), ptr(g_agg), ptr(gd), ptr(ga),
                          ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]), ptr(g[0]), ptr(dlw), ptr(dlb))
                g_direct, g_agg = gd, ga
                k -= 1
        ctx.states = None
        f, r = acc['f'], acc['r']
        return (None, None, f[0], f[1], f[2], f[3], f[4], r[0], r[1], r[2], r[3], r[4], dlw, dlb)


# ------------------------------------------------------------------------------------------------
# Linear over node rows (hs_linear / hs_decompose / VAE heads / readout layers)
# ------------------------------------------------------------------------------------------------
_LIN_X3 = {}


def _lin_x3(M, K):
    """Layer shapes served by the bf16x3 linear kernels (the others stay on the fp32 MFMA ones)."""
    if PRECISION != 'x3':
        return False
    key = (int(M), int(K))
    if key not in _LIN_X3:
        _LIN_X3[key] = bool(_hip.call_value('mgv_linear_x3_supported', *key))
    return _LIN_X3[key]


# MGV_FUSED_LINEAR_BWD=0 keeps a Linear's input- and weight-gradient launches separate for a same-process A/B: tests flip this flag
FUSED_LINEAR_BWD = os.environ.get('MGV_FUSED_LINEAR_BWD', '1') != '0'


def _lin_bwd_x3(M, K):
    """Layer shapes whose whole backward is one launch (mgv_linear_bwd_x3)."""
    if PRECISION != 'x3':
        return False
    key = ('bwd', int(M), int(K))
    if key not in _LIN_X3:
        _LIN_X3[key] = bool(_hip.call_value('mgv_linear_bwd_x3_supported', int(M), int(K)))
    return _LIN_X3[key]


def _lin_fwd(x1, x2, W, b, M, wpack=None, res=None):
    """wpack given: W is ignored (bf16x3 path with a ready fragment-order pack).  res [N, M]: added to the result (in the
    kernel's store phase on the bf16x3 path)."""
    N, K1 = x1.shape
    K2 = 0 if x2 is None else x2.shape[1]
    check(x1, F32, 'x1'); check(x2, F32, 'x2'); check(b, F32, 'b')
    y = torch.empty(N, M, dtype=F32, device=x1.device)
    if wpack is not None or _lin_x3(M, K1 + K2):
        if wpack is None:
            wpack = linear_wpack(check(W, F32, 'W'))
        if res is not None:
            res = _rowmajor(check(res, F32, 'res'))
            _hip.call('mgv_linear_fwd_x3_res', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0),
                      ptr(wpack), ptr(b), M, ptr(res), res.stride(0), ptr(y), M)
        else:
            _hip.call('mgv_linear_fwd_x3', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0),
                      ptr(wpack), ptr(b), M, ptr(y), M)
        return y
    check(W, F32, 'W')
    assert W.shape == (M, K1 + K2)
    _hip.call('mgv_linear_fwd', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0),
              ptr(W), ptr(b), M, ptr(y), M)
    return y if res is None else y.add_(res)


def _rowmajor(t):
    """Tensors whose rows are contiguous (column slices of a wider matrix are fine)."""
    if t is None:
        return None
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def _linear_backward(x1, x2, W, has_b, needs, gy, g_pass=None):
    """(gx1, gx2, gW, gb) of y = [x1 | x2] W^T + b for the upstream gy; `needs` as ctx.needs_input_grad of (x1, x2, W, b); g_pass
    (optional) is added to gx1 in the input-gradient kernel's store phase."""
    gy = _rowmajor(gy).contiguous()      # (a column slice of a wider gradient, e.g. behind torch.cat, arrives row-strided)
    N, K1 = x1.shape
    K2 = 0 if x2 is None else x2.shape[1]
    M = W.shape[0]
    gx1 = gx2 = gW = gb = None
    def dgrad(Ws, Kx, res=None):    # gy [N, M] x Ws [M, Kx]: the transposed weight view is packed straight from W
        if _lin_x3(Kx, M):
            pack = torch.empty(2 * Ws.numel(), dtype=torch.bfloat16, device=W.device)
            _pack_into(pack, 0, Ws, True)
            return _lin_fwd(gy, None, None, None, Kx, wpack=pack, res=res)
        return _lin_fwd(gy, None, Ws.t().contiguous(), None, Kx, res=res)
    want_w = needs[2] or (has_b and needs[3])
    if (FUSED_LINEAR_BWD and want_w and needs[0] and (x2 is None or needs[1]) and _lin_bwd_x3(M, K1 + K2)
            and _lin_x3(K1, M) and (x2 is None or _lin_x3(K2, M))):
        # input and weight gradients in one pass over gy (the same bits as the separate launches below)
        pack = torch.empty(2 * W.numel(), dtype=torch.bfloat16, device=W.device)
        _pack_into(pack, 0, W, True)
        res = _rowmajor(check(g_pass.detach(), F32, 'g_pass')) if g_pass is not None else None
        gx1 = torch.empty(N, K1, dtype=F32, device=W.device)
        gx2 = torch.empty(N, K2, dtype=F32, device=W.device) if x2 is not None else None
        gW = torch.zeros_like(W)
        gb = torch.zeros(M, dtype=F32, device=W.device) if has_b else None
        ws = workspace(_hip.call_value('mgv_linear_wgrad_x3_ws_floats', M, K1 + K2, N), W.device)
        _hip.call('mgv_linear_bwd_x3', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0), ptr(gy), gy.stride(0),
                  M, ptr(pack), ptr(gW), ptr(gb), ptr(gx1), K1, ptr(gx2), K2, ptr(res), 0 if res is None else res.stride(0), ptr(ws), ws.numel())
        return gx1, gx2, gW, gb
    if needs[0]:
        gx1 = dgrad(W[:, :K1], K1, res=g_pass.detach() if g_pass is not None else None)
    if x2 is not None and needs[1]:
        gx2 = dgrad(W[:, K1:], K2)
    if want_w:
        gW = torch.zeros_like(W)
        gb = torch.zeros(M, dtype=F32, device=W.device) if has_b else None
        if _lin_x3(M, K1 + K2):
            ws = workspace(_hip.call_value('mgv_linear_wgrad_x3_ws_floats', M, K1 + K2, N), W.device)
            _hip.call('mgv_linear_wgrad_x3', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0),
                      ptr(gy), gy.stride(0), M, ptr(gW), ptr(gb), ptr(ws), ws.numel())
        else:
            _hip.call('mgv_linear_wgrad', N, ptr(x1), K1, x1.stride(0), ptr(x2), K2, 0 if x2 is None else x2.stride(0),
                      ptr(gy), gy.stride(0), M, ptr(gW), ptr(gb))
    return gx1, gx2, gW, gb


class LinearFn(torch.autograd.Function):
    """y = [x1 | x2] W^T + b on the MFMA row-streaming kernel (x2 optional: fuses torch.cat).
    `passthrough`: also return x1 itself; a second consumer of x1 that reads THIS output hands its gradient to this node's
    backward, whose input-gradient kernel adds it in its store phase — autograd then sees one consumer of x1, no N x K add."""

    @staticmethod
    def forward(ctx, x1, x2, W, b, passthrough=False):
        x1d, x2d = _rowmajor(x1.detach()), _rowmajor(x2.detach()) if x2 is not None else None
        Wd = W.detach().contiguous()
        bd = b.detach().contiguous() if b is not None else None
        ctx.save_for_backward(x1d, x2d, Wd)
        ctx.has_b = b is not None
        ctx.set_materialize_grads(False)
        y = _lin_fwd(x1d, x2d, Wd, bd, W.shape[0])
        return (y, x1.view_as(x1)) if passthrough else y

    @staticmethod
    def backward(ctx, gy, g_pass=None):
        x1, x2, W = ctx.saved_tensors
        if gy is None:                     # only the pass-through output was used
            return g_pass, None, None, None, None
        return _linear_backward(x1, x2, W, ctx.has_b, ctx.needs_input_grad, gy, g_pass) + (None,)


def linear(x, W, b=None, x2=None):
    return LinearFn.apply(x, x2, W, b)


def linear_passthrough(x, W, b=None):
    """(y, x'): x' is x; feed x' to the other consumer of x and its gradient is added inside this Linear's input-gradient kernel."""
    return LinearFn.apply(x, None, W, b, True)


# MGV_LINEAR_PAIR=0 keeps hs_linear and hs_decompose on their own launches for a same-process A/B: tests flip this flag
LINEAR_PAIR = os.environ.get('MGV_LINEAR_PAIR', '1') != '0'
# The pair serves batches from this many rows on: the size from which a step is bound by memory and not by launches (the boundary of
# GraphPlan.QUOTIENT_MIN_NODES).  Below it the seam's passes cost nothing that can be measured, and the reconstruction branch keeps
# the launch sequence tests/test_hip_step_branch.py and tests/test_hip_variational_model.py pin on their small batches.
LINEAR_PAIR_MIN_ROWS = 131072


def linear_pair_ok(s, t, Wl, Wd):
    """Whether (hs, st) = linear_pair(s, t, ...) serves these tensors: a training pass at H = 64 in bf16x3 mode on the GPU."""
    return (LINEAR_PAIR and s.shape[0] >= LINEAR_PAIR_MIN_ROWS and PRECISION == 'x3' and s.is_cuda and torch.is_grad_enabled() and tuple(Wl.shape) == (64, 128)
            and tuple(Wd.shape) == (128, 64) and s.shape[1] == 64 and t.shape[1] == 64
            and any(x.requires_grad for x in (s, t, Wl, Wd)))


def _rows_in(t, name):
    """A row matrix as the pair launchers take it: fp32 on the GPU, any row stride _rowmajor accepts (a column slice of a wider
    matrix stays a view; anything else is copied)."""
    if not t.is_cuda or t.dtype != F32:
        raise HipLibraryError('%s must be an fp32 GPU tensor (got %s on %s)' % (name, t.dtype, t.device))
    return _rowmajor(t.detach())


def _grad_in(g):
    """An upstream gradient as the launchers take it."""
    return _rows_in(g, 'gradient')


class LinearPairFn(torch.autograd.Function):
    """(hs, st) = (hs_linear([s | t]), hs_decompose(hs)) in one pass over the rows (mgv_linear_pair_fwd_x3: the bits of the two
    Linears), and their backward in one pass too: dhs = g_st Wd + g_hs lives per tile inside mgv_linear_pair_bwd_x3 and never in
    memory.  A backward that gets no g_st, or that does not want every gradient, runs on the Linears' own kernels."""

    @staticmethod
    def forward(ctx, s, t, Wl, bl, Wd, bd):
        sd, td = _rows_in(s, 's'), _rows_in(t, 't')      # (check() refused the column slices _rowmajor had just let through)
        Wld, Wdd = Wl.detach().contiguous(), Wd.detach().contiguous()
        bld = check(bl.detach().contiguous(), F32, 'bl') if bl is not None else None
        bdd = check(bd.detach().contiguous(), F32, 'bd') if bd is not None else None
        N = sd.shape[0]
        hs = torch.empty(N, 64, dtype=F32, device=sd.device)
        st = torch.empty(N, 128, dtype=F32, device=sd.device)
        _hip.call('mgv_linear_pair_fwd_x3', N, ptr(sd), sd.stride(0), ptr(td), td.stride(0), ptr(linear_wpack(check(Wld, F32, 'Wl'))), ptr(bld),
                  ptr(linear_wpack(check(Wdd, F32, 'Wd'))), ptr(bdd), ptr(hs), 64, ptr(st), 128)
        ctx.save_for_backward(sd, td, Wld, Wdd, hs)
        ctx.has_b = (bl is not None, bd is not None)
        ctx.set_materialize_grads(False)
        return hs, st

    @staticmethod
    def backward(ctx, g_hs, g_st):
        s, t, Wl, Wd, hs = ctx.saved_tensors
        need = ctx.needs_input_grad
        has_bl, has_bd = ctx.has_b
        if g_st is None or not (FUSED_LINEAR_BWD and all(need[:3]) and need[4]):
            # the two Linears' own backward launches: hs_decompose's (g_hs rides in as its residual), then hs_linear's on that dhs
            dhs, gWd, gbd = g_hs, None, None
            if g_st is not None:
                dhs, _, gWd, gbd = _linear_backward(hs, None, Wd, has_bd, (True, False, need[4], need[5]), g_st, g_hs)
            if dhs is None:
                return None, None, None, None, None, None
            return _linear_backward(s, t, Wl, has_bl, need[:4], dhs) + (gWd, gbd)
        dev = Wl.device
        N = s.shape[0]
        g_st = _grad_in(g_st)
        g_hs = _grad_in(g_hs) if g_hs is not None else None
        packs = torch.empty(4 * Wl.numel(), dtype=torch.bfloat16, device=dev)
        _pack_into(packs, _pack_into(packs, 0, Wl, True), Wd, True)
        gs, gt = torch.empty(N, 64, dtype=F32, device=dev), torch.empty(N, 64, dtype=F32, device=dev)
        gWl, gWd = torch.zeros_like(Wl), torch.zeros_like(Wd)
        gbl = torch.zeros(64, dtype=F32, device=dev) if has_bl else None
        gbd = torch.zeros(128, dtype=F32, device=dev) if has_bd else None
        ws = workspace(_hip.call_value('mgv_linear_pair_bwd_x3_ws_floats', N), dev)
        _hip.call('mgv_linear_pair_bwd_x3', N, ptr(g_st), g_st.stride(0), ptr(g_hs), 0 if g_hs is None else g_hs.stride(0), ptr(hs), 64,
                  ptr(s), s.stride(0), ptr(t), t.stride(0), ptr(packs), _hip.ctypes.c_void_p(packs.data_ptr() + 4 * Wl.numel()),
                  ptr(gs), 64, ptr(gt), 64, ptr(gWl), ptr(gbl), ptr(gWd), ptr(gbd), ptr(ws), ws.numel())
        return gs, gt, gWl, gbl, gWd, gbd


def linear_pair(s, t, Wl, bl, Wd, bd):
    """(hs, st) = (Linear(Wl, bl)([s | t]), Linear(Wd, bd)(hs)): call only where linear_pair_ok(s, t, Wl, Wd)."""
    return LinearPairFn.apply(s, t, Wl, bl, Wd, bd)


class RoundGhFn(torch.autograd.Function):
    """gh[N, 3H] = W_hh[slot(v)] h[v] + b_hh[slot(v)] for every node v the sweep updates (zero rows elsewhere): the hidden half of each
    gate's own GRU for rounds >= 2 (dg_ae_model_aig.py:70,88-94), as ONE grouped Linear over the sweep's (level, slot) tiles
    (csrc/linear_x3.hip grouped mode) — and its backward: the input gradient as a grouped Linear with the transposed packs, the weight
    and bias gradients per slot over the slot's tile list.  W [T, 3H, H], b [T, 3H] stacked in slot order."""

    @staticmethod
    def forward(ctx, plan, h, W, b):
        hd, Wd, bd = check(h.detach().contiguous(), F32, 'h'), check(W.detach().contiguous(), F32, 'W'), check(b.detach().contiguous(), F32, 'b')
        N, H = hd.shape
        T, M = Wd.shape[0], 3 * H
        assert plan.has_levels and plan.num_slots == T and plan.N == N and Wd.shape == (T, M, H) and bd.shape == (T, M)
        pack = torch.empty(T, 2, M * H, dtype=torch.bfloat16, device=hd.device)
        for s_ in range(T):
            _hip.call('mgv_wpack_bf16x3', ptr(Wd[s_]), M, H, H, 0, ptr(pack[s_, 0]), ptr(pack[s_, 1]))
        gh = torch.zeros(N, M, dtype=F32, device=hd.device)
        _hip.call('mgv_grouped_linear_fwd_x3', plan.num_tiles, None, ptr(plan.order), ptr(plan.tile_start), ptr(plan.tile_count), ptr(plan.tile_slot),
                  ptr(hd), H, H, ptr(pack), ptr(bd), M, None, 0, ptr(gh), M)
        ctx.save_for_backward(hd, Wd)
        ctx.plan = plan
        return gh

    @staticmethod
    def backward(ctx, dgh):
        hd, Wd = ctx.saved_tensors
        plan = ctx.plan
        d = check(dgh.contiguous(), F32, 'dgh')
        N, H = hd.shape
        T, M = Wd.shape[0], 3 * H
        packT = torch.empty(T, 2, H * M, dtype=torch.bfloat16, device=hd.device)
        for s_ in range(T):
            _hip.call('mgv_wpack_bf16x3', ptr(Wd[s_]), H, M, H, 1, ptr(packT[s_, 0]), ptr(packT[s_, 1]))      # the transposed view of W[s]
        dh = torch.zeros(N, H, dtype=F32, device=hd.device)
        _hip.call('mgv_grouped_linear_fwd_x3', plan.num_tiles, None, ptr(plan.order), ptr(plan.tile_start), ptr(plan.tile_count), ptr(plan.tile_slot),
                  ptr(d), M, M, ptr(packT), None, H, None, 0, ptr(dh), H)
        dW, db = torch.zeros_like(Wd), torch.zeros(T, M, dtype=F32, device=hd.device)
        stp = plan.slot_tile_ptr
        for s_ in range(T):
            n_t = stp[s_ + 1] - stp[s_]
            if n_t == 0:
                continue
            ws = workspace(_hip.call_value('mgv_grouped_linear_wgrad_x3_ws_floats', M, H, n_t), hd.device)
            tiles = plan.slot_tiles[stp[s_]:]
            _hip.call('mgv_grouped_linear_wgrad_x3', n_t, ptr(tiles), ptr(plan.order), ptr(plan.tile_start), ptr(plan.tile_count), ptr(hd), H, H,
                      ptr(d), M, M, ptr(dW[s_]), ptr(db[s_]), ptr(ws), ws.numel())
        return None, dh, dW, db


class GatherSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, plan, reverse):
        hd = h.detach().contiguous()
        N, H = hd.shape
        p, i = plan.csr(reverse)
        agg = torch.empty_like(hd)
        deg = torch.empty(N, dtype=F32, device=hd.device)
        _hip.call('mgv_gather_sum', H, N, ptr(hd), ptr(p), ptr(i), ptr(agg), ptr(deg))
        ctx.plan, ctx.reverse = plan, reverse
        ctx.mark_non_differentiable(deg)
        return agg, deg

    @staticmethod
    def backward(ctx, gagg, _gdeg):
        g = gagg.contiguous()
        N, H = g.shape
        p, i = ctx.plan.csr(not ctx.reverse)      # the scatter of a gather is the gather over the flipped CSR
        out = torch.empty_like(g)
        _hip.call('mgv_gather_sum', H, N, ptr(g), ptr(p), ptr(i), ptr(out), None)
        return out, None, None


def gather_sum(h, nbr_ptr=None, nbr_idx=None, plan=None, reverse=False):
    if plan is not None:
        return GatherSumFn.apply(h, plan, reverse)
    hd = check(h.detach().contiguous(), F32, 'h')
    N, H = hd.shape
    agg = torch.empty_like(hd)
    deg = torch.empty(N, dtype=F32, device=hd.device)
    _hip.call('mgv_gather_sum', H, N, ptr(hd), ptr(nbr_ptr), ptr(nbr_idx), ptr(agg), ptr(deg))
    return agg, deg


# ------------------------------------------------------------------------------------------------
# DiGAE baseline layer (DirectedGCNConv, digae_layer.py:73-114)
# ------------------------------------------------------------------------------------------------
DIGCN_WIDTHS = (16, 32, 64, 128)          # csrc/mgv_launch.h AllWidths


def digcn_scales(plan, reverse, alpha, beta, self_loops):
    """(r, c) of a DirectedGCNConv over plan.csr(reverse): r[i] = din(i)^-alpha, c[j] = dout(j)^-beta (digae_layer.py:98-105), one
    launch, kept on the plan per (direction, alpha, beta, self_loops)."""
    key = (bool(reverse), float(alpha), float(beta), bool(self_loops))

    def build():
        lp, op = plan.csr(reverse)[0], plan.csr(not reverse)[0]
        check(lp, I32, 'list_ptr'); check(op, I32, 'opp_ptr')
        rc = torch.empty(2, max(plan.N, 1), dtype=F32, device=lp.device)
        _hip.call('mgv_digcn_scales', plan.N, ptr(lp), ptr(op), key[1], key[2], int(key[3]), ptr(rc[0]), ptr(rc[1]))
        return (rc[0], rc[1])
    return plan.cache.get('digcn_scales', key, build)


def _digcn_gather(y, plan, reverse, outer, inner, mask, self_loops, relu):
    N, H = y.shape
    p, i = plan.csr(reverse)
    hn, hnodes = plan.heavy(reverse)
    out = torch.empty_like(y)
    _hip.call('mgv_digcn_gather', H, N, ptr(y), ptr(p), ptr(i), ptr(outer), ptr(inner), ptr(mask), int(self_loops), int(relu),
              hn, ptr(hnodes) if hn else None, ptr(out))
    return out


class DiGCNGatherFn(torch.autograd.Function):
    """z = act(r_i * sum_{j in L(i)} c_j y_j) over plan.csr(reverse), exact fp32 (MessagePassing.propagate with the norm of
    digae_layer.py:107-114, and the F.relu of :127,146 when `relu`).  Backward: the same kernel over the opposite CSR with the
    two scales swapped and the ReLU mask read from z while gathering — a pull, no scatter."""

    @staticmethod
    def forward(ctx, y, plan, reverse, alpha, beta, self_loops, relu):
        yd = check(y.detach().contiguous(), F32, 'y')
        if yd.shape[0] != plan.N or yd.shape[1] not in DIGCN_WIDTHS:
            raise HipLibraryError('DirectedGCNConv rows must be [%d, 16|32|64|128] (got %s)' % (plan.N, tuple(yd.shape)))
        r, c = digcn_scales(plan, reverse, alpha, beta, self_loops)
        z = _digcn_gather(yd, plan, reverse, r, c, None, self_loops, relu)
        ctx.plan, ctx.args = plan, (reverse, self_loops, relu)
        ctx.save_for_backward(r, c, z if relu else None)
        return z

    @staticmethod
    def backward(ctx, gz):
        r, c, z = ctx.saved_tensors
        reverse, self_loops, _ = ctx.args
        g = check(gz.contiguous(), F32, 'gz')
        return _digcn_gather(g, ctx.plan, not reverse, c, r, z, self_loops, False), None, None, None, None, None, None


class DiGCNClassFn(torch.autograd.Function):
    """The first layer when the node features are class rows (digae_layer.feature_classes): z = act(r_i * sum_{j in L(i)} c_j T[cls_j])
    with T [C, H] = rows W^T + b formed by the caller in weight space; one byte per neighbour instead of a row.  Backward: dT."""

    @staticmethod
    def forward(ctx, T, plan, xcls, reverse, alpha, beta, self_loops, relu):
        Td = check(T.detach().contiguous(), F32, 'T')
        check(xcls, U8, 'xcls')
        C, H = Td.shape
        if xcls.shape[0] != plan.N or H not in DIGCN_WIDTHS or not 1 <= C <= 8:
            raise HipLibraryError('DirectedGCNConv class table must be [1..8, 16|32|64|128] over %d nodes (got %s, %d)' % (plan.N, tuple(Td.shape), xcls.shape[0]))
        r, c = digcn_scales(plan, reverse, alpha, beta, self_loops)
        p, i = plan.csr(reverse)
        z = torch.empty(plan.N, H, dtype=F32, device=Td.device)
        _hip.call('mgv_digcn_class_fwd', H, plan.N, ptr(xcls), ptr(Td), C, ptr(p), ptr(i), ptr(r), ptr(c), int(self_loops), int(relu), ptr(z))
        ctx.plan, ctx.args = plan, (reverse, self_loops, C)
        ctx.save_for_backward(r, c, xcls, z if relu else None)
        return z

    @staticmethod
    def backward(ctx, gz):
        r, c, xcls, z = ctx.saved_tensors
        reverse, self_loops, C = ctx.args
        plan = ctx.plan
        g = check(gz.contiguous(), F32, 'gz')
        H = g.shape[1]
        p, i = plan.csr(reverse)
        dT = torch.zeros(C, H, dtype=F32, device=g.device)
        ws = workspace(_hip.call_value('mgv_digcn_class_bwd_ws_floats', H, plan.N), g.device)
        _hip.call('mgv_digcn_class_bwd', H, plan.N, ptr(xcls), C, ptr(p), ptr(i), ptr(r), ptr(c), int(self_loops), ptr(z), ptr(g), ptr(dT),
                  ptr(ws), ws.numel())
        return dT, None, None, None, None, None, None, None


class AttnPoolFn(torch.autograd.Function):
    """zbar[i] = sum_j softmax_j(u . x_j) x_j over i's in-edges (csrc/attn_pool.hip): the stand-alone TFMlpAggr call."""

    @staticmethod
    def forward(ctx, x, u, plan):
        xd = check(x.detach().contiguous(), F32, 'x')
        ud = check(u.detach().contiguous(), F32, 'u')
        N, W = xd.shape
        if W not in (32, 64, 128) or ud.numel() != W:
            raise ValueError('attention pooling: row width %d (u: %d) is not one of 32 / 64 / 128' % (W, ud.numel()))
        zbar = torch.empty_like(xd)
        m, inv = torch.empty(N, dtype=F32, device=xd.device), torch.empty(N, dtype=F32, device=xd.device)
        _hip.call('mgv_attn_pool_fwd', W, N, ptr(plan.in_ptr), ptr(plan.in_src), ptr(xd), ptr(ud), ptr(zbar), ptr(m), ptr(inv))
        ctx.plan = plan
        ctx.save_for_backward(xd, ud, zbar, m, inv)
        return zbar

    @staticmethod
    def backward(ctx, gz):
        xd, ud, zbar, m, inv = ctx.saved_tensors
        N, W = xd.shape
        g = _rowmajor(gz).contiguous()
        dx, du = torch.zeros_like(xd), torch.zeros_like(ud)
        _hip.call('mgv_attn_pool_bwd', W, N, ptr(ctx.plan.in_ptr), ptr(ctx.plan.in_src), ptr(xd), ptr(ud), ptr(zbar), ptr(m), ptr(inv),
                  ptr(g), ptr(dx), ptr(du))
        return dx, du, None


# ------------------------------------------------------------------------------------------------
# levelised functional sweep
# ------------------------------------------------------------------------------------------------
def _sweep_bwd_prep(plan, T, H, dev):
    """Scratch and heavy-list arguments of mgv_func_sweep_bwd_x3."""
    ltp = plan.level_tile_ptr
    widest = max([ltp[i + 1] - ltp[i] for i in range(1, len(ltp) - 1)] + [1])
    # rows for the deferred weight gradient, small-gradient slabs of the widest level, 256 rows of weight-gradient partials
    scratch = torch.empty(plan.n_active * 5 * H + widest * T * 11 * H + 256 * 6 * H * H, dtype=F32, device=dev)
    stp = (_hip.ctypes.c_int32 * len(plan.slot_tile_ptr))(*plan.slot_tile_ptr)
    hv = plan.heavy_segments(True, inactive_only=True)
    hav = plan.heavy_segments(True, active_by_level=True)      # updated gates with very long consumer lists
    if hav is None:
        ha = (0, None, None, None, None, None, None, None, 0)
    else:
        i32a = _hip.ctypes.c_int32
        kp = (i32a * len(hav['lvl_k_ptr']))(*hav['lvl_k_ptr'])
        sp_ = (i32a * len(hav['lvl_seg_ptr']))(*hav['lvl_seg_ptr'])
        hws = workspace((hav['K'] + hav['S']) * 2 * H, dev, tag='heavy_active')      # its own buffer: it must outlive the launcher call's other scratch users
        ha = (hav['K'], ptr(hav['nodes']), ptr(hav['node_seg_ptr']), ptr(hav['seg_e0']), ptr(hav['seg_e1']), kp, sp_, ptr(hws), plan.HEAVY_ROW)
    return scratch, stp, hv, ha


SWEEP_X3_MAX_SLOTS = 6          # csrc/func_level_x3_common.h kMaxSlots: the bf16x3 level kernels keep every slot's attention vector in LDS


def _sweep_x3(H, T=1):
    """The bf16x3 level kernels serve this width and slot count (else the exact-fp32 ones, which have no slot cap: H = 16,
    T > SWEEP_X3_MAX_SLOTS, MGV_PRECISION=f32, MGV_SWEEP_X3=0)."""
    return use_x3(H) and T <= SWEEP_X3_MAX_SLOTS and os.environ.get('MGV_SWEEP_X3', '1') != '0'


GROUPED_ROUND = True            # rounds >= 2: W_hh h_prev + b_hh of every updated gate as one grouped Linear (RoundGhFn); False: per gate type on the plain kernels

# The level kernels read packed rows (GraphPlan.order_rows: spans + first in-edge sources + first consumers, one 128-byte line per
# updated node) or the 16-byte span rows and the CSR lists behind them.  Packed rows cost 0.43 ms to build and save 0.13 ms per sweep
# backward (config 2): they pay from a plan's THIRD step on, so a plan gets them when it comes back for a second step (a resident
# batch) and a batch that is planned, stepped once and dropped (every batch of a shuffled training loop) never builds them.
# MGV_PACKED_ROWS=0: never; =2: from the first step.
PACKED_ROWS = {'0': 0, '2': 2}.get(os.environ.get('MGV_PACKED_ROWS', '1'), 1)


def _sweep_rows(plan, forward=False):
    """(pointer, ints per row) of the rows the level kernels read; `forward`: a sweep forward (counts the plan's steps)."""
    if PACKED_ROWS and forward and plan.cache.peek('order_rows') is None:
        steps = plan.cache.peek('sweep_steps') or 0
        plan.cache.put('sweep_steps', None, steps + 1, level_derived=True)
        if PACKED_ROWS == 2 or steps >= 1:
            plan.order_rows                  # (built here, on the step's stream: 0.43 ms once; the first step's backward keeps the span rows)
    if PACKED_ROWS and plan.cache.peek('order_rows') is not None:
        return ptr(plan.order_rows), 32
    return ptr(plan.order_span), 4


class FuncSweepFn(torch.autograd.Function):
    """hf = sweep(hs) over levels 1..L-1 (dg_ae_model_aig.py:70-97) on the HIP level kernels, bf16x3 or exact fp32; parameters are
    the per-slot composed tensors attn_u [T,2H], Wvc [T,3H,2H], bvc/bih/bhh [T,3H].
    Rounds r >= 2 (num_rounds > 1) pass `hprev` [N, H], the previous round's states, from which every updated gate's GRU starts,
    `gh` [N, 3H] = W_hh h_prev + b_hh of each node's own aggregator, formed by the caller with ops.linear (so that autograd carries
    its gradient to W_hh, b_hh and h_prev through the linear kernels), and bhh=None (b_hh is inside gh: a zero bias).  The level
    kernels add gh to the gate pre-activations, mix z * h_prev into the new state and leave d(gh) and dh * z on the way back.
    High fan-out lists take the same pre-passes in every round (GraphPlan.heavy_segments)."""

    @staticmethod
    def forward(ctx, plan, hs, attn_u, Wvc, bvc, bih, bhh, hprev=None, gh=None):
        hsd = check(hs.detach().contiguous(), F32, 'hs')
        N, H = hsd.shape
        T = attn_u.shape[0]
        if bhh is None:
            bhh = torch.zeros(T, 3 * H, dtype=F32, device=hsd.device)
        par = [check(t.detach().contiguous(), F32, 'sweep parameter') for t in (attn_u, Wvc, bvc, bih, bhh)]
        assert plan.has_levels and plan.num_slots == T and plan.N == N
        hp = ghd = None
        if hprev is not None:
            hp = check(hprev.detach().contiguous(), F32, 'h_prev')
            ghd = check(gh.detach().contiguous(), F32, 'gh')
            assert ghd.shape == (N, 3 * H) and hp.shape == (N, H)
        ltp = (_hip.ctypes.c_int32 * len(plan.level_tile_ptr))(*plan.level_tile_ptr)
        wpack = sweep_wpack(par[1]) if _sweep_x3(H, T) else None
        if hp is not None:
            hf = hp.clone()                  # never-updated rows keep their state; every updated row is rewritten by its level
        elif wpack is not None:
            hf = torch.empty(N, H, dtype=F32, device=hsd.device)          # every updated row is written by its level; the rest here
            _hip.call('mgv_sweep_zero_inactive', H, N, ptr(plan.gslot), ptr(hf))
        else:
            hf = torch.zeros(N, H, dtype=F32, device=hsd.device)
        if wpack is not None:
            _hip.call('mgv_func_sweep_fwd_x3', H, N, T, plan.num_levels, ltp, ptr(plan.order), *_sweep_rows(plan, True),
                      ptr(plan.tile_start), ptr(plan.tile_count), ptr(plan.tile_slot), ptr(plan.in_ptr), ptr(plan.in_src), ptr(hsd), ptr(hf),
                      ptr(par[0]), ptr(wpack), ptr(par[2]), ptr(par[3]), ptr(par[4]), ptr(ghd), ptr(hp))
        else:
            _hip.call('mgv_func_sweep_fwd', H, N, T, plan.num_levels, ltp, ptr(plan.order), ptr(plan.tile_start),
                      ptr(plan.tile_count), ptr(plan.tile_slot), ptr(plan.in_ptr), ptr(plan.in_src), ptr(hsd), ptr(hf),
                      *[ptr(t) for t in par], ptr(ghd), ptr(hp))
        ctx.plan, ctx.par, ctx.ltp, ctx.wpack = plan, par, ltp, wpack
        ctx.save_for_backward(hsd, hf, hp, ghd)
        return hf

    @staticmethod
    def backward(ctx, ghf):
        plan, par = ctx.plan, ctx.par
        hs, hf, hp, ghd = ctx.saved_tensors
        N, H = hs.shape
        T = par[0].shape[0]
        dev = hs.device
        ghf = check(ghf.contiguous(), F32, 'ghf')
        ghs = (torch.empty if ctx.wpack is not None else torch.zeros)(N, H, dtype=F32, device=dev)    # (the fp32 kernels add to it)
        dzb = torch.empty(N, 2 * H, dtype=F32, device=dev)
        alpha = torch.empty(max(plan.E, 1), dtype=F32, device=dev)
        dsc = torch.empty(max(plan.E, 1), dtype=F32, device=dev)
        grads = [torch.zeros_like(t) for t in par]      # rounds >= 2: the last one (dbhh) is not meaningful
        d_gh = g_hprev = None
        if hp is not None:
            d_gh = torch.zeros(N, 3 * H, dtype=F32, device=dev)      # rows of never-updated nodes stay zero
            g_hprev = torch.zeros(N, H, dtype=F32, device=dev)       # (their states are constants of round 1: no gradient to carry)
        rnd = (ptr(ghd), ptr(hp), ptr(d_gh), ptr(g_hprev))
        if ctx.wpack is not None:
            scratch, stp, hv, ha = _sweep_bwd_prep(plan, T, H, dev)
            _hip.call('mgv_func_sweep_bwd_x3', H, N, T, plan.num_levels, ctx.ltp, ptr(plan.order), *_sweep_rows(plan),
                      plan.n_active, ptr(plan.tile_start), ptr(plan.tile_count), ptr(plan.tile_slot), ptr(plan.slot_tiles), stp,
                      ptr(plan.in_ptr), ptr(plan.in_src), ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.out_slot),
                      ptr(plan.gslot), ptr(hs), ptr(hf), ptr(par[0]), ptr(ctx.wpack), ptr(par[2]), ptr(par[3]), ptr(par[4]),
                      ptr(ghf), ptr(ghs), ptr(dzb), ptr(alpha), ptr(dsc), *[ptr(g) for g in grads], ptr(scratch),
                      scratch.numel(), plan.HEAVY_ROW if hv is not None else 0, *ha, *rnd)
            if hv is not None:
                # primary inputs (never updated) that drive thousands of gates: their pull by whole workgroups, per list segment
                pw = workspace(hv['S'] * H, dev)
                _hip.call('mgv_sweep_pull_heavy', H, hv['K'], ptr(hv['nodes']), ptr(hv['node_seg_ptr']), hv['S'], ptr(hv['seg_e0']), ptr(hv['seg_e1']),
                          ptr(plan.out_dst), ptr(plan.out_slot), ptr(plan.gslot), ptr(alpha), ptr(dsc), ptr(dzb), ptr(par[0]), ptr(pw), ptr(ghs))
        else:
            WvcT = par[1].transpose(1, 2).contiguous()
            _hip.call('mgv_func_sweep_bwd', H, N, T, plan.num_levels, ctx.ltp, ptr(plan.order), ptr(plan.tile_start),
                      ptr(plan.tile_count), ptr(plan.tile_slot), ptr(plan.in_ptr), ptr(plan.in_src), ptr(plan.out_ptr),
                      ptr(plan.out_dst), ptr(plan.out_slot), ptr(plan.gslot), ptr(hs), ptr(hf), ptr(par[0]), ptr(par[1]),
                      ptr(WvcT), ptr(par[2]), ptr(par[3]), ptr(par[4]), ptr(ghf), ptr(ghs), ptr(dzb), ptr(alpha), ptr(dsc),
                      *[ptr(g) for g in grads], *rnd)
        return (None, ghs, *grads[:4], grads[4] if hp is None else None, g_hprev, d_gh)


# ------------------------------------------------------------------------------------------------
# decoder, reconstruction loss, confusion counters
# ------------------------------------------------------------------------------------------------
class EdgeDotFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, edge_index, sigmoid):
        sd, td = check(s.detach().contiguous(), F32, 's'), check(t.detach().contiguous(), F32, 't')
        src, dst = edge_rows(edge_index)
        E, H = src.numel(), sd.shape[1]
        out = torch.empty(E, dtype=F32, device=sd.device)
        _hip.call('mgv_edge_dot_fwd', H, E, ptr(sd), ptr(td), H, ptr(src), ptr(dst), int(bool(sigmoid)), ptr(out))
        ctx.save_for_backward(sd, td, src, dst)
        ctx.sigmoid = bool(sigmoid)
        return out

    @staticmethod
    def backward(ctx, gout):
        sd, td, src, dst = ctx.saved_tensors
        H = sd.shape[1]
        ds, dt = torch.zeros_like(sd), torch.zeros_like(td)
        gout = gout.contiguous()             # (named: the launcher takes a raw pointer)
        _hip.call('mgv_edge_dot_bwd', H, src.numel(), ptr(sd), ptr(td), H, ptr(src), ptr(dst), int(ctx.sigmoid),
                  ptr(gout), ptr(ds), ptr(dt))
        return ds, dt, None, None


def edge_dot(s, t, edge_index, sigmoid=True):
    return EdgeDotFn.apply(s, t, edge_index, sigmoid)


def _recon_heavy(plan):
    """((which, segments, list), ...) of the plan's heavy positive lists and the list length from which the per-node walk leaves
    them to the segment kernels (0: no heavy list)."""
    heavy = [(0, plan.heavy_segments(True), plan.out_dst), (1, plan.heavy_segments(False), plan.in_src)]
    return heavy, (plan.HEAVY_ROW if any(hv is not None for _, hv, _ in heavy) else 0)


class ReconLossFn(torch.autograd.Function):
    """-mean log(sigma(<s_u,t_v>)+1e-15) over positives - mean log(1-sigma+1e-15) over negatives
    (dg_ae_model_aig.py:108-130) on st = hs_decompose(hs) [N,2H]; also the confusion counters and,
    on request, pred_bin.
    Two routes.  The pair pass (mgv_recon_loss_fwd) with the gradient walk in backward; and, for a training step (plan and neg_csr
    given, st requires grad, grad mode on at `apply`, no pred_bin wanted), ONE walk of the lists in forward that leaves the loss
    sums, the counters and the gradient rows for the upstream gradient `expect_scale` (mgv_recon_step_csr).  backward then only
    compares the upstream gradient it is given with expect_scale on the device and rescales the rows if they differ.
    MGV_RECON_ONE_PASS=0 keeps every call on the pair pass."""

    @classmethod
    def apply(cls, st, pos_edge_index, neg_edge_index, want_pred, plan=None, neg_csr=None, expect_scale=1.0):
        """`expect_scale`: the upstream gradient the caller will bring to backward (Trainer: the loss's weight).  A hint: any other
        upstream gradient is served as well, by one more pass over the rows."""
        # (grad mode is off inside forward: whether this call will ever see a backward is decided here)
        expect_scale = float(expect_scale)
        one_pass = bool(plan is not None and neg_csr is not None and not want_pred and torch.is_grad_enabled() and st.requires_grad
                        and st.is_cuda and expect_scale != 0.0 and math.isfinite(expect_scale)
                        and os.environ.get('MGV_RECON_ONE_PASS', '1') != '0')
        return super().apply(st, pos_edge_index, neg_edge_index, want_pred, plan, neg_csr, expect_scale if one_pass else None)

    @staticmethod
    def forward(ctx, st, pos_edge_index, neg_edge_index, want_pred, plan=None, neg_csr=None, expect_scale=None):
        """`plan`: GraphPlan whose edges are exactly pos_edge_index (any order) -> atomic-free positive half;
        `neg_csr`: (out_ptr, out_dst, in_ptr, in_src) over neg_edge_index (sampling.NegativeEdges) -> atomic-free
        negative half as well; `expect_scale` not None: the one-walk route (see `apply`)."""
        std = check(st.detach().contiguous(), F32, 'st')
        N, H2 = std.shape
        H = H2 // 2
        ps, pd = edge_rows(pos_edge_index)
        ns, nd = edge_rows(neg_edge_index)
        Ep, En = ps.numel(), ns.numel()
        dev = std.device
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        pred = torch.empty(Ep + En, dtype=torch.int32, device=dev) if want_pred else None
        t_view = std[:, H:]
        ctx.dst_ = ctx.expect_scale = None
        if expect_scale is not None:
            dst_ = torch.empty_like(std)
            heavy, skip = _recon_heavy(plan)
            _hip.call('mgv_recon_step_csr', H, N, ptr(std), ptr(t_view), H2, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(plan.in_ptr),
                      ptr(plan.in_src), Ep, *[ptr(c) for c in neg_csr], En, expect_scale, ptr(sums), ptr(counts), ptr(dst_),
                      ptr(dst_[:, H:]), skip, *_sw(dev))
            for which, hv, lst in heavy:
                if hv is not None:
                    pw = workspace(hv['S'] * H, dev)
                    _hip.call('mgv_recon_step_heavy_lists', H, ptr(std), ptr(t_view), H2, Ep, expect_scale, hv['K'], ptr(hv['nodes']),
                              ptr(hv['node_seg_ptr']), hv['S'], ptr(hv['seg_node']), ptr(hv['seg_e0']), ptr(hv['seg_e1']), ptr(lst), which,
                              ptr(pw), ptr(dst_[:, H:]) if which else ptr(dst_), ptr(sums), ptr(counts), *_sw(dev))
            ctx.dst_, ctx.expect_scale = dst_, expect_scale      # lives until backward: one more [N, 2H] beside std
        else:
            _hip.call('mgv_recon_loss_fwd', H, ptr(std), ptr(t_view), H2, ptr(ps), ptr(pd), Ep, ptr(ns), ptr(nd), En,
                      ptr(sums), ptr(counts), ptr(pred), *_sw(std.device))
        loss = (sums[0] / max(Ep, 1) + sums[1] / max(En, 1)).to(F32)
        ctx.save_for_backward(std, ps, pd, ns, nd)
        ctx.plan, ctx.neg_csr = plan, neg_csr
        ctx.mark_non_differentiable(counts)
        if pred is not None:
            ctx.mark_non_differentiable(pred)
            return loss, counts, pred
        return loss, counts, torch.empty(0, dtype=torch.int32, device=dev)

    @staticmethod
    def backward(ctx, gloss, _gc, _gp):
        std, ps, pd, ns, nd = ctx.saved_tensors
        H2 = std.shape[1]
        H = H2 // 2
        g = gloss.detach().to(F32).reshape(1).contiguous()
        pl = ctx.plan
        if ctx.dst_ is not None:
            # the rows the forward's walk left, formed for expect_scale: mended on the device if the upstream gradient is another
            # (no host read).  They are handed over: a second backward through the same graph takes the walk below.
            dst_, ctx.dst_ = ctx.dst_, None
            _hip.call('mgv_rows_rescale_unless', dst_.numel(), ptr(dst_), ptr(g), ctx.expect_scale)
            return dst_, None, None, None, None, None, None
        if pl is not None and ctx.neg_csr is not None:
            dst_ = torch.empty_like(std)
            # positive lists of high fan-out / fan-in nodes: skipped by the per-node pull, summed per segment by whole workgroups
            heavy, skip = _recon_heavy(pl)
            _hip.call('mgv_recon_loss_bwd_csr', H, std.shape[0], ptr(std), ptr(std[:, H:]), H2, ptr(pl.out_ptr), ptr(pl.out_dst),
                      ptr(pl.in_ptr), ptr(pl.in_src), ps.numel(), *[ptr(c) for c in ctx.neg_csr], ns.numel(), ptr(g), ptr(dst_),
                      ptr(dst_[:, H:]), skip)
            for which, hv, lst in heavy:
                if hv is not None:
                    pw = workspace(hv['S'] * H, std.device)
                    _hip.call('mgv_recon_heavy_lists', H, ptr(std), ptr(std[:, H:]), H2, ps.numel(), ptr(g), hv['K'], ptr(hv['nodes']),
                              ptr(hv['node_seg_ptr']), hv['S'], ptr(hv['seg_node']), ptr(hv['seg_e0']), ptr(hv['seg_e1']), ptr(lst), which,
                              ptr(pw), ptr(dst_[:, H:]) if which else ptr(dst_))
            return dst_, None, None, None, None, None, None
        dst_ = torch.zeros_like(std)
        csr = (pl.out_ptr, pl.out_dst, pl.in_ptr, pl.in_src) if pl is not None else (None, None, None, None)
        _hip.call('mgv_recon_loss_bwd', H, std.shape[0], ptr(std), ptr(std[:, H:]), H2, ptr(ps), ptr(pd), ps.numel(),
                  *[ptr(c) for c in csr], ptr(ns), ptr(nd), ns.numel(), ptr(g), ptr(dst_), ptr(dst_[:, H:]))
        return dst_, None, None, None, None, None, None


def confusion_counts(pred_bin, gt_bin):
    """{TP, FP, TN, FN} counts (trainer.py:240-244) as an int64[4] device tensor."""
    counts = torch.zeros(4, dtype=torch.int64, device=pred_bin.device)
    _hip.call('mgv_confusion', pred_bin.numel(), ptr(check(pred_bin.contiguous(), torch.int32, 'pred_bin')),
              ptr(check(gt_bin.contiguous(), torch.int32, 'gt_bin')), ptr(counts))
    return counts


# ------------------------------------------------------------------------------------------------
# losses on node rows
# ------------------------------------------------------------------------------------------------
class L1LossFn(torch.autograd.Function):
    """nn.L1Loss() (mean) as used for the probability task (trainer.py:71,156)."""

    @staticmethod
    def forward(ctx, x, target):
        xd = check(x.detach().contiguous(), F32, 'x')
        td = check(target.detach().contiguous(), F32, 'target')
        assert xd.numel() == td.numel()
        s = torch.zeros(1, dtype=torch.float64, device=xd.device)
        _hip.call('mgv_l1_loss_fwd', xd.numel(), ptr(xd), ptr(td), ptr(s), *_sw(xd.device))
        ctx.save_for_backward(xd, td)
        return (s[0] / max(xd.numel(), 1)).to(F32)

    @staticmethod
    def backward(ctx, g):
        xd, td = ctx.saved_tensors
        dx = torch.empty_like(xd)
        gs = g.detach().to(F32).reshape(1).contiguous()
        _hip.call('mgv_l1_loss_bwd', xd.numel(), ptr(xd), ptr(td), ptr(gs), ptr(dx))
        return dx, None


def l1_loss(x, target):
    return L1LossFn.apply(x, target)


def pair_lists(tt_pair_index, num_nodes):
    """The truth-table pairs grouped by first and by second member: (a_ptr[N+1], a_pair[P], b_ptr[N+1], b_pair[P]), pair ids in
    their original order inside a group (csrc/plan_build.hip).  Static per batch: the trainer caches it on the batch."""
    pa, pb = edge_rows(tt_pair_index)
    P, N, dev = pa.numel(), int(num_nodes), pa.device
    i32 = dict(dtype=I32, device=dev)
    a_ptr, b_ptr = torch.empty(N + 1, **i32), torch.empty(N + 1, **i32)
    junk = torch.empty(4, max(P, 1), **i32)                      # neighbour / slot arrays of the CSR build, not needed here
    a_pair, b_pair = torch.empty(max(P, 1), **i32), torch.empty(max(P, 1), **i32)
    n_s = _hip.call_value('mgv_plan_csr_scratch_ints', N, P)
    scratch = torch.empty(n_s, **i32)
    status = torch.empty(2, **i32)
    _hip.call('mgv_plan_csr', N, P, ptr(pa), ptr(pb), ptr(b_ptr), ptr(junk[0]), ptr(junk[1]), ptr(a_ptr), ptr(junk[2]), ptr(junk[3]),
              ptr(b_pair), ptr(a_pair), ptr(scratch), n_s, ptr(status))
    if int(status[0].item()) != 0:           # built once per batch and cached: one host read
        raise ValueError('tt_pair_index holds node ids outside [0, num_nodes)')
    return a_ptr, a_pair, b_ptr, b_pair


class FuncLossFn(torch.autograd.Function):
    """L1(z(1 - cos(hf[a], hf[b])), z(tt_sim)) with z = zero_normalization (trainer.py:158-163).
    `lists` (optional, from pair_lists): backward without atomics and without a zero-filled gradient.
    `passthrough`: also return hf itself; a second consumer of hf (the readout) that reads THIS output hands its gradient to
    this node's backward, whose pull kernel adds it on the way out — autograd then sees one consumer of hf and no N x H add."""

    @staticmethod
    def forward(ctx, hf, tt_pair_index, tt_sim, lists=None, passthrough=False):
        hfd = check(hf.detach().contiguous(), F32, 'hf')
        pa, pb = edge_rows(tt_pair_index)
        tt = check(tt_sim.detach().to(F32).contiguous(), F32, 'tt_sim')
        P, H = pa.numel(), hfd.shape[1]
        dis = torch.empty(P, dtype=F32, device=hfd.device)
        ws = torch.zeros(8, dtype=torch.float64, device=hfd.device)
        _hip.call('mgv_func_loss_fwd', H, P, ptr(hfd), ptr(pa), ptr(pb), ptr(tt), 1e-8, ptr(dis), ptr(ws), *_sw(hfd.device))
        ctx.save_for_backward(hfd, pa, pb, tt, dis, ws)
        ctx.lists = lists
        ctx.set_materialize_grads(False)
        loss = (ws[4] / P).to(F32)
        if passthrough:
            return loss, hf.view_as(hf)
        return loss

    @staticmethod
    def backward(ctx, g, g_pass=None):
        hfd, pa, pb, tt, dis, ws = ctx.saved_tensors
        if g is None:                      # only the pass-through output was used
            return g_pass, None, None, None, None
        gs = g.detach().to(F32).reshape(1).contiguous()
        if ctx.lists is not None:
            dhf = torch.empty_like(hfd)
            add = check(g_pass.detach().contiguous(), F32, 'g_pass') if g_pass is not None else None
            _hip.call('mgv_func_loss_bwd_csr', hfd.shape[1], hfd.shape[0], pa.numel(), ptr(hfd), ptr(pa), ptr(pb), ptr(tt), ptr(dis), 1e-8,
                      ptr(ws), ptr(gs), *[ptr(t) for t in ctx.lists], ptr(add), ptr(dhf))
            return dhf, None, None, None, None
        dhf = torch.zeros_like(hfd) if g_pass is None else g_pass.detach().to(F32).clone()
        _hip.call('mgv_func_loss_bwd', hfd.shape[1], pa.numel(), ptr(hfd), ptr(pa), ptr(pb), ptr(tt), ptr(dis), 1e-8,
                  ptr(ws), ptr(gs), ptr(dhf))
        return dhf, None, None, None, None


def _pair_lists_for(hf, tt_pair_index, cache):
    lists = None
    if cache is not None and hf.is_cuda and tt_pair_index.shape[1] >= 2:
        lists = getattr(cache, '_mgv_pair_lists', None)
        if lists is None or lists[0].numel() != hf.shape[0] + 1 or lists[1].device != hf.device:
            lists = pair_lists(tt_pair_index, hf.shape[0])
            cache._mgv_pair_lists = lists
    return lists


def func_loss(hf, tt_pair_index, tt_sim, cache=None):
    """`cache`: any object that lives as long as the pairs do (the batch): the grouped pair lists are built once and kept on it."""
    return FuncLossFn.apply(hf, tt_pair_index, tt_sim, _pair_lists_for(hf, tt_pair_index, cache))


def func_loss_passthrough(hf, tt_pair_index, tt_sim, cache=None):
    """(loss, hf'): hf' is hf; feed hf' to the other consumer of hf (the readout) and the two gradients meet inside the
    function-loss backward kernel instead of in an N x H add."""
    return FuncLossFn.apply(hf, tt_pair_index, tt_sim, _pair_lists_for(hf, tt_pair_index, cache), True)


# ------------------------------------------------------------------------------------------------
# readout: BatchNorm1d + ReLU + Dropout block, 32 -> 1 head with clamp
# ------------------------------------------------------------------------------------------------
class BnReluDropFn(torch.autograd.Function):
    """dropout_p(relu(batch_norm(y))) for y [N,C] (mlp.py:31-36).  training=True uses batch statistics
    and updates the running buffers in place like nn.BatchNorm1d (momentum 0.1, unbiased running var)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, p_drop, seed, momentum, eps):
        yd = check(y.detach().contiguous(), F32, 'y')
        N, C = yd.shape
        dev = yd.device
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        if training:
            sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
            _hip.call('mgv_colstats', N, C, ptr(yd), C, ptr(sums), *_sw(yd.device))
            mean64 = sums[:C] / N
            var64 = (sums[C:] / N - mean64 * mean64).clamp_min(0.0)
            mean, var = mean64.to(F32), var64.to(F32)
            with torch.no_grad():
                running_mean.mul_(1 - momentum).add_(momentum * mean)
                running_var.mul_(1 - momentum).add_(momentum * (var64 * (N / max(N - 1, 1))).to(F32))
        else:
            mean, var = running_mean.detach().clone(), running_var.detach().clone()
        invstd = torch.rsqrt(var + eps).contiguous()
        mean = mean.contiguous()
        p = float(p_drop) if training else 0.0
        a = torch.empty_like(yd)
        _hip.call('mgv_bn_act_fwd', N, C, ptr(yd), ptr(mean), ptr(invstd), ptr(g), ptr(b), p, int(seed), ptr(a))
        ctx.save_for_backward(yd, mean, invstd, g, b)
        ctx.cfg = (bool(training), p, int(seed))
        return a

    @staticmethod
    def backward(ctx, ga):
        yd, mean, invstd, g, b = ctx.saved_tensors
        training, p, seed = ctx.cfg
        N, C = yd.shape
        ga = check(ga.contiguous(), F32, 'ga')
        dz = torch.empty_like(yd)
        sums = torch.zeros(2 * C, dtype=torch.float64, device=yd.device)
        _hip.call('mgv_bn_act_bwd', N, C, ptr(yd), ptr(mean), ptr(invstd), ptr(g), ptr(b), p, seed, ptr(ga), ptr(dz), ptr(sums), *_sw(yd.device))
        dy = torch.empty_like(yd)
        _hip.call('mgv_bn_bwd_apply', N, C, ptr(yd), ptr(mean), ptr(invstd), ptr(g), ptr(dz), ptr(sums), int(training), ptr(dy))
        return dy, sums[C:].to(F32), sums[:C].to(F32), None, None, None, None, None, None, None


class HeadFn(torch.autograd.Function):
    """clamp(a w^T + b, 0, 1): last Linear of the readout MLP + torch.clamp (dg_ae_model_aig.py:105)."""

    @staticmethod
    def forward(ctx, a, w, b, clamp01):
        ad = check(a.detach().contiguous(), F32, 'a')
        wd, bd = w.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
        N, C = ad.shape
        prob = torch.empty(N, 1, dtype=F32, device=ad.device)
        _hip.call('mgv_readout_head_fwd', N, C, ptr(ad), ptr(wd), ptr(bd), int(bool(clamp01)), ptr(prob))
        ctx.save_for_backward(ad, wd, bd)
        ctx.wshape, ctx.clamp01 = w.shape, int(bool(clamp01))
        return prob

    @staticmethod
    def backward(ctx, gprob):
        ad, wd, bd = ctx.saved_tensors
        N, C = ad.shape
        gp = check(gprob.contiguous().reshape(-1), F32, 'gprob')
        da = torch.empty_like(ad)
        dw = torch.zeros_like(wd)
        db = torch.zeros_like(bd)
        _hip.call('mgv_readout_head_bwd', N, C, ptr(ad), ptr(wd), ptr(bd), ctx.clamp01, ptr(gp), ptr(da), ptr(dw), ptr(db), *_sw(ad.device))
        return da, dw.reshape(ctx.wshape), db, None


class ReadoutMLPFn(torch.autograd.Function):
    """Training-mode readout 64 -> 32 -> 32 -> 1 (arch/mlp.py MLP.forward, dg_ae_model_aig.py:102-106) in a few streaming passes
    (csrc/readout_fused_x3.hip): the same arithmetic as linear() + BnReluDropFn + HeadFn (bf16x3 products, double batch statistics,
    the same dropout masks for the same seeds, the running buffers updated in place), but only y1, y2 [N, 32] are kept between the
    layers; activations, masks and BatchNorm gradients are recomputed in the backward passes."""

    @staticmethod
    def forward(ctx, hf, W1, b1, g1, be1, W2, b2, g2, be2, W3, b3, rm1, rv1, rm2, rv2, p1, p2, seed1, seed2, momentum, eps, clamp01):
        hfd = check(hf.detach().contiguous(), F32, 'hf')
        N, dev = hfd.shape[0], hfd.device
        par = [check(t.detach().contiguous(), F32, n) for t, n in ((W1, 'W1'), (b1, 'b1'), (g1, 'g1'), (be1, 'be1'), (W2, 'W2'), (b2, 'b2'),
                                                                     (g2, 'g2'), (be2, 'be2'), (W3, 'W3'), (b3, 'b3'))]
        W1d, b1d, g1d, be1d, W2d, b2d, g2d, be2d, W3d, b3d = par
        assert W1d.shape == (32, 64) and W2d.shape == (32, 32) and W3d.shape == (1, 32)
        for t in (rm1, rv1, rm2, rv2):
            check(t, F32, 'running buffer')
            assert t.is_contiguous()
        pack = torch.empty(_hip.call_value('mgv_readout_fused_pack_elems'), dtype=torch.bfloat16, device=dev)
        off = 0
        for w, tr in ((W1d, False), (W2d, False), (W2d, True), (W1d, True)):
            off = _pack_into(pack, off, w, tr)
        y1 = torch.empty(N, 32, dtype=F32, device=dev)
        y2 = torch.empty(N, 32, dtype=F32, device=dev)
        stats = torch.empty(128, dtype=F32, device=dev)
        sums = torch.empty(128, dtype=torch.float64, device=dev)
        prob = torch.empty(N, 1, dtype=F32, device=dev)
        ws = workspace(_hip.call_value('mgv_readout_fused_ws_doubles', N), dev, torch.float64)
        _hip.call('mgv_readout_fused_fwd', N, ptr(hfd), ptr(pack), ptr(b1d), ptr(g1d), ptr(be1d), ptr(rm1), ptr(rv1), ptr(b2d), ptr(g2d),
                  ptr(be2d), ptr(rm2), ptr(rv2), ptr(W3d), ptr(b3d), float(p1), float(p2), int(seed1), int(seed2), float(momentum),
                  1 - momentum, float(eps), int(bool(clamp01)), ptr(y1), ptr(y2), ptr(stats), ptr(sums), ptr(prob), ptr(ws), ws.numel())
        ctx.save_for_backward(hfd, y1, y2, stats, pack, g1d, be1d, g2d, be2d, W3d, b3d)
        ctx.cfg = (float(p1), float(p2), int(seed1), int(seed2), int(bool(clamp01)))
        return prob

    @staticmethod
    def backward(ctx, gprob):
        hfd, y1, y2, stats, pack, g1, be1, g2, be2, W3, b3 = ctx.saved_tensors
        p1, p2, seed1, seed2, clamp01 = ctx.cfg
        N, dev = hfd.shape[0], hfd.device
        gp = check(gprob.contiguous().reshape(-1), F32, 'gprob')
        dhf = torch.empty_like(hfd)
        grads = torch.empty(_hip.call_value('mgv_readout_fused_grad_floats'), dtype=F32, device=dev)
        sums = torch.empty(128, dtype=torch.float64, device=dev)
        ws = workspace(_hip.call_value('mgv_readout_fused_ws_doubles', N), dev, torch.float64)
        _hip.call('mgv_readout_fused_bwd', N, ptr(hfd), ptr(y1), ptr(y2), ptr(stats), ptr(gp), ptr(pack), ptr(g1), ptr(be1), ptr(g2), ptr(be2),
                  ptr(W3), ptr(b3), p1, p2, seed1, seed2, clamp01, ptr(dhf), ptr(grads), ptr(sums), ptr(ws), ws.numel())
        sizes = (32 * 64, 32, 32, 32, 32 * 32, 32, 32, 32, 32, 1)
        dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3 = torch.split(grads, sizes)
        return (dhf, dW1.view(32, 64), db1, dg1, dbe1, dW2.view(32, 32), db2, dg2, dbe2, dW3.view(1, 32), db3) + (None,) * 11


# ------------------------------------------------------------------------------------------------
# VAE sampler + KL
# ------------------------------------------------------------------------------------------------
class ReparamFn(torch.autograd.Function):
    """z = mu + exp(logstd) * eps and klsum = sum(1 + 2 logstd - mu^2 - exp(logstd)^2)
    (digvae_model.py:138-141, trainer.py:146-147)."""

    @staticmethod
    def forward(ctx, mu, logstd, eps, seed):
        mud, lsd = check(mu.detach().contiguous(), F32, 'mu'), check(logstd.detach().contiguous(), F32, 'logstd')
        n = mud.numel()
        z = torch.empty_like(mud)
        kl = torch.zeros(1, dtype=torch.float64, device=mud.device)
        if eps is None:
            eps_used = torch.empty_like(mud)
            _hip.call('mgv_reparam_fwd', n, ptr(mud), ptr(lsd), None, int(seed), ptr(eps_used), ptr(z), ptr(kl))
        else:
            eps_used = check(eps.detach().contiguous(), F32, 'eps')
            _hip.call('mgv_reparam_fwd', n, ptr(mud), ptr(lsd), ptr(eps_used), 0, None, ptr(z), ptr(kl))
        ctx.save_for_backward(mud, lsd, eps_used)
        return z, kl[0].to(F32)

    @staticmethod
    def backward(ctx, gz, gkl):
        mud, lsd, eps = ctx.saved_tensors
        dmu, dls = torch.empty_like(mud), torch.empty_like(mud)
        gzc = gz.contiguous() if gz is not None else None
        gk = gkl.detach().to(F32).reshape(1).contiguous() if gkl is not None else None
        _hip.call('mgv_reparam_bwd', mud.numel(), ptr(mud), ptr(lsd), ptr(eps), ptr(gzc), ptr(gk), 1.0, ptr(dmu), ptr(dls))
        return dmu, dls, None, None


# ------------------------------------------------------------------------------------------------
# variational link heads on st = hs_decompose(hs): fc_{s,t}_{mu,logstd}, the sample and the KL sums (digvae_model.py:134-142,
# trainer.py:145-148) — one launch forward, one backward (csrc/var_head_x3.hip), or composed from linear + ReparamFn
# ------------------------------------------------------------------------------------------------
# MGV_VAR_HEAD_FUSED=0 forces the composed route for a same-process A/B: tests flip this flag
VAR_HEAD_FUSED = os.environ.get('MGV_VAR_HEAD_FUSED', '1') != '0'


def _var_head_ws(H, N, backward, device):
    return workspace(_hip.call_value('mgv_var_head_x3_ws_floats', H, N, int(backward)), device)


def _var_head_packs(heads):
    """Per half: Wp [2H, H] = fc_mu.weight over fc_logstd.weight, bp [2H] likewise.  `heads` = (Ws_mu, bs_mu, Ws_ls, bs_ls, Wt_mu,
    bt_mu, Wt_ls, bt_ls)."""
    out = []
    for Wm, bm, Wl, bl in (heads[:4], heads[4:]):
        out.append((torch.cat([check(Wm.detach().contiguous(), F32, 'W_mu'), check(Wl.detach().contiguous(), F32, 'W_logstd')]),
                    torch.cat([check(bm.detach().contiguous(), F32, 'b_mu'), check(bl.detach().contiguous(), F32, 'b_logstd')])))
    return out


def _var_head_fwd(st, Wp_b, packs, eps, seed, sample, want_ml=False):
    N, H = st.shape[0], st.shape[1] // 2
    z = torch.empty(N, 2 * H, dtype=F32, device=st.device)
    ml = torch.empty(N, 4 * H, dtype=F32, device=st.device) if want_ml else None
    kl = torch.zeros(2, dtype=torch.float64, device=st.device)
    ws = _var_head_ws(H, N, False, st.device)
    _hip.call('mgv_var_head_fwd_x3', H, N, ptr(st), st.stride(0), ptr(packs[0]), ptr(packs[1]), ptr(Wp_b[0][1]), ptr(Wp_b[1][1]),
              ptr(eps), 0 if eps is None else eps.stride(0), int(seed), int(bool(sample)), ptr(z), 2 * H, ptr(ml), 4 * H, ptr(kl),
              ptr(ws), ws.numel())
    return z, kl, ml


class VarHeadFn(torch.autograd.Function):
    """(z [N, 2H], klsum [2]) of st [N, 2H] = [s | t] under the eight head parameters: per half h, [mu | logstd] = X_h Wp_h^T + bp_h,
    z = mu + exp(logstd) eps (sample) or mu, klsum[h] = sum(1 + 2 logstd - mu^2 - exp(logstd)^2).  eps [N, 2H] = [eps_s | eps_t] or
    None: the kernel draws element r * H + c of seed (s) / seed + 1 (t), as DirectedGVAE.sample.  Nothing but st is kept for the
    backward, which recomputes the heads and the noise."""

    @staticmethod
    def forward(ctx, st, Ws_mu, bs_mu, Ws_ls, bs_ls, Wt_mu, bt_mu, Wt_ls, bt_ls, eps, seed, sample):
        std = _rowmajor(st.detach())
        if std.dtype != F32 or not std.is_cuda:
            raise HipLibraryError('st must be an fp32 GPU matrix')
        epsd = _rowmajor(eps.detach()) if eps is not None else None
        Wp_b = _var_head_packs((Ws_mu, bs_mu, Ws_ls, bs_ls, Wt_mu, bt_mu, Wt_ls, bt_ls))
        packs = [linear_wpack(W) for W, _ in Wp_b]
        z, kl, _ = _var_head_fwd(std, Wp_b, packs, epsd, seed, sample)
        ctx.save_for_backward(std, epsd, Wp_b[0][0], Wp_b[0][1], Wp_b[1][0], Wp_b[1][1], *packs)
        ctx.seed, ctx.sample = int(seed), bool(sample)
        ctx.set_materialize_grads(False)
        return z, kl.to(F32)

    @staticmethod
    def backward(ctx, gz, gkl):
        st, eps, Wps, bps, Wpt, bpt, pack_s, pack_t = ctx.saved_tensors
        N, H = st.shape[0], st.shape[1] // 2
        gz = _rowmajor(gz.detach()) if gz is not None else None
        gk = gkl.detach().to(F32).reshape(2).contiguous() if gkl is not None else None
        tpacks = []
        for W in (Wps, Wpt):
            tp = torch.empty(2 * W.numel(), dtype=torch.bfloat16, device=W.device)
            _pack_into(tp, 0, W, True)
            tpacks.append(tp)
        dst = torch.empty(N, 2 * H, dtype=F32, device=st.device)
        dWs, dWt = torch.zeros_like(Wps), torch.zeros_like(Wpt)
        dbs, dbt = torch.zeros_like(bps), torch.zeros_like(bpt)
        ws = _var_head_ws(H, N, True, st.device)
        _hip.call('mgv_var_head_bwd_x3', H, N, ptr(st), st.stride(0), ptr(pack_s), ptr(pack_t), ptr(tpacks[0]), ptr(tpacks[1]), ptr(bps), ptr(bpt),
                  ptr(eps), 0 if eps is None else eps.stride(0), ctx.seed, int(ctx.sample), ptr(gz), 0 if gz is None else gz.stride(0), ptr(gk),
                  ptr(dst), 2 * H, ptr(dWs), ptr(dWt), ptr(dbs), ptr(dbt), ptr(ws), ws.numel())
        return dst, dWs[:H], dbs[:H], dWs[H:], dbs[H:], dWt[:H], dbt[:H], dWt[H:], dbt[H:], None, None, None


def var_head_fused(H):
    """Whether var_head takes the fused route at width H (csrc/mgv_launch.h X3Widths, bf16x3 mode, MGV_VAR_HEAD_FUSED)."""
    return VAR_HEAD_FUSED and use_x3(H)


def var_head(st, heads, eps=None, seed=0, sample=True):
    """(z [N, 2H], klsum [2]) — VarHeadFn where var_head_fused(H) holds, else the same function composed from today's operators
    (four ops.linear and two ReparamFn: PRECISION = f32, H = 16 / 128, MGV_VAR_HEAD_FUSED=0).  `heads` as _var_head_packs takes them."""
    H = st.shape[1] // 2
    if st.shape[0] > 0 and var_head_fused(H):
        return VarHeadFn.apply(st, *heads, eps, seed, sample)
    s, t = st[:, :H].contiguous(), st[:, H:].contiguous()          # (the plain Linear takes contiguous rows)
    zs, kls = [], []
    for x, (Wm, bm, Wl, bl), e, sd in ((s, heads[:4], None if eps is None else eps[:, :H], seed), (t, heads[4:], None if eps is None else eps[:, H:], seed + 1)):
        mu, ls = linear(x, Wm, bm), linear(x, Wl, bl)
        z, kl = ReparamFn.apply(mu, ls, e, sd)
        zs.append(z if sample else mu)
        kls.append(kl)
    return torch.cat(zs, dim=1), torch.stack(kls)


def var_head_latent(st, heads):
    """(mu_s, logstd_s, mu_t, logstd_t) of st under the heads, without gradients: the fused forward's ML rows, or four ops.linear."""
    H = st.shape[1] // 2
    with torch.no_grad():
        if st.shape[0] > 0 and var_head_fused(H):
            std = _rowmajor(st.detach())
            Wp_b = _var_head_packs(heads)
            ml = _var_head_fwd(std, Wp_b, [linear_wpack(W) for W, _ in Wp_b], None, 0, False, want_ml=True)[2]
            return ml[:, :H], ml[:, H:2 * H], ml[:, 2 * H:3 * H], ml[:, 3 * H:]
        s, t = st[:, :H].contiguous(), st[:, H:].contiguous()
        return (linear(s, heads[0], heads[1]), linear(s, heads[2], heads[3]), linear(t, heads[4], heads[5]), linear(t, heads[6], heads[7]))


# ------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, grad_scale, step):
    for n, t in (('param', param), ('grad', grad), ('exp_avg', exp_avg), ('exp_avg_sq', exp_avg_sq)):
        check(t, F32, n)
    _hip.call('mgv_adam_step', param.numel(), ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), float(lr),
              float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale), int(step))


# ------------------------------------------------------------------------------------------------
# the analysis surface lives in pairs / similarity / metrics (none of them imports this module); the documented public names are
# re-bound here.  Their underscored helpers are not: patch those in their home module.
# ------------------------------------------------------------------------------------------------
from .pairs import (FANIN_MAX, PROFILE_MAX_EDGES, PairScoresFn, counts_above, dense_scores, fanin_decode, fanin_edges,  # noqa: E402,F401
                    pair_profile, pair_scores, pair_scores_at, pair_select, pair_topk, reconstruct_edges, reconstruction_counts,
                    reconstruction_curve)
from .similarity import (SIM_THRESHOLD, class_table, components, cross_classes, cross_mutual, cross_pairs,  # noqa: E402,F401
                         cross_profile, cross_threshold_for, cross_topk, row_unit, sim_at, sim_classes, sim_pairs, sim_profile, sim_threshold_for, sim_topk,
                         threshold_search)
from .metrics import (CONCORD_MAX_GAPS, CONCORD_TILE, FANIN_RECORD, LINK_RECORD_WORDS, MIN_GAP, FaninRecovery, LinkRanks,  # noqa: E402,F401
                      RankLists, RankMetrics, concord_counts, fanin_recovery, function_accuracy, link_auc_ap, link_rank_filter, link_rank_lists, link_ranks, link_record,
                      pair_rank_counts, pair_segments, rank_metrics, read_link_records, segment_table, true_fanin_lists)
