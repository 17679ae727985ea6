"""The device builder of a GraphPlan's tables (graph_plan.py): the callers of csrc/plan_build.hip and csrc/radix_sort.hip — degree
histogram + scan + cursor fill + per-list sort for the CSRs, a stable counting sort by (level, slot) for the buckets (SURVEY.md §8f
row 1), keys + one radix sort + runs + exact check for a refinement stage.  Same functions, same arrays as plan_torch.py.  A function
that returns DECLINED leaves its table to the torch builder; GraphPlan states where that happens.
"""
import ctypes

import torch

from . import _hip
from ._hip import ptr
from .plan_torch import HEAVY_ROW, NO_GATE, ROW_INTS, SEED, colour_lists_equal, lists, owner, stage

DECLINED = False
COUNT_SORT_KEYS = 8192      # mgv_count_sort_i32 takes at most this many distinct keys


def _ints(n, dev):
    """Uninitialised int32 [n], cut from an allocation of at least one element (n = 0 included: never a tensor without storage)."""
    return torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]


def _count_sort(n, keys, K, order):
    """Stable counting sort of n int32 keys in [0, K) (negative keys are left out) into `order`; -> key_start int32 [K + 1]."""
    key_start = torch.empty(K + 1, dtype=torch.int32, device=keys.device)
    n_s = _hip.call_value('mgv_count_sort_scratch_ints', n, K)
    scratch = torch.empty(n_s, dtype=torch.int32, device=keys.device)
    _hip.call('mgv_count_sort_i32', n, ptr(keys), K, ptr(order), ptr(key_start), ptr(scratch), n_s)
    return key_start


def csr(src, dst, N):
    """The plan's CSR fields from contiguous int64 edge ends, plus `_status` (read lazily, with the level checks: one host round trip
    per batch) and `_keep` (the launches' inputs).  The arrays are safe to launch on before the status is read: the CSR kernels skip
    out-of-range edges and zero the unfilled tail, so every stored id lies in [0, N)."""
    E, dev = int(src.numel()), src.device
    i32 = dict(dtype=torch.int32, device=dev)
    f = dict(in_ptr=torch.empty(N + 1, **i32), out_ptr=torch.empty(N + 1, **i32), in_src=_ints(E, dev), in_dst=_ints(E, dev),
             out_dst=_ints(E, dev), out_slot=_ints(E, dev))
    n_s = _hip.call_value('mgv_plan_csr_scratch_ints', N, E)
    scratch = torch.empty(n_s, **i32)
    status = torch.empty(2, **i32)
    _hip.call('mgv_plan_csr', N, E, ptr(src), ptr(dst), ptr(f['in_ptr']), ptr(f['in_src']), ptr(f['in_dst']), ptr(f['out_ptr']),
              ptr(f['out_dst']), ptr(f['out_slot']), None, None, ptr(scratch), n_s, ptr(status))
    if N == 0 and E > 0:
        raise ValueError('edge_index holds node ids outside [0, num_nodes)')
    return dict(f, _status=status, _keep=(src, dst))


def asap_levels(g):
    """Frontier relaxation over the out-CSR.  Raises on a cycle."""
    N, dev = g.N, g.in_ptr.device
    level = torch.zeros(max(N, 1), dtype=torch.int32, device=dev)[:N]
    if N == 0:
        return level.long()
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    rounds = 512
    while True:
        scratch = torch.empty(3 * N + rounds + 2, dtype=torch.int32, device=dev)
        _hip.call('mgv_plan_levels', N, ptr(g.in_ptr), ptr(g.out_ptr), ptr(g.out_dst), ptr(level), rounds, ptr(scratch),
                  scratch.numel(), ptr(done))
        if int(done.item()) == N:
            return level.long()
        if rounds >= N + 1:              # more rounds than nodes cannot help: some node never lost its last pending parent
            raise ValueError('edge_index is not a DAG (%d of %d nodes levelised)' % (int(done.item()), N))
        rounds = min(rounds * 8, N + 1)


def set_levels(g, gate, forward_level, gate_ids):
    """The level fields of a plan (GraphPlan.set_levels), three host round trips; DECLINED with more (level, slot) keys than the
    counting sort takes."""
    N, E, dev, T = g.N, g.E, g.in_ptr.device, len(gate_ids)
    i32 = dict(dtype=torch.int32, device=dev)
    gt = gate.reshape(-1).to(dev, torch.float32).contiguous()
    lv = forward_level.reshape(-1).to(dev, torch.int64).contiguous()
    if gt.numel() != N or lv.numel() != N:
        raise ValueError('gate / forward_level must have one entry per node')
    tab = (ctypes.c_uint8 * 256)(*([NO_GATE] * 256))
    for s_, gid in enumerate(gate_ids):
        tab[int(gid)] = s_
    gslot = torch.empty(N, dtype=torch.uint8, device=dev)
    level = torch.empty(N, **i32)
    key = torch.empty(max(N, 1), **i32)
    flags = torch.zeros(2, **i32)                       # [max level, level-order violation]
    _hip.call('mgv_plan_keys', N, T, ptr(gt), ptr(lv), tab, ptr(gslot), ptr(level), ptr(key), ptr(flags))
    _hip.call('mgv_plan_check_levels', E, ptr(g.in_src), ptr(g.in_dst), ptr(gslot), ptr(level), ptr(flags[1:]))
    maxlevel, bad = (int(v) for v in flags.tolist())    # the batch's first host round trip
    if bad:
        raise ValueError('forward_level is not a topological levelisation of edge_index')
    L = maxlevel + 1 if N > 0 else 0
    K = max(L, 1) * T
    if K > COUNT_SORT_KEYS:
        return DECLINED
    order = torch.empty(max(N, 1), **i32)
    key_start = _count_sort(N, key, K, order)
    small = torch.empty(2 * (K + 1) + K // 2048 + 64 + max(L, 1) + 1, **i32)
    ntile, tile_first, scan_s = small[:K + 1], small[K + 1:2 * (K + 1)], small[2 * (K + 1):2 * (K + 1) + K // 2048 + 64]
    ltp_dev = small[2 * (K + 1) + K // 2048 + 64:]
    _hip.call('mgv_plan_tile_counts', K, ptr(key_start), ptr(ntile), ptr(tile_first), ptr(scan_s))
    n_active, num_tiles = int(key_start[K].item()), int(tile_first[K].item())         # second round trip
    f = dict(gslot=gslot, level=level, num_levels=L, order=order[:n_active], order_span=torch.empty(max(n_active, 1), 4, **i32)[:n_active],
             tile_start=_ints(num_tiles, dev), tile_count=_ints(num_tiles, dev), tile_slot=_ints(num_tiles, dev))
    _hip.call('mgv_plan_tiles', K, T, max(L, 1), n_active, ptr(key_start), ptr(tile_first), ptr(f['order']), ptr(g.in_ptr), ptr(g.out_ptr),
              ptr(f['tile_start']), ptr(f['tile_count']), ptr(f['tile_slot']), ptr(f['order_span']), ptr(ltp_dev))
    # tiles grouped by slot (stable), for the per-slot weight-gradient pass of the backward sweep
    f['slot_tiles'] = _ints(num_tiles, dev)
    slot_start = _count_sort(num_tiles, f['tile_slot'], T, f['slot_tiles'])
    host = torch.cat([ltp_dev[:max(L, 1) + 1], slot_start]).tolist()  # third (last) round trip
    return dict(f, level_tile_ptr=host[:max(L, 1) + 1], slot_tile_ptr=host[max(L, 1) + 1:], num_tiles=num_tiles, n_active=n_active,
                num_slots=T)


def order_rows(g, n, order, order_span, gslot):
    dev = order.device
    rows = torch.empty(max(n, 1), ROW_INTS, dtype=torch.int32, device=dev)[:n]
    edge_lists = (g.in_src, g.out_dst, g.out_slot)
    if g.E == 0:                         # (empty tensors have no address, and the entry insists on its lists: every span is empty)
        edge_lists = (torch.zeros(1, dtype=torch.int32, device=dev),) * 3
    _hip.call('mgv_plan_order_rows', n, ptr(order), ptr(g.in_ptr), ptr(edge_lists[0]), ptr(g.out_ptr), ptr(edge_lists[1]),
              ptr(edge_lists[2]), ptr(gslot), ptr(rows))
    return rows


def first_stage_pairs(g, xcls, max_classes):
    """GraphPlan.first_stage_classes by the pair kernels, which number the (in-degree, class) table in one pass (ids ascending in the
    pair code, every id present); DECLINED when a degree is above 255."""
    N, dev = g.N, g.in_ptr.device
    if N == 0:
        return None
    i32 = dict(dtype=torch.int32, device=dev)
    work = torch.empty(2 * 65537 + 64, **i32)
    cid = torch.empty(N, **i32)
    cls_deg = torch.zeros(65536, **i32)
    cls_x = torch.zeros(65536, dtype=torch.uint8, device=dev)
    status = torch.empty(1, **i32)
    xc = xcls.contiguous()
    _hip.call('mgv_plan_pairs', N, ptr(g.in_ptr), ptr(xc), ptr(work), ptr(work[65537:]), ptr(work[2 * 65537:]), ptr(cid), ptr(cls_deg),
              ptr(cls_x), ptr(status))
    C, bad = int(work[65537 + 65536].item()), int(status.item())
    if bad:
        return DECLINED
    if not 0 < C <= max_classes:
        return None
    p = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    p[1:] = torch.cumsum(cls_deg[:C].long(), 0)             # C entries: a dozen
    idx = torch.zeros(max(int(p[-1].item()), 1), **i32)
    return (cid, C, p.to(torch.int32).contiguous(), idx, cls_x[:C].contiguous())


def _stage1_pairs(g, xcls):
    """The first refinement stage without a sort: every node starts from the same state, so its colour after the first half round
    is its (in-degree, feature class) pair.  None when that table does not apply (a degree above 255, or too many pairs)."""
    return first_stage_pairs(g, xcls, 1 << 15) or None


def key_bits(N, Cp):
    """Bits of the grouping key a refinement stage sorts on: enough that two of the colours to expect (at most 1,024 per previous
    colour, at most N) share a key with probability below 2^-20 — early stages sort 40-odd bits instead of 63."""
    expect = min(N, int(Cp) * 1024)
    return min(63, max(24, 2 * max(expect, 2).bit_length() + 20))


def sort_by_key(keys, n, K):
    """(order int32 [n], members per key int32 [K]) of a STABLE sort of n int32 keys in [0, K): the counting sort of the tile
    builder while its (key, block) histogram stays small, else a radix sort over the keys' bits."""
    i32 = dict(dtype=torch.int32, device=keys.device)
    if n == 0:
        return torch.zeros(0, **i32), torch.zeros(K, **i32)
    order = torch.empty(n, **i32)
    if K <= COUNT_SORT_KEYS and K * ((n + 1023) // 1024) <= 4 * n + 65536:
        ks = _count_sort(n, keys, K, order)
        return order, ks[1:] - ks[:-1]
    sk = torch.empty(n, **i32)
    t_i = _hip.call_value('mgv_sort_pairs_temp_ints', 4, n)
    temp = torch.empty(t_i, **i32)
    _hip.call('mgv_sort_pairs', 4, n, ptr(keys), ptr(sk), ptr(order), max((K - 1).bit_length(), 1), ptr(temp), t_i)
    counts = torch.empty(K, **i32)
    _hip.call('mgv_sorted_key_counts', n, ptr(sk), K, ptr(counts))
    return order, counts


def class_sum_levels(counts, C, seg=64):
    """GraphPlan.class_sum_levels' tables from the members per colour (int32 [C]): per level one scan pass (segments, members,
    partial rows, colours going on), one read-back of the four totals, one fill pass."""
    i32 = dict(dtype=torch.int32, device=counts.device)
    counts0 = counts
    levels = []
    gid, G = None, C
    base, src_row = C, 0
    while True:
        w_i = _hip.call_value('mgv_seg_level_work_ints', G)
        work = torch.empty(w_i, **i32)
        _hip.call('mgv_seg_level_scan', G, ptr(counts), seg, ptr(work), w_i)
        total, _, n_partial, g_next = work[:4].tolist()
        sp = torch.empty(total + 1, **i32)
        out_row = None if (n_partial == 0 and G == C and base == C) else torch.empty(total, **i32)
        gid_n = torch.empty(g_next, **i32) if g_next else None
        counts_n = torch.empty(g_next, **i32) if g_next else None
        _hip.call('mgv_seg_level_fill', G, total, ptr(gid), seg, base, ptr(work), ptr(sp), ptr(out_row), ptr(gid_n), ptr(counts_n))
        levels.append((total, sp, out_row, src_row))
        if n_partial == 0:
            return dict(C=C, rows=base, levels=levels, counts=counts0)
        gid, counts, G = gid_n, counts_n, g_next
        src_row, base = base, base + n_partial


def colour_key_and_check(g, xcls, first_stage_is_pairs=False):
    """(key, check) of a refinement stage on a device plan, for the stage loop below and for plan_torch.quotient_stages: the grouping
    key by mgv_colour_keys (at stage 1, with `first_stage_is_pairs`, the pair table's id: that stage IS the (in-degree, class)
    grouping) and the exact check by mgv_colour_check, with the sort-based check behind it for the lists longer than the kernel
    compares pairwise.  Colours and representatives as int32 or int64."""
    shared = {}                              # the previous colours as int32: written by key, read by check

    def key(t, rev, prev, Cp, f):
        p, idx = lists(g, rev)
        shared['prev32'] = prev32 = prev.to(torch.int32)
        pairs = _stage1_pairs(g, xcls) if (t == 1 and first_stage_is_pairs) else None
        if pairs is not None:
            return pairs[0].long()
        mix = torch.empty(g.N, dtype=torch.int64, device=p.device)
        _hip.call('mgv_colour_keys', g.N, ptr(p), ptr(idx), ptr(prev32), ptr(f), Cp + 1, ptr(xcls), key_bits(g.N, Cp), ptr(mix))
        return mix

    def check(rev, prev, Cp, inv, rep):
        p, idx = lists(g, rev)
        flags = torch.zeros(2, dtype=torch.int32, device=p.device)
        inv32, rep32 = inv.to(torch.int32), rep.to(torch.int32)      # (named: a temporary would be freed, and its memory reused, before the launch)
        _hip.call('mgv_colour_check', g.N, ptr(p), ptr(idx), ptr(shared['prev32']), ptr(xcls), ptr(inv32), ptr(rep32), ptr(flags))
        bad, n_long = flags.tolist()
        if bad or not n_long:
            return not bad
        return colour_lists_equal(p.long(), idx.long(), owner(g, rev), prev.long(), inv.long(), rep.long(), xcls.long(), Cp)
    return key, check


def quotient_stages(g, xcls, max_stages, admits, goes_on):
    """The stages of GraphPlan.quotient with every table built by the plan builder's kernels: per stage the grouping keys, ONE radix
    sort of them (the permutation as int32), runs -> colours / representatives, the exact check, the representatives' lists in
    previous colours, and the segment tables of the colour-level sums (stable sort by previous colour + per-level scans).  Host
    read-backs per stage: the colour count, the check's flags, the list length, and four totals per table level.  Same numbering,
    same tables as plan_torch.quotient_stages (GPU test, field by field); `admits` / `goes_on` as there."""
    N, dev = g.N, g.in_ptr.device
    i32 = dict(dtype=torch.int32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    stages = []
    key, check = colour_key_and_check(g, xcls)
    prev32, Cp = torch.zeros(N, **i32), 1
    t_sort = _hip.call_value('mgv_sort_pairs_temp_ints', 8, N)
    n_grp = 2 * N + N // 2048 + 66
    last = None
    for t_ in range(1, max_stages + 1):
        rev = t_ % 2 == 0
        p, idx = lists(g, rev)
        f = torch.randint(1, 1 << 62, (3, Cp + 1), generator=gen, **i64)
        pairs = _stage1_pairs(g, xcls) if t_ == 1 else None
        if pairs is not None:
            # stage 1 = the (in-degree, class) table (exact by construction: no keys, no sort, no check); every list names the one
            # shared start row
            cid, C, rptr, _, xrep = pairs
            if not admits(C):
                break
            dr = rptr[1:] - rptr[:-1]
            n_ent = int(rptr[-1].item())
            own32 = torch.zeros(C, **i32)
            ent = torch.zeros(max(n_ent, 1), **i32)
            row = torch.repeat_interleave(torch.arange(C, **i32), dr.long()) if n_ent else torch.zeros(1, **i32)
            heavy = torch.nonzero(dr > HEAVY_ROW).reshape(-1).to(torch.int32)
            last = None
        else:
            mix, skey = key(t_, rev, prev32, Cp, f), torch.empty(N, **i64)
            by_colour, temp = torch.empty(N, **i32), torch.empty(t_sort, **i32)
            _hip.call('mgv_sort_pairs', 8, N, ptr(mix), ptr(skey), ptr(by_colour), key_bits(N, Cp), ptr(temp), t_sort)
            cid, starts, rep = torch.empty(N, **i32), torch.empty(N + 1, **i32), torch.empty(N, **i32)
            n_colours = torch.zeros(1, **i32)
            scratch = torch.empty(n_grp, **i32)
            _hip.call('mgv_colour_groups', N, ptr(skey), ptr(by_colour), ptr(cid), ptr(starts), ptr(rep), ptr(n_colours), ptr(scratch), n_grp)
            C = int(n_colours.item())
            if not admits(C) or not check(rev, prev32, Cp, cid, rep[:C]):
                break
            small = torch.empty(C + 2, **i32)                   # rptr [C + 1], then the heavy-row count
            rptr, own32, xrep = small[:C + 1], torch.empty(C, **i32), torch.empty(C, dtype=torch.uint8, device=dev)
            n_rr = C + C // 2048 + 66
            scratch = torch.empty(n_rr, **i32)
            _hip.call('mgv_colour_rep_rows', C, ptr(rep), ptr(p), ptr(prev32), ptr(xcls), HEAVY_ROW, ptr(rptr), ptr(own32), ptr(xrep),
                      ptr(small[C + 1:]), ptr(scratch), n_rr)
            n_ent, n_heavy = small[C:].tolist()
            ent, row = torch.empty(max(n_ent, 1), **i32), torch.empty(max(n_ent, 1), **i32)
            if n_ent:
                _hip.call('mgv_colour_rep_lists', C, ptr(rep), ptr(p), ptr(idx), ptr(prev32), ptr(rptr), ptr(ent), ptr(row))
            else:
                ent.zero_()
            heavy = (torch.nonzero((rptr[1:] - rptr[:-1]) > HEAVY_ROW).reshape(-1).to(torch.int32) if n_heavy
                     else torch.zeros(0, **i32))
            last = (by_colour, starts)
        # the stable sorts by previous colour and the segment tables
        own_o, own_counts = sort_by_key(own32, C, Cp)
        ent_o, ent_counts = sort_by_key(ent, n_ent, Cp)
        stages.append(stage(C, cid, rev, rptr, (ent + C) if n_ent else ent, ent, own32.long(), own32, xrep, heavy,
                            own_o, class_sum_levels(own_counts, Cp), row.index_select(0, ent_o) if n_ent else ent,
                            class_sum_levels(ent_counts, Cp)))
        prev32, Cp = cid, C
        if not goes_on(C):
            break                        # colours multiply per half round: the next one would not qualify
    if stages:
        C = stages[-1]['C']
        if last is None:                 # (the pair-table stage is the last one: its members by colour through the counting sort)
            by_colour, counts = sort_by_key(stages[-1]['cid'], N, C)
        else:
            by_colour, counts = last[0], last[1][1:C + 1] - last[1][:C]
        stages[-1]['sum_levels'] = (by_colour, class_sum_levels(counts, C))
    return stages


def seg_entries(g, reverse, order, n_seg, seg_ptr):
    """GraphPlan.seg_entries by mgv_seg_entries."""
    p, idx = lists(g, reverse)
    n, dev = int(order.numel()), order.device
    cap = n + g.E                            # every node once and every list once
    entries, esp = _ints(cap, dev), torch.zeros(n_seg + 1, dtype=torch.int32, device=dev)
    n_s = _hip.call_value('mgv_seg_entries_scratch_ints', n)
    scratch = torch.empty(max(n_s, 1), dtype=torch.int32, device=dev)
    _hip.call('mgv_seg_entries', n, ptr(order), ptr(p), ptr(idx), n_seg, ptr(seg_ptr), cap, ptr(entries), ptr(esp), ptr(scratch), n_s)
    return entries, esp
