"""The torch builder of a GraphPlan's tables (graph_plan.py): stable sorts and scans, plain functions of tensors on any device — the
plans on CPU tensors and, with `MGV_PLAN=torch`, the GPU tests' cross-check of plan_device.py.  Nothing here calls the native library
or caches.  What both builders share is stated here once: `Graph`, `owner`, `stage`, `colour_lists_equal`.
"""
import functools
from collections import namedtuple

import torch

TILE = 64
NO_GATE = 255
HEAVY_ROW = 64      # csrc/struct_stage_x3_common.h: kHeavyRow
ROW_INTS = 32       # func_level_x3_common.h kRowInts
ROW_OUT = 8
SEED = 0x5EED5      # of the per-colour random values the grouping keys are summed from

# The two CSRs of a plan, as both builders read them (GraphPlan's docstring has the fields).
Graph = namedtuple('Graph', 'N E in_ptr in_src in_dst out_ptr out_dst out_slot')


def lists(g, reverse):
    """(ptr, idx) of the neighbours a node sums over: in-neighbours, or out-neighbours when the edges are flipped."""
    return (g.out_ptr, g.out_dst) if reverse else (g.in_ptr, g.in_src)


def owner(g, reverse):
    """The node (int64) whose list each slot of `lists(g, reverse)` belongs to."""
    if not reverse:
        return g.in_dst.long()
    p = g.out_ptr.long()
    return torch.repeat_interleave(torch.arange(g.N, dtype=torch.int64, device=p.device), p[1:] - p[:-1])


def _ptr(index, n):
    cnt = torch.bincount(index, minlength=n)
    p = torch.zeros(n + 1, dtype=torch.int64, device=index.device)
    p[1:] = torch.cumsum(cnt, 0)
    return p.to(torch.int32).contiguous()


def csr(src, dst, N):
    """The plan's CSR fields from int64 edge ends: stable sorts by destination / source."""
    E = int(src.numel())
    perm_in = torch.sort(dst, stable=True).indices
    perm_out = torch.sort(src, stable=True).indices
    inv_in = torch.empty(E, dtype=torch.long, device=src.device)
    inv_in[perm_in] = torch.arange(E, device=src.device)
    return dict(in_src=src[perm_in].to(torch.int32).contiguous(), out_dst=dst[perm_out].to(torch.int32).contiguous(),
                out_slot=inv_in[perm_out].to(torch.int32).contiguous(), in_ptr=_ptr(dst, N), out_ptr=_ptr(src, N),
                in_dst=dst[perm_in].to(torch.int32).contiguous(),   # destination of each in-CSR slot
                perm_in=perm_in)


def asap_levels(g):
    from .parser import forward_levels
    ei = torch.stack([g.in_src.long(), g.in_dst.long()]).cpu().numpy()
    return torch.from_numpy(forward_levels(ei, g.N)).to(g.in_ptr.device)


def set_levels(g, gate, forward_level, gate_ids):
    """The level fields of a plan (GraphPlan.set_levels): buckets by a stable sort of (level, slot), tiles by scans."""
    dev, N = g.in_ptr.device, g.N
    f = {}
    gt = gate.reshape(-1).to(dev).long()
    lv = forward_level.reshape(-1).to(dev).long()
    if gt.numel() != N or lv.numel() != N:
        raise ValueError('gate / forward_level must have one entry per node')
    slot_of = torch.full((256,), NO_GATE, dtype=torch.long, device=dev)
    for s, gid in enumerate(gate_ids):
        slot_of[int(gid)] = s
    gslot = slot_of[gt.clamp(0, 255)]
    active = (lv >= 1) & (gslot != NO_GATE)
    gslot = torch.where(active, gslot, torch.full_like(gslot, NO_GATE))
    f['gslot'] = gslot.to(torch.uint8).contiguous()
    f['level'] = lv.to(torch.int32).contiguous()
    f['num_levels'] = L = int(lv.max().item()) + 1 if N > 0 else 0
    nodes = torch.nonzero(active).reshape(-1)
    # every source of an updated node must sit on a strictly lower level: the kernels update a
    # level in place, the reference reads the pre-level state (dg_ae_model_aig.py:97)
    if g.E > 0:
        d = g.in_dst.long()
        s = g.in_src.long()
        bad = active[d] & (lv[s] >= lv[d])
        if bool(bad.any()):
            raise ValueError('forward_level is not a topological levelisation of edge_index')
    T = len(gate_ids)
    key = lv[nodes] * T + gslot[nodes]
    o = torch.sort(key, stable=True)
    f['order'] = nodes[o.indices].to(torch.int32).contiguous()
    # CSR spans in sweep order {in0, in1, out0, out1}: a tile reaches its edge lists with one load per row
    on = nodes[o.indices]
    f['order_span'] = torch.stack([g.in_ptr[on], g.in_ptr[on + 1], g.out_ptr[on], g.out_ptr[on + 1]], 1).to(torch.int32).contiguous()
    keys, counts = torch.unique_consecutive(o.values, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    ntile = (counts + TILE - 1) // TILE
    gidx = torch.repeat_interleave(torch.arange(keys.numel(), device=dev), ntile)
    first = torch.cumsum(ntile, 0) - ntile
    k_in_group = torch.arange(int(ntile.sum()), device=dev) - first[gidx]
    t_start = starts[gidx] + k_in_group * TILE
    t_count = torch.minimum(counts[gidx] - k_in_group * TILE, torch.full_like(k_in_group, TILE))
    t_slot = keys[gidx] % T
    t_level = keys[gidx] // T
    f['tile_start'] = t_start.to(torch.int32).contiguous()
    f['tile_count'] = t_count.to(torch.int32).contiguous()
    f['tile_slot'] = t_slot.to(torch.int32).contiguous()
    # tiles grouped by slot, for the per-slot weight-gradient pass of the backward sweep
    f['slot_tiles'] = torch.sort(t_slot, stable=True).indices.to(torch.int32).contiguous()
    stp = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    stp[1:] = torch.cumsum(torch.bincount(t_slot, minlength=T), 0)
    f['slot_tile_ptr'] = [int(v) for v in stp.tolist()]        # host copy
    per_level = torch.bincount(t_level, minlength=max(L, 1))
    ltp = torch.zeros(max(L, 1) + 1, dtype=torch.int64, device=dev)
    ltp[1:] = torch.cumsum(per_level, 0)
    f['level_tile_ptr'] = [int(v) for v in ltp.tolist()]      # host copy: launch geometry
    f['num_tiles'] = int(t_start.numel())
    f['n_active'] = int(nodes.numel())
    f['num_slots'] = T
    return f


def order_rows(g, n, order, order_span, gslot):
    dev, E = order.device, g.E
    on = order.long()
    rows = torch.full((n, ROW_INTS), -1, dtype=torch.int32, device=dev)
    rows[:, 0:4] = order_span
    if E > 0 and n > 0:
        in0, in1 = g.in_ptr[on].long(), g.in_ptr[on + 1].long()
        idx = in0[:, None] + torch.arange(4, device=dev)
        ok = idx < in1[:, None]
        rows[:, 4:8] = torch.where(ok, g.in_src[idx.clamp(max=E - 1)], torch.full_like(idx, -1, dtype=torch.int32))
        o0, o1 = g.out_ptr[on].long(), g.out_ptr[on + 1].long()
        oidx = o0[:, None] + torch.arange(ROW_OUT, device=dev)
        ook = oidx < o1[:, None]
        oc = oidx.clamp(max=E - 1)
        c = torch.where(ook, g.out_dst[oc], torch.full_like(oc, -1, dtype=torch.int32))
        sl = torch.where(ook, g.out_slot[oc], torch.full_like(oc, -1, dtype=torch.int32))
        rows[:, 8:24] = torch.stack([c, sl], 2).reshape(n, 2 * ROW_OUT)
        gc = torch.where(ook, gslot[c.clamp(min=0).long()], torch.full_like(oc, NO_GATE, dtype=torch.uint8))
        rows[:, 24:26] = gc.contiguous().view(torch.int32)
    return rows


def first_stage_pairs(g, xcls, max_classes):
    """GraphPlan.first_stage_classes by torch.unique of the (in-degree, class) codes."""
    dev = g.in_ptr.device
    deg = (g.in_ptr[1:] - g.in_ptr[:-1]).long()
    uniq, inv = torch.unique(deg * 256 + xcls.long(), return_inverse=True)
    C = int(uniq.numel())
    if not 0 < C <= max_classes:
        return None
    ptr = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(uniq // 256, 0)
    idx = torch.zeros(max(int(ptr[-1].item()), 1), dtype=torch.int32, device=dev)
    return (inv.to(torch.int32).contiguous(), C, ptr.to(torch.int32).contiguous(), idx, (uniq % 256).to(torch.uint8).contiguous())


def stage(C, cid, rev, ptr, idx, ent_idx, own, own32, xcls, heavy, own_rows, own_levels, ent_rows, ent_levels):
    """A quotient stage as the encoders read it (GraphPlan.quotient has the fields); `heavy`: the rows with more than HEAVY_ROW
    neighbours, int32."""
    return dict(C=C, cid=cid, rev=rev, ptr=ptr, idx=idx, ent_idx=ent_idx, own=own, own32=own32, xcls=xcls,
                heavy=(int(heavy.numel()), heavy), own_rows=own_rows, own_levels=own_levels, ent_rows=ent_rows, ent_levels=ent_levels)


def colour_lists_equal(pl, il, owner, prev, inv, rep, xc, Cp):
    """Exact check of a grouping by sorting: every node has its representative's feature class, previous colour, degree and
    neighbour-colour multiset (both lists sorted by colour and compared entry by entry).  All arguments int64."""
    deg = pl[1:] - pl[:-1]
    pn = prev[il]
    ri = rep[inv]
    same = (xc == xc[ri]) & (prev == prev[ri]) & (deg == deg[ri])
    sorted_col = torch.sort(owner * (Cp + 1) + pn).values - owner * (Cp + 1)      # each node's list, colours ascending
    k_in_list = torch.arange(owner.numel(), dtype=torch.int64, device=pl.device) - pl[:-1][owner]
    lists_same = sorted_col == sorted_col[(pl[:-1][ri[owner]] + k_in_list).clamp_(max=max(owner.numel() - 1, 0))]
    return bool(same.all()) and bool(lists_same.all())


def colour_key_and_check(g, xcls, first_stage_is_pairs=False):
    """(key, check) of the stage loop below, by torch: key(t, rev, prev, Cp, f) -> the int64 grouping key of every node, two sums of
    the random values f of its neighbours' colours folded with its own colour, class and degree; check(rev, prev, Cp, inv, rep) ->
    whether the grouping `inv` with representatives `rep` is exact (colour_lists_equal).  `first_stage_is_pairs` is plan_device's
    (one signature for both builders); the torch key of stage 1 is the general one."""
    xc = xcls.long()
    owner_of = functools.lru_cache(None)(lambda rev: owner(g, rev))      # the row of every CSR slot, once per direction

    def key(t, rev, prev, Cp, f):
        p, idx = lists(g, rev)
        pl, pn = p.long(), prev[idx.long()]
        i64 = dict(dtype=torch.int64, device=pl.device)
        h1 = torch.zeros(g.N, **i64).index_add_(0, owner_of(rev), f[0][pn])
        h2 = torch.zeros(g.N, **i64).index_add_(0, owner_of(rev), f[1][pn])
        return h1 * 0x1E3779B97F4A7C15 + h2 + f[2][prev] + xc * 0x632BE59BD9B4E019 + (pl[1:] - pl[:-1]) * 0x2545F4914F6CDD1D

    def check(rev, prev, Cp, inv, rep):
        p, idx = lists(g, rev)
        return colour_lists_equal(p.long(), idx.long(), owner_of(rev), prev, inv, rep, xc, Cp)
    return key, check


def quotient_stages(g, xcls, max_stages, admits, goes_on, key=None, check=None):
    """The stages of GraphPlan.quotient by torch sorts and scans.  `admits(C)`: a stage of C colours still runs on colours;
    `goes_on(C)`: a stage behind it is worth trying.  `key` / `check`: the grouping key and the exact check of a stage
    (colour_key_and_check; a device plan passes plan_device's, which put the plan builder's kernels there)."""
    if key is None:
        key, check = colour_key_and_check(g, xcls)
    N, dev = g.N, g.in_ptr.device
    i64 = dict(dtype=torch.int64, device=dev)
    empty = lambda: torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    stages = []
    prev, Cp = torch.zeros(N, **i64), 1
    for t_ in range(1, max_stages + 1):
        rev = t_ % 2 == 0
        p, idx = lists(g, rev)
        pl, il = p.long(), idx.long()
        deg = pl[1:] - pl[:-1]
        f = torch.randint(1, 1 << 62, (3, Cp + 1), generator=gen, **i64)
        mix = key(t_, rev, prev, Cp, f)
        # ONE stable sort of the keys groups the nodes: colour = rank of the key, representative = first member of its run
        # (a scatter-min onto a handful of addresses costs 27 ms; torch.unique + a second sort by colour 1.6 ms more)
        skey, by_colour = torch.sort(mix, stable=True)
        first = torch.ones(N, dtype=torch.bool, device=dev)
        first[1:] = skey[1:] != skey[:-1]
        starts = torch.nonzero(first).reshape(-1)
        C = int(starts.numel())
        if not admits(C):
            break
        inv = torch.empty(N, **i64)
        inv[by_colour] = torch.cumsum(first, 0) - 1
        members = torch.diff(starts, append=torch.tensor([N], **i64))
        rep = by_colour[starts]
        # the key above only PROPOSES the grouping: every member has its representative's feature class, previous colour, degree and
        # neighbour-colour multiset, or the refinement stops here
        if not check(rev, prev, Cp, inv, rep):
            break
        dr = deg[rep]
        rptr = torch.zeros(C + 1, **i64)
        rptr[1:] = torch.cumsum(dr, 0)
        n_ent = int(rptr[-1].item())
        row = torch.repeat_interleave(torch.arange(C, **i64), dr)
        k = torch.arange(n_ent, **i64) - rptr[row]
        ent = prev[il[pl[rep][row] + k]] if n_ent else torch.zeros(0, **i64)
        own = prev[rep]
        # per colour of stage t-1: the representatives that own it / the list entries that name it, as segment tables of
        # mgv_seg_sum (a colour like "AND gate" is named by thousands of entries: balanced, and summed in a fixed order)
        own_o, own_levels = class_sum_levels(own, Cp)
        ent_o, ent_levels = class_sum_levels(ent, Cp)
        stages.append(stage(C, inv.to(torch.int32).contiguous(), rev, rptr.to(torch.int32).contiguous(),
                            (ent + C).to(torch.int32).contiguous() if n_ent else empty(),
                            ent.to(torch.int32).contiguous() if n_ent else empty(),
                            own, own.to(torch.int32).contiguous(), xcls[rep].contiguous(),
                            torch.nonzero(dr > HEAVY_ROW).reshape(-1).to(torch.int32).contiguous(), own_o, own_levels,
                            row[ent_o.long()].to(torch.int32).contiguous() if n_ent else empty(), ent_levels))
        prev, Cp = inv, C
        last_sorted = (by_colour, members)
        if not goes_on(C):
            break                    # colours multiply per half round: the next one would not qualify
    if stages:
        stages[-1]['sum_levels'] = class_sum_levels(stages[-1]['cid'], stages[-1]['C'], presorted=last_sorted)
    return stages


def class_sum_levels(cid, C, seg=64, presorted=None):
    """Segment tables of mgv_seg_sum for per-colour row sums: (order [N] int32 = nodes sorted by colour, tables) with
    tables = dict(C, rows, levels=[(n_seg, seg_ptr int32, out_row int32 | None, src_row)]).  The sums live in ONE buffer of
    `rows` rows: the first C are the colours' sums, partial rows follow.  Level 1 cuts every colour's run of members into
    segments of <= seg: a colour that fits one segment writes its final row, the others leave one partial row per segment
    (colour by colour, in order) from row C on; level l+1 does the same with the partial rows level l left at `src_row`
    — only for the colours that still have more than one — until none is left.  `presorted`: (items sorted by colour, members per
    colour) in place of a sort of `cid`."""
    i64 = dict(dtype=torch.int64, device=cid.device)
    if presorted is not None:
        order, counts = presorted[0].to(torch.int32).contiguous(), presorted[1]
    else:
        srt = torch.sort(cid.long(), stable=True)
        order = srt.indices.to(torch.int32).contiguous()
        # members per colour from the sorted run boundaries (a histogram with atomics costs ~1 ms on 2.7 M entries, this 30 us)
        bounds = torch.searchsorted(srt.values, torch.arange(C + 1, **i64))
        counts = bounds[1:] - bounds[:-1]
    levels = []
    counts0 = counts
    gid = torch.arange(C, **i64)         # the colours still being summed
    base, src_row = C, 0
    while True:
        G = int(gid.numel())
        nseg = torch.clamp((counts + seg - 1) // seg, min=1)         # (a colour nobody carries still gets its zero row)
        cls = torch.repeat_interleave(torch.arange(G, **i64), nseg)
        total = int(cls.numel())
        first = torch.cumsum(nseg, 0) - nseg
        start = torch.cumsum(counts, 0) - counts
        sp = torch.empty(total + 1, **i64)
        sp[:total] = start[cls] + seg * (torch.arange(total, **i64) - first[cls])
        sp[total] = counts.sum()
        multi = nseg > 1
        seg_multi = multi[cls]
        n_partial = int(seg_multi.sum().item())
        if n_partial == 0 and G == C and base == C:
            out_row = None                                           # every colour is one segment: segment s writes row s
        else:
            out_row = torch.where(seg_multi, base + torch.cumsum(seg_multi, 0) - 1, gid[cls]).to(torch.int32).contiguous()
        levels.append((total, sp.to(torch.int32).contiguous(), out_row, src_row))
        if n_partial == 0:
            return order, dict(C=C, rows=base, levels=levels, counts=counts0)
        gid, counts = gid[multi], nseg[multi]
        src_row, base = base, base + n_partial


def seg_entries(g, reverse, order, n_seg, seg_ptr):
    """GraphPlan.seg_entries: per member its own entry, then the complement of every neighbour in `lists(g, reverse)`."""
    p, idx = lists(g, reverse)
    n, dev = int(order.numel()), order.device
    o, pl = order.long(), p.long()
    deg = pl[o + 1] - pl[o]
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(deg + 1, 0)
    entries = torch.empty(int(off[-1].item()), dtype=torch.int64, device=dev)
    entries[off[:-1]] = o
    member = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), deg)
    k = torch.arange(int(member.numel()), dtype=torch.int64, device=dev) - (off[:-1] - torch.arange(n, dtype=torch.int64, device=dev))[member]
    entries[off[member] + 1 + k] = ~idx.long()[pl[o][member] + k]
    return entries.to(torch.int32).contiguous(), off[seg_ptr.long()].to(torch.int32).contiguous()
