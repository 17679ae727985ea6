"""Negative edge sampling for the reconstruction loss.

The reference calls `torch_geometric.utils.negative_sampling(pos ∪ self-loops, N)`
(dg_ae_model_aig.py:115-119): as many (src, dst) pairs as that edge set has, drawn uniformly from the
pairs that are neither an existing edge nor a self loop (pairs may cross graphs of a batch).  Same
distribution here, from rejection sampling on the device with torch index ops (the pairs feed the
HIP recon-loss kernel), or — when the batch's GraphPlan is at hand — from the fused device sampler
(`negative_sampling_device`, csrc/neg_sample.hip), which also buckets the pairs by source and by destination so
that the loss gradient needs no atomics.

Opt-in, beside the reference's draw: `graph_ptr=` draws the destination inside the source's own graph (the candidates the evaluation
entries rank a link against), `reverse=` makes a share of the pairs reversals (v, u) of true links (u, v), the hard negatives of a
directed decoder (csrc/mgv_neg_draw.h: neg_draw_slot_local; csrc/neg_partition.hip: mgv_neg_partition_local, mgv_neg_draw_local)."""
import itertools
import os

import torch

from . import _hip
from ._hip import ptr

_CALLS = itertools.count()

# the block-partition route of negative_sampling_device (csrc/neg_partition.hip); MGV_NEG_PARTITION=0, or PARTITION = False from a test,
# keeps the two-entry route (mgv_neg_sample, mgv_neg_bucket, two list sorts): the same arrays either way
PARTITION = os.environ.get('MGV_NEG_PARTITION', '1') != '0'
PART_MAX_SHIFT = 12          # nodes per block the finishing pass scans in LDS: 4,096
PART_MAX_BLOCKS = 2048       # blocks the partition pass ranks in LDS
PART_TARGET = 12288          # expected pairs per block, at the most: a finishing trip holds 16,384 (Poisson: 37 sigma of margin)
PART_MAX_E = 1 << 28


def partition_shift(N, E):
    """log2 of the node-block size of the partition route for E pairs over N nodes, or None where negative_sampling_device takes
    the two-entry route: the smallest shift that keeps the block count inside PART_MAX_BLOCKS, raised while the expected pairs per
    block (E 2^shift / N) stay inside PART_TARGET.  A pure function of (N, E): no device state, no read-back."""
    N, E = int(N), int(E)
    if N < 2 or N >= 1 << 31 or E < 1 or E >= PART_MAX_E:
        return None
    s = 0
    while s < PART_MAX_SHIFT and (N + (1 << s) - 1) >> s > PART_MAX_BLOCKS:
        s += 1
    if (N + (1 << s) - 1) >> s > PART_MAX_BLOCKS:
        return None
    while s < PART_MAX_SHIFT and E << (s + 1) <= PART_TARGET * N:
        s += 1
    return s


class NegativeEdges:
    """Sampled negative pairs grouped by source: `edge_index` [2, E] int64 plus the two int32 CSRs over them."""

    def __init__(self, edge_index, out_ptr, out_dst, in_ptr, in_src):
        self.edge_index, self.out_ptr, self.out_dst, self.in_ptr, self.in_src = edge_index, out_ptr, out_dst, in_ptr, in_src

    @property
    def csr(self):
        return self.out_ptr, self.out_dst, self.in_ptr, self.in_src


def bucket_negatives(neg, N):
    """NegativeEdges over the pairs `neg` [2, E] (int64, device): both CSRs from the batch builder's CSR kernels (histogram,
    scan, cursor fill, per-list sort by pair id: every list comes out in pair order whatever order the atomics ran in), the pair
    list re-emitted in by-source order.  Deterministic, unlike a plain atomic-cursor bucketing."""
    dev = neg.device
    E = int(neg.shape[1])
    i32 = dict(dtype=torch.int32, device=dev)
    src, dst = neg[0].contiguous(), neg[1].contiguous()
    in_ptr, out_ptr = torch.empty(N + 1, **i32), torch.empty(N + 1, **i32)
    in_src, in_dst, out_dst, out_slot = (torch.empty(max(E, 1), **i32) for _ in range(4))
    n_s = _hip.call_value('mgv_plan_csr_scratch_ints', N, E)
    scratch = torch.empty(n_s, **i32)
    status = torch.empty(2, **i32)
    _hip.call('mgv_plan_csr', N, E, ptr(src), ptr(dst), ptr(in_ptr), ptr(in_src), ptr(in_dst), ptr(out_ptr), ptr(out_dst), ptr(out_slot),
              None, None, ptr(scratch), n_s, ptr(status))
    if int(status[0].item()) != 0:           # caller-supplied pairs, bucketed once and cached: one host read
        raise ValueError('neg_edge_index holds node ids outside [0, num_nodes)')
    counts = (out_ptr[1:] - out_ptr[:-1]).long()
    srt_src = torch.repeat_interleave(torch.arange(N, device=dev), counts, output_size=E)
    srt = torch.stack([srt_src, out_dst[:E].long()])
    return NegativeEdges(srt, out_ptr, out_dst, in_ptr, in_src)


def check_graph_ptr(graph_ptr, num_nodes):
    """The batch's graph table as a host int64 tensor [G + 1], validated on the host: at least one graph, non-decreasing (empty graphs
    allowed), first entry 0, last entry num_nodes.  ValueError otherwise."""
    gp = torch.as_tensor(graph_ptr).detach().to('cpu', torch.int64).reshape(-1)
    if gp.numel() < 2:
        raise ValueError('graph_ptr needs at least one graph (two entries), got %d entries' % gp.numel())
    if int(gp[0]) != 0 or int(gp[-1]) != int(num_nodes):
        raise ValueError('graph_ptr must start at 0 and end at num_nodes = %d, got %d .. %d' % (int(num_nodes), int(gp[0]), int(gp[-1])))
    if bool((gp[1:] < gp[:-1]).any()):
        raise ValueError('graph_ptr must be non-decreasing')
    return gp


def reverse_count(reverse, E):
    """R = floor(reverse * E + 0.5) of E slots: the slots that are reversals of a true edge.  reverse lies in [0, 1]."""
    reverse = float(reverse)
    if not 0.0 <= reverse <= 1.0:                # (also refuses a NaN)
        raise ValueError('reverse must lie in [0, 1], got %r' % reverse)
    return int(reverse * int(E) + 0.5)


def device_graph_ptr(plan, graph_ptr):
    """(int32 device tensor [G + 1], G) of a batch's graph table for the local draw: validated (check_graph_ptr) and uploaded once, on the
    current stream, and kept on the batch's plan for as long as the same table object comes back (BatchPrefetcher makes this call on
    its worker's stream, with the rest of the batch).  None: the whole batch is one graph."""
    if graph_ptr is None:
        graph_ptr = getattr(plan, '_one_graph_ptr', None)
        if graph_ptr is None:
            graph_ptr = plan._one_graph_ptr = torch.tensor([0, plan.N], dtype=torch.int64)
    hit = getattr(plan, '_graph_ptr_i32', None)
    if hit is None or hit[0] is not graph_ptr:
        gp = check_graph_ptr(graph_ptr, plan.N)
        hit = plan._graph_ptr_i32 = (graph_ptr, gp.to(torch.int32).to(plan.device, non_blocking=True), int(gp.numel()) - 1)
    return hit[1], hit[2]


def _local_negatives(plan, E, seed, graph_ptr, R):
    """NegativeEdges of the local draw (csrc/mgv_neg_draw.h, neg_draw_slot_local): in one entry (mgv_neg_partition_local) where
    partition_shift allows, else the draw alone (mgv_neg_draw_local) bucketed by the plan builder's CSR kernels (bucket_negatives: one
    host read of its status) and the two list sorts.  The same arrays either way."""
    N, dev = plan.N, plan.device
    gp, G = device_graph_ptr(plan, graph_ptr)
    local = (R, G, ptr(gp), plan.E, ptr(plan.in_src), ptr(plan.in_dst))
    i32 = dict(dtype=torch.int32, device=dev)
    shift = partition_shift(N, E) if PARTITION else None
    if shift is not None:
        srt = torch.empty(2, E, dtype=torch.int64, device=dev)
        ptrs, out_dst, in_src = torch.empty(2, N + 1, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
        ws = torch.empty(_hip.call_value('mgv_neg_partition_ws_ints', N, E), **i32)
        _hip.call('mgv_neg_partition_local', N, E, seed, shift, ptr(plan.out_ptr), ptr(plan.out_dst), *local, ptr(srt), ptr(ptrs[0]),
                  ptr(out_dst), ptr(ptrs[1]), ptr(in_src), ptr(ws), ws.numel())
        return NegativeEdges(srt, ptrs[0], out_dst, ptrs[1], in_src)
    neg = torch.empty(2, E, dtype=torch.int64, device=dev)
    _hip.call('mgv_neg_draw_local', N, E, seed, R, G, ptr(gp), ptr(plan.out_ptr), ptr(plan.out_dst), plan.E, ptr(plan.in_src), ptr(plan.in_dst),
              ptr(neg[0]), ptr(neg[1]))
    if E == 0:                                   # no slots: empty buckets
        return NegativeEdges(neg, torch.zeros(N + 1, **i32), torch.empty(1, **i32), torch.zeros(N + 1, **i32), torch.empty(1, **i32))
    ne = bucket_negatives(neg, N)
    ss = torch.empty(N + 1 + E, **i32)           # lists in pair order -> ascending, as the partition route leaves them
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ne.out_ptr), ptr(ne.out_dst), ptr(ss), ss.numel())
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ne.in_ptr), ptr(ne.in_src), ptr(ss), ss.numel())
    ne.edge_index[1].copy_(ne.out_dst[:E])
    return ne


def negative_sampling_device(plan, num_neg_samples=None, generator=None, graph_ptr=None, reverse=0.0):
    """Same distribution as `negative_sampling` (uniform over non-edges that are not self loops, with replacement),
    drawn by one kernel from a counter-based generator seeded from torch's seed and a call counter (no host sync).
    Bucketed by block partition in the same entry (mgv_neg_partition) where partition_shift allows, else by the two-entry route:
    NegativeEdges is the same function of (seed, call number, plan) on both.

    `graph_ptr` (the batch's host int64 table [G + 1]) and `reverse` (a share in [0, 1]) opt into the local draw: the source uniform
    over the batch, the destination uniform over the source's own graph, and the first R = floor(reverse * E + 0.5) slots reversals
    (v, u) of listed edges (u, v) — the candidates link_ranking and predict_links rank a link against, where the reference's draw
    (dg_ae_model_aig.py:115-119) crosses graphs.  Same seed, same count; with neither given, today's calls and today's bits."""
    N, dev = plan.N, plan.device
    loops = plan.count_self_loops()          # (one host read-back per plan; GraphPlan.warm does it on the prefetcher's stream for fresh batches)
    E = (plan.E - loops) + N if num_neg_samples is None else int(num_neg_samples)
    R = reverse_count(reverse, E if plan.E > 0 else 0)          # (no edge to reverse: no reversed slot)
    base = generator.initial_seed() if generator is not None else torch.initial_seed()
    seed = (base * 0x9E3779B97F4A7C15 + next(_CALLS) * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
    if graph_ptr is not None or reverse != 0.0:
        return _local_negatives(plan, E, seed, graph_ptr, R)
    shift = partition_shift(N, E) if PARTITION else None
    if shift is not None:
        i32 = dict(dtype=torch.int32, device=dev)
        srt = torch.empty(2, E, dtype=torch.int64, device=dev)
        ptrs, out_dst, in_src = torch.empty(2, N + 1, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
        ws = torch.empty(_hip.call_value('mgv_neg_partition_ws_ints', N, E), **i32)
        _hip.call('mgv_neg_partition', N, E, seed, shift, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(srt), ptr(ptrs[0]), ptr(out_dst),
                  ptr(ptrs[1]), ptr(in_src), ptr(ws), ws.numel())
        return NegativeEdges(srt, ptrs[0], out_dst, ptrs[1], in_src)
    scratch = torch.zeros(2, N, dtype=torch.int32, device=dev)          # counts by source / destination
    neg = torch.empty(2, E, dtype=torch.int64, device=dev)
    rank = torch.empty(2, max(E, 1), dtype=torch.int32, device=dev)     # every pair's place inside its two buckets
    _hip.call('mgv_neg_sample', N, E, seed, ptr(plan.out_ptr), ptr(plan.out_dst), ptr(neg[0]), ptr(neg[1]), ptr(scratch[0]), ptr(scratch[1]),
              ptr(rank[0]), ptr(rank[1]))
    ptrs = torch.zeros(2, N + 1, dtype=torch.int32, device=dev)
    for k in range(2):                 # 1-D scans (the device-wide scan; the batched innermost-dim kernel is ~100x slower here)
        ptrs[k, 1:] = torch.cumsum(scratch[k], 0, dtype=torch.int32)
    srt = torch.empty(2, E, dtype=torch.int64, device=dev)
    out_dst = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    in_src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    _hip.call('mgv_neg_bucket', E, ptr(neg[0]), ptr(neg[1]), ptr(ptrs[0]), ptr(ptrs[1]), ptr(rank[0]), ptr(rank[1]),
              ptr(srt[0]), ptr(srt[1]), ptr(out_dst), ptr(in_src))
    # the buckets were filled in thread-arrival order: sort every list by neighbour id so that the order (and with it every
    # floating-point sum over a list) no longer depends on thread arrival; equal ids are duplicates of one pair
    ss = torch.empty(N + 1 + E, dtype=torch.int32, device=dev)
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ptrs[0]), ptr(out_dst), ptr(ss), ss.numel())
    _hip.call('mgv_sort_lists_i32', N, E, ptr(ptrs[1]), ptr(in_src), ptr(ss), ss.numel())
    srt[1].copy_(out_dst[:E])          # the pair list in by-source order (sources are constant inside a list)
    return NegativeEdges(srt, ptrs[0], out_dst, ptrs[1], in_src)


def sorted_edge_keys(pos_edge_index, num_nodes):
    """Sorted src*N+dst keys of the non-self-loop edges (static per batch: cache them)."""
    src, dst = pos_edge_index[0].long(), pos_edge_index[1].long()
    keep = src != dst
    return torch.sort(src[keep] * int(num_nodes) + dst[keep]).values


def negative_sampling(pos_edge_index, num_nodes, num_neg_samples=None, generator=None, keys=None, graph_ptr=None, reverse=0.0):
    """The torch route (no plan, or CPU tensors).  `graph_ptr` / `reverse`: the local draw of negative_sampling_device — the same
    distribution (source uniform over the batch, destination uniform over its graph; the first R pairs reversals of listed edges),
    not the same bits."""
    dev = pos_edge_index.device
    N = int(num_nodes)
    if keys is None:
        keys = sorted_edge_keys(pos_edge_index, N)
    want = int(keys.numel()) + N if num_neg_samples is None else int(num_neg_samples)
    R = reverse_count(reverse, want if pos_edge_index.shape[1] > 0 else 0)
    gp = None
    if graph_ptr is not None:
        gp = check_graph_ptr(graph_ptr, N).to(dev)
    if R > 0:
        rev = _rejection(R, N, keys, dev, generator, edges=pos_edge_index)
        return torch.cat([rev, _rejection(want - R, N, keys, dev, generator, gp=gp)], dim=1).contiguous()
    return _rejection(want, N, keys, dev, generator, gp=gp)


def _rejection(want, N, keys, dev, generator, gp=None, edges=None):
    """`want` pairs that are neither a self pair nor an edge of `keys`, by rejection: both ends uniform over [0, N); with `gp` the
    destination uniform over the source's graph; with `edges` the reversal of a uniformly chosen listed edge."""
    out = torch.empty((2, 0), dtype=torch.long, device=dev)
    guard = 0
    while out.shape[1] < want:
        m = want - out.shape[1]
        m = m + m // 8 + 16
        if edges is not None:
            e = torch.randint(0, edges.shape[1], (m,), device=dev, generator=generator)
            s, d = edges[1].long()[e], edges[0].long()[e]
        else:
            s = torch.randint(0, N, (m,), device=dev, generator=generator)
            if gp is None:
                d = torch.randint(0, N, (m,), device=dev, generator=generator)
            else:                            # 31 uniform bits scaled into [gp[g], gp[g + 1]) of s's graph, as the device scales 32
                g = (torch.searchsorted(gp, s, right=True) - 1).clamp_(max=gp.numel() - 2)
                d = gp[g] + ((torch.randint(0, 1 << 31, (m,), device=dev, generator=generator) * (gp[g + 1] - gp[g])) >> 31)
        k = s * N + d
        ok = s != d
        if keys.numel() > 0:
            pos = torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)
            ok &= keys[pos] != k
        out = torch.cat([out, torch.stack([s[ok], d[ok]])], dim=1)
        guard += 1
        if guard > 64:
            raise RuntimeError('negative_sampling: graph too dense to draw %d non-edges' % want)
    return out[:, :want].contiguous()
