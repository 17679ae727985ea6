#!/usr/bin/env python3
"""Time the cross-circuit search (mgv_cross_topk of csrc/pair_scores.hip, ops.cross_topk) against the own-graph search on the same rows
(mgv_pair_topk(y, y, skip_self = 1), ops.sim_topk) and against the chunked torch route, on the same device, in the same process.

    python tools/bench_cross_match.py                      # the three cases
    python tools/bench_cross_match.py --skip-batch

H = 64, k = 8, threshold 0.999, random normal rows made unit rows by mgv_row_unit.  Three cases:
  two_graphs : two 65,536-node graphs, each the other's peer, against sim_topk on ONE such graph: every row scores the same number of
               column tiles in both, so the figure is time PER ROW (cross over 2 N rows, own over N), entry against entry and operator
               against operator; torch: y[a] @ y[b].T and topk(8) per 4,096 rows.
  config2    : a config-2-shaped batch, --batch-graphs graphs in pairs (2i, 2i + 1), against sim_topk on the same batch.
  scattered  : the worst case for row tiles that straddle graphs — 65,536 nodes in graphs of --small-n nodes whose peers are a random
               involution, so the 64 rows of a tile name 64 / small-n peers scattered over the whole batch — against the same batch
               with adjacent peers (2i, 2i + 1).  tiles_scored is what the walk loads and scores (the spans of cross_spans),
               tiles_in_hull what one range from the first to the last candidate would.
One process; every shape warmed up first; HIP events around the device work, median of --reps; the two routes of a comparison are timed
alternately, call by call.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    return sorted(_once(fn) for _ in range(reps))[reps // 2]


def timed_alternately(fa, fb, reps):
    """Medians of two routes measured in turn: a, b, a, b, ..."""
    fa()
    fb()
    ma, mb = [], []
    for _ in range(reps):
        ma.append(_once(fa))
        mb.append(_once(fb))
    return sorted(ma)[reps // 2], sorted(mb)[reps // 2]


def tile_counts(gp, peer):
    """(column tiles the walk scores, column tiles between each row tile's first and last candidate), summed over the row tiles."""
    gp, peer = np.asarray(gp, dtype=np.int64), np.asarray(peer, dtype=np.int64)
    N = int(gp[-1])
    graph_of = np.searchsorted(gp[1:], np.arange(N), side='right')
    p = peer[graph_of]
    lo, hi = np.where(p >= 0, gp[np.maximum(p, 0)], 0), np.where(p >= 0, gp[np.maximum(p, 0) + 1], 0)
    scored = hull = 0
    for r0 in range(0, N, 64):
        a, b = lo[r0:r0 + 64], hi[r0:r0 + 64]
        ok = a < b
        if not ok.any():
            continue
        rng = np.unique(np.stack([a[ok] // 64, (b[ok] + 63) // 64], 1), axis=0)
        scored += len({t for t0, t1 in rng.tolist() for t in range(t0, t1)})
        hull += int(rng[:, 1].max() - rng[:, 0].min())
    return scored, hull


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--small-n', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H, k, thr = 64, 8, 0.999
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = dict(dtype=torch.int32, device=dev)

    def entries(y, gp, peer):
        """(the cross entry, the own-graph entry) on unit rows y as closures over their outputs."""
        N, G = y.shape[0], gp.numel() - 1
        idx, sc, na = torch.empty((N, k), **i32), torch.empty((N, k), device=dev), torch.empty(N, **i32)
        cross = lambda: _hip.call('mgv_cross_topk', H, N, ptr(y), H, ptr(gp), G, ptr(peer), k, thr, ptr(idx), ptr(sc), ptr(na))   # noqa: E731
        own = lambda: _hip.call('mgv_pair_topk', H, N, ptr(y), H, ptr(y), H, ptr(gp), G, k, 0, thr, 1, ptr(idx), ptr(sc), ptr(na))   # noqa: E731
        return cross, own

    n = a.graph_n
    # ---- two graphs against one
    x2 = torch.randn(2 * n, H, generator=g, device=dev)
    y2 = ops.row_unit(x2)
    gp2, gp1, peer2 = torch.tensor([0, n, 2 * n], **i32), torch.tensor([0, n], **i32), torch.tensor([1, 0], **i32)
    cross, _ = entries(y2, gp2, peer2)
    _, own = entries(y2[:n], gp1, torch.tensor([0], **i32))
    cross_ms, own_ms = timed_alternately(cross, own, a.reps)
    op_cross_ms, op_own_ms = timed_alternately(lambda: ops.cross_topk(x2, k, gp2, peer2, threshold=thr),
                                               lambda: ops.sim_topk(x2[:n], k, graph_ptr=gp1, threshold=thr), a.reps)

    def torch_chunks():
        for lo, po in ((0, n), (n, 0)):
            tg = y2[po:po + n].T
            for b0 in range(lo, lo + n, 4096):
                torch.mm(y2[b0:b0 + 4096], tg).topk(k, dim=1)
    torch_ms = timed(torch_chunks, a.reps)
    scored, hull = tile_counts(gp2.tolist(), peer2.tolist())
    print(json.dumps({'case': 'two_graphs', 'nodes_per_graph': n, 'H': H, 'k': k, 'cross_ms': cross_ms, 'sim_topk_one_graph_ms': own_ms,
                      'per_row_over_sim_topk': cross_ms / 2 / own_ms, 'op_cross_ms': op_cross_ms, 'op_sim_topk_one_graph_ms': op_own_ms,
                      'op_per_row_over_sim_topk': op_cross_ms / 2 / op_own_ms, 'torch_chunked_ms': torch_ms,
                      'torch_over_cross': torch_ms / op_cross_ms, 'tiles_scored': scored, 'tiles_in_hull': hull}), flush=True)
    del x2, y2

    # ---- the worst case for straddling row tiles: small graphs, peers scattered over the batch
    s = a.small_n
    Gs = n // s // 2 * 2
    xs = torch.randn(Gs * s, H, generator=g, device=dev)
    ys = ops.row_unit(xs)
    gps = torch.arange(Gs + 1, **i32) * s
    perm = np.random.default_rng(0).permutation(Gs)
    far = np.empty(Gs, dtype=np.int64)
    far[perm[0::2]], far[perm[1::2]] = perm[1::2], perm[0::2]             # a random involution without fixed points
    near = np.arange(Gs) ^ 1
    far_d, near_d = torch.tensor(far, **i32), torch.tensor(near, **i32)
    cross_far, own = entries(ys, gps, far_d)
    cross_near, _ = entries(ys, gps, near_d)
    far_ms, near_ms = timed_alternately(cross_far, cross_near, a.reps)
    own_ms = timed(own, a.reps)
    fs, fh = tile_counts(gps.tolist(), far)
    ns, nh = tile_counts(gps.tolist(), near)
    print(json.dumps({'case': 'scattered', 'graphs': Gs, 'nodes_per_graph': s, 'N': Gs * s, 'H': H, 'k': k, 'scattered_ms': far_ms,
                      'adjacent_ms': near_ms, 'sim_topk_ms': own_ms, 'scattered_over_adjacent': far_ms / near_ms,
                      'tiles_scored': fs, 'tiles_in_hull': fh, 'us_per_scored_tile': 1e3 * far_ms / fs,
                      'adjacent_tiles_scored': ns, 'adjacent_tiles_in_hull': nh}), flush=True)
    del xs, ys

    # ---- a config-2-shaped batch of pairs
    if not a.skip_batch:
        Gb = a.batch_graphs // 2 * 2
        xb = torch.randn(Gb * n, H, generator=g, device=dev)
        yb = ops.row_unit(xb)
        del xb
        gpb = torch.arange(Gb + 1, **i32) * n
        cross, own = entries(yb, gpb, torch.tensor(np.arange(Gb) ^ 1, **i32))
        cross_ms, own_ms = timed_alternately(cross, own, 1)
        print(json.dumps({'case': 'config2', 'graphs': Gb, 'pairs_of_graphs': Gb // 2, 'nodes_per_graph': n, 'N': Gb * n, 'H': H, 'k': k,
                          'cross_ms': cross_ms, 'sim_topk_ms': own_ms, 'over_sim_topk': cross_ms / own_ms}), flush=True)


if __name__ == '__main__':
    main()
