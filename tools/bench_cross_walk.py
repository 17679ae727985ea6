#!/usr/bin/env python3
"""Time the two further consumers of the cross walk (mgv_cross_union and mgv_cross_hist of csrc/pair_scores.hip; ops.cross_classes with
route='walk', ops.cross_threshold_for) against what they replace, on the same device, in the same process.

    python tools/bench_cross_walk.py
    python tools/bench_cross_walk.py --skip-equal

H = 64, random normal rows made unit rows by mgv_row_unit.
Classes — ops.cross_classes(route='walk') against route='pairs' (cross_pairs + sim_pairs + components, the only route before) and
against the floor of one walk each, mgv_cross_select_count + mgv_sim_select_count, with the peak device memory of both routes:
  two_graphs : two 65,536-node circuits, each the other's peer, at the threshold ops.cross_threshold_for gives for 100,000 cross pairs;
  scattered  : 8,192 circuits of 8 gates whose peers are a random involution, threshold 0.25;
  equal_rows : two 16,384-node circuits that share --equal rows of ONE direction each (power-of-two multiples): --equal^2 cross pairs from
               each side and --equal^2 / 2 in each circuit for what is one class of 2 x --equal gates, threshold 0.999.
Threshold by count, on the two_graphs rows:
  threshold  : ops.cross_threshold_for(max_pairs = 100,000) against a bisection of mgv_cross_select_count walks over the float32 values
               of [0, 2] down to adjacent floats (one walk and one read-back of the total per step), both to the same answer;
  hist_walk  : one mgv_cross_hist walk at B = 64 against one mgv_cross_select_count walk.
One process; every shape warmed up first; HIP events around the work (read-backs included), median of --reps; the two routes of a
comparison are timed alternately, call by call.  Prints one JSON line per case."""
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


def timed_alternately(fns, reps):
    """Medians of several routes measured in turn: a, b, c, a, b, c, ..."""
    for f in fns:
        f()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for m, f in zip(ms, fns):
            m.append(_once(f))
    return [sorted(m)[reps // 2] for m in ms]


def peak_bytes(fn):
    """The device memory fn holds at its peak beyond what is allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--small-graphs', type=int, default=8192)
    ap.add_argument('--small-n', type=int, default=8)
    ap.add_argument('--equal', type=int, default=5000)
    ap.add_argument('--max-pairs', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-equal', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H = 64
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = dict(dtype=torch.int32, device=dev)

    def counts(y, gp, peer, thr):
        """(the cross count walk, the own-graph count walk) on unit rows y as closures over their output."""
        N, G = y.shape[0], gp.numel() - 1
        n_sel = torch.empty(N, **i32)
        cross = lambda t=thr: _hip.call('mgv_cross_select_count', H, N, ptr(y), H, ptr(gp), G, ptr(peer), float(t), ptr(n_sel))   # noqa: E731
        own = lambda t=thr: _hip.call('mgv_sim_select_count', H, N, ptr(y), H, ptr(gp), G, float(t), ptr(n_sel))   # noqa: E731
        return cross, own, n_sel

    def classes_case(case, x, gp, peer, thr, reps, **more):
        y = ops.row_unit(x)
        cross, own, n_sel = counts(y, gp, peer, thr)
        cross()
        cross_pairs = int(n_sel.sum(dtype=torch.int64))
        own()
        own_pairs = int(n_sel.sum(dtype=torch.int64))
        walk = lambda: ops.cross_classes(x, gp, peer, threshold=thr, route='walk')     # noqa: E731
        pairs = lambda: ops.cross_classes(x, gp, peer, threshold=thr, route='pairs')   # noqa: E731
        floor = lambda: (cross(), own())                                               # noqa: E731
        lw, lp = walk(), pairs()
        same = all(torch.equal(p, q) for p, q in zip(lw, lp))
        sizes = torch.bincount(lw[0].long())
        del lw, lp
        walk_ms, pairs_ms, floor_ms = timed_alternately([walk, pairs, floor], reps)
        walk_mem, pairs_mem = peak_bytes(walk), peak_bytes(pairs)
        print(json.dumps(dict(case=case, N=x.shape[0], graphs=gp.numel() - 1, H=H, threshold=thr, cross_pairs=cross_pairs,
                              own_pairs=own_pairs, classes_of_2_or_more=int((sizes >= 2).sum()), largest_class=int(sizes.max()),
                              routes_agree=same, walk_ms=walk_ms, pairs_ms=pairs_ms, two_count_walks_ms=floor_ms,
                              walk_over_count_walks=walk_ms / floor_ms, pairs_over_walk=pairs_ms / walk_ms,
                              walk_peak_MiB=walk_mem / 2 ** 20, pairs_peak_MiB=pairs_mem / 2 ** 20, **more)), flush=True)

    n = a.graph_n
    # ---- two large circuits
    x2 = torch.randn(2 * n, H, generator=g, device=dev)
    gp2, peer2 = torch.tensor([0, n, 2 * n], **i32), torch.tensor([1, 0], **i32)
    found = ops.cross_threshold_for(x2, a.max_pairs, gp2, peer2)
    thr2 = found['threshold']
    classes_case('two_graphs', x2, gp2, peer2, thr2, a.reps, nodes_per_graph=n)

    # ---- the threshold by count on the same rows
    y2 = ops.row_unit(x2)
    cross, _, n_sel = counts(y2, gp2, peer2, thr2)
    key = lambda v: int(np.float32(v).view(np.int32))                    # noqa: E731  (non-negative floats: the order of their bits)
    val = lambda k: float(np.int32(k).view(np.float32))                 # noqa: E731
    walks = [0]

    def bisect():
        lo, hi = key(0.0), key(2.0)                                      # count(0) > max_pairs >= count(2) = 0
        walks[0] = 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            cross(val(mid))
            walks[0] += 1
            if int(n_sel.sum(dtype=torch.int64)) <= a.max_pairs:         # the step's read-back
                hi = mid
            else:
                lo = mid
        return val(hi)
    assert bisect() == thr2, (bisect(), found)
    calls = []
    real = _hip.call
    _hip.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    try:
        ops.cross_threshold_for(x2, a.max_pairs, gp2, peer2)
    finally:
        _hip.call = real
    search_ms, bisect_ms = timed_alternately([lambda: ops.cross_threshold_for(x2, a.max_pairs, gp2, peer2), bisect], max(a.reps // 2, 1))
    print(json.dumps(dict(case='threshold', N=2 * n, H=H, max_pairs=a.max_pairs, result=found, profile_walks=calls.count('mgv_cross_hist'),
                          cross_threshold_for_ms=search_ms, bisection_walks=walks[0], bisection_ms=bisect_ms,
                          bisection_over_search=bisect_ms / search_ms)), flush=True)
    for B in (1, 64, 256):
        e = torch.sort(torch.cat([torch.linspace(-1.0, 1.0, B, device=dev)[:B - 1], torch.tensor([thr2], device=dev)]))[0].contiguous()
        hist = torch.empty((2, B + 1), dtype=torch.int64, device=dev)
        walk = lambda: _hip.call('mgv_cross_hist', H, 2 * n, ptr(y2), H, ptr(gp2), 2, ptr(peer2), ptr(e), B, ptr(hist))   # noqa: E731
        hist_ms, count_ms = timed_alternately([walk, cross], a.reps)
        print(json.dumps(dict(case='hist_walk', N=2 * n, H=H, B=B, hist_ms=hist_ms, count_ms=count_ms, hist_over_count=hist_ms / count_ms,
                              candidates=int(hist.sum()))), flush=True)
    del x2, y2

    # ---- many small circuits, peers scattered over the batch
    Gs, s = a.small_graphs // 2 * 2, a.small_n
    xs = torch.randn(Gs * s, H, generator=g, device=dev)
    perm = np.random.default_rng(0).permutation(Gs)
    far = np.empty(Gs, dtype=np.int64)
    far[perm[0::2]], far[perm[1::2]] = perm[1::2], perm[0::2]             # a random involution without fixed points
    classes_case('scattered', xs, torch.arange(Gs + 1, **i32) * s, torch.tensor(far, **i32), 0.25, a.reps, nodes_per_graph=s)
    del xs

    # ---- thousands of equal rows: the pair lists are quadratic, the classes are not
    if not a.skip_equal:
        m, q = 16384, a.equal
        xe = torch.randn(2 * m, H, generator=g, device=dev)
        d = torch.randn(H, generator=g, device=dev)
        scale = 2.0 ** torch.randint(-3, 4, (q, 1), generator=g, device=dev).float()
        for base in (0, m):
            rows = base + torch.randperm(m, generator=g, device=dev)[:q]
            xe[rows] = d * scale
        classes_case('equal_rows', xe, torch.tensor([0, m, 2 * m], **i32), torch.tensor([1, 0], **i32), 0.999, max(a.reps // 2, 1),
                     nodes_per_graph=m, equal_rows_per_graph=q)


if __name__ == '__main__':
    main()
