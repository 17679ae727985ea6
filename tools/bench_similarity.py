#!/usr/bin/env python3
"""Time the functional-similarity search (mgv_row_unit, mgv_sim_select_count / mgv_sim_select_fill of csrc/pair_scores.hip, ops.sim_topk,
ops.sim_pairs) against the general selection on the same unit rows (mgv_pair_select_*, ops.pair_select(y, y, skip_self=True)) and against
the chunked torch route, on the same device, in the same process.

    python tools/bench_similarity.py                       # one 65,536-node graph and a config-2 batch of 64 such graphs
    python tools/bench_similarity.py --skip-batch

H = 64.  Rows: every graph's nodes fall, in a random order, into clusters of 9 around a random centre with noise 1e-2 |c| / sqrt(H) per
entry (cosine about 0.9999 inside a cluster: 8 partners per row, 4 pairs per row in the upper triangle), each row scaled into (0, 1).
Two regimes per box:
  sparse : threshold 0.999, the clusters
  dense  : the threshold is the 0.99 quantile of a 2,048 x 2,048 sample of the cosines: about 1 % of the pairs
unit   : mgv_row_unit, in GB/s against 2 N H 4 bytes         topk8 : ops.sim_topk at k = 8 (unit rows included)
count / fill / whole : the symmetric entries and ops.sim_pairs(with_scores=True) (unit rows, count, scan, read-back, fill, pair_index)
gen_*  : the general entries on (y, y, skip_self = 1) and ops.pair_select(y, y, ..., with_scores=True): every pair from both sides
torch  : (y[blk] @ y.T > thr).nonzero() per 4,096 rows of each graph, kept where v > u
The symmetric walk visits (T + 1) / (2 T) of the general walk's tiles (T = 64-row tiles per graph): the floor of count / gen_count.
One process; every shape warmed up first; HIP events around the device work, median of --reps; the symmetric and the general route
are timed alternately, call by call.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

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


def clustered_rows(graphs, n, H, g, dev, size=9):
    N = graphs * n
    centres = torch.randn(graphs * ((n + size - 1) // size), H, generator=g, device=dev)
    per = (n + size - 1) // size
    x = torch.empty(N, H, device=dev)
    for gi in range(graphs):
        cid = torch.randperm(n, generator=g, device=dev) // size + gi * per
        c = centres[cid]
        c = c + 1e-2 * c.norm(dim=1, keepdim=True) / H ** 0.5 * torch.randn(n, H, generator=g, device=dev)
        x[gi * n:(gi + 1) * n] = c * (torch.rand(n, 1, generator=g, device=dev) * 0.2 + 0.01)
    return x


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H = 64
    g = torch.Generator(device=dev).manual_seed(0)

    def box(graphs, tag, reps):
        n = a.graph_n
        N = graphs * n
        x = clustered_rows(graphs, n, H, g, dev)
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        y = torch.empty_like(x)
        unit_ms = timed(lambda: _hip.call('mgv_row_unit', H, N, ptr(x), H, 1e-8, ptr(y), H, None), max(reps, 5), warm=2)
        m = min(2048, n)
        sample = torch.mm(y[:m], y[:m].T).flatten()
        dense = float(sample.kthvalue(int(0.99 * sample.numel())).values)
        del sample
        topk_ms = timed(lambda: ops.sim_topk(x, 8, graph_ptr=gp), reps)
        T = (n + 63) // 64
        for regime, thr in (('sparse', 0.999), ('dense', dense)):
            sym = (H, N, ptr(y), H, ptr(gp), graphs, thr)
            gen = (H, N, ptr(y), H, ptr(y), H, ptr(gp), graphs, 0, thr, 1)
            n_sym = torch.empty(N, dtype=torch.int32, device=dev)
            n_gen = torch.empty(N, dtype=torch.int32, device=dev)
            count_ms, gen_count_ms = timed_alternately(lambda: _hip.call('mgv_sim_select_count', *sym, ptr(n_sym)),
                                                       lambda: _hip.call('mgv_pair_select_count', *gen, ptr(n_gen)), reps)

            def scan(cnt):
                row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
                torch.cumsum(cnt, 0, dtype=torch.int64, out=row_ptr[1:])
                return row_ptr, int(row_ptr[-1])
            sym_ptr, pairs = scan(n_sym)
            gen_ptr, links = scan(n_gen)
            col, val = torch.empty(links, dtype=torch.int32, device=dev), torch.empty(links, device=dev)
            fill_ms, gen_fill_ms = timed_alternately(lambda: _hip.call('mgv_sim_select_fill', *sym, ptr(sym_ptr), pairs, ptr(col), ptr(val)),
                                                     lambda: _hip.call('mgv_pair_select_fill', *gen, ptr(gen_ptr), links, ptr(col), ptr(val)), reps)
            del col, val
            whole_ms, gen_whole_ms = timed_alternately(
                lambda: ops.sim_pairs(x, graph_ptr=gp, threshold=thr, with_scores=True),
                lambda: ops.pair_select(y, y, graph_ptr=gp, sigmoid=False, threshold=thr, skip_self=True, with_scores=True), reps)
            found = [0]

            def torch_chunks():
                found[0] = 0
                for gi in range(graphs):
                    lo = gi * n
                    tg = y[lo:lo + n].T
                    for b0 in range(lo, lo + n, 4096):
                        nz = (torch.mm(y[b0:b0 + 4096], tg) > thr).nonzero()
                        found[0] += int((nz[:, 1] + lo > nz[:, 0] + b0).sum())
            torch_ms = timed(torch_chunks, max(1, reps // 2 if graphs > 1 else reps), warm=1 if graphs == 1 else 0)
            print(json.dumps({'case': '%s_%s' % (tag, regime), 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'threshold': thr,
                              'pairs': pairs, 'pairs_per_row': pairs / N, 'share_of_pairs': links / (graphs * float(n) * n),
                              'links_general': links, 'general_is_twice_symmetric': links == 2 * pairs,
                              'unit_ms': unit_ms, 'unit_GBps': 2.0 * N * H * 4 / (unit_ms * 1e-3) / 1e9, 'topk8_ms': topk_ms,
                              'count_ms': count_ms, 'fill_ms': fill_ms, 'whole_ms': whole_ms,
                              'gen_count_ms': gen_count_ms, 'gen_fill_ms': gen_fill_ms, 'gen_whole_ms': gen_whole_ms,
                              'count_over_gen': count_ms / gen_count_ms, 'fill_over_gen': fill_ms / gen_fill_ms,
                              'whole_over_gen': whole_ms / gen_whole_ms, 'tile_floor': (T + 1) / (2.0 * T),
                              'torch_chunked_ms': torch_ms, 'torch_over_whole': torch_ms / whole_ms, 'torch_pairs': found[0]}), flush=True)

    box(1, 'one_graph', a.reps)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', 1)


if __name__ == '__main__':
    main()
