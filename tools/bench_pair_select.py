#!/usr/bin/env python3
"""Time the thresholded-link entries (mgv_pair_select_count / mgv_pair_select_fill of csrc/pair_scores.hip, ops.pair_select) against
mgv_pair_topk at k = 1 and against the chunked torch route on the same device, in the same process.

    python tools/bench_pair_select.py                      # one 65,536-node graph and a config-2 batch of 64 such graphs
    python tools/bench_pair_select.py --skip-batch

Raw scores (no sigmoid), H = 64, operands 0.3 randn, two regimes per box:
  sparse : the threshold is the median over the rows of the second-best raw score (mgv_pair_topk, k = 2): about two links per row
  dense  : the threshold is the 0.99 quantile of a 2,048 x 2,048 sample of the scores: about 1 % of the pairs
count  : mgv_pair_select_count                fill : mgv_pair_select_fill (col and score) on the scanned counts
whole  : ops.pair_select(with_scores=True): count, scan, the read-back of the total, allocation, fill
topk1  : mgv_pair_topk at k = 1 with the same threshold (it scans AND inserts; the expectation is count <= topk1 and fill <= topk1)
torch  : (s[blk] @ t.T > thr).nonzero() per 4,096 rows of each graph
One process; warm-up first; HIP events around the device work, median of --reps.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_F32_MATRIX = 157e12


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


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
        st = 0.3 * torch.randn(N, 2 * H, generator=g, device=dev)
        s, t = st[:, :H], st[:, H:]
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        idx = torch.empty(N, 2, dtype=torch.int32, device=dev)
        score = torch.empty(N, 2, device=dev)
        na = torch.empty(N, dtype=torch.int32, device=dev)
        _hip.call('mgv_pair_topk', H, N, ptr(s), 2 * H, ptr(t), 2 * H, ptr(gp), graphs, 2, 0, 0.0, 0, ptr(idx), ptr(score), ptr(na))
        sparse = float(score[:, 1].median())
        m = min(2048, n)
        sample = torch.mm(s[:m].contiguous(), t[:m].contiguous().T).flatten()
        dense = float(sample.kthvalue(int(0.99 * sample.numel())).values)
        del sample
        sc, tc = s.contiguous(), t.contiguous()
        for regime, thr in (('sparse', sparse), ('dense', dense)):
            common = (H, N, ptr(s), 2 * H, ptr(t), 2 * H, ptr(gp), graphs, 0, thr, 0)
            n_sel = torch.empty(N, dtype=torch.int32, device=dev)
            count_ms = timed(lambda: _hip.call('mgv_pair_select_count', *common, ptr(n_sel)), reps)
            row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            torch.cumsum(n_sel, 0, dtype=torch.int64, out=row_ptr[1:])
            total = int(row_ptr[-1])
            col = torch.empty(total, dtype=torch.int32, device=dev)
            val = torch.empty(total, device=dev)
            fill_ms = timed(lambda: _hip.call('mgv_pair_select_fill', *common, ptr(row_ptr), total, ptr(col), ptr(val)), reps)
            del col, val
            whole_ms = timed(lambda: ops.pair_select(s, t, graph_ptr=gp, sigmoid=False, threshold=thr, with_scores=True), reps)
            topk_ms = timed(lambda: _hip.call('mgv_pair_topk', H, N, ptr(s), 2 * H, ptr(t), 2 * H, ptr(gp), graphs, 1, 0, thr, 0, ptr(idx),
                                              ptr(score), ptr(na)), reps)
            same_counts = bool(torch.equal(na, n_sel))
            found = [0]

            def torch_chunks():
                found[0] = 0
                for gi in range(graphs):
                    lo = gi * n
                    tg = tc[lo:lo + n].T
                    for b0 in range(lo, lo + n, 4096):
                        found[0] += (torch.mm(sc[b0:b0 + 4096], tg) > thr).nonzero().shape[0]
            torch_ms = timed(torch_chunks, max(1, reps // 2 if graphs > 1 else reps), warm=1 if graphs == 1 else 0)
            print(json.dumps({'case': '%s_%s' % (tag, regime), 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'threshold': thr,
                              'links': total, 'links_per_row': total / N, 'share_of_pairs': total / (graphs * float(n) * n),
                              'count_ms': count_ms, 'fill_ms': fill_ms, 'whole_ms': whole_ms, 'topk1_ms': topk_ms, 'torch_chunked_ms': torch_ms,
                              'count_over_topk1': count_ms / topk_ms, 'fill_over_topk1': fill_ms / topk_ms, 'torch_over_whole': torch_ms / whole_ms,
                              'mfma_floor_ms': 2.0 * graphs * float(n) ** 2 * H / PEAK_F32_MATRIX * 1e3,
                              'n_sel_equals_n_above': same_counts, 'torch_links': found[0]}), flush=True)

    box(1, 'one_graph', a.reps)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', 1)


if __name__ == '__main__':
    main()
