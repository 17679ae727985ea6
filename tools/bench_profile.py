#!/usr/bin/env python3
"""Time the score-distribution walk (mgv_sim_hist of csrc/pair_scores.hip, ops.sim_profile / ops.sim_threshold_for) against the count walk
it stands in for (mgv_sim_select_count, one threshold per walk) and against a chunked torch route, on the same device, in the same
process.

    python tools/bench_profile.py                       # one 65,536-node graph and a config-2 batch of 64 such graphs
    python tools/bench_profile.py --skip-batch

H = 64, the clustered rows of tools/bench_similarity.py (cosine about 0.9999 inside clusters of 9, 4 pairs per row above 0.999).
hist_B   : one mgv_sim_hist walk over B edges evenly spaced across [-1, 1) plus 0.999 as the last one, B = 1 (0.999 alone), 16, 64, 256
count    : one mgv_sim_select_count walk at 0.999; count_x16: sixteen of them in a row, timed; B count walks cost B times one
torch_64 : the B = 64 profile from torch: per 4,096 rows of each graph the dense cosines against the columns from the block on,
           torch.bucketize against the table and a bincount; the lower triangle of the diagonal block goes to -inf and is taken out of bin 0
search   : ops.sim_threshold_for(x, max_pairs) end to end (unit rows, at most 6 profile walks of 64 edges, one read-back each)
bisect   : the same threshold from a bisection over the float32 values of (0, 2] that calls the count entry once per step
           (unit rows, count, sum, read-back): about 30 walks; both must return the same threshold and pair count
The search replaces about 30 count walks by about 5 profile walks: it pays only while hist_64 costs less than about 5 count walks;
`hist64_over_count` says which.  One process; every shape warmed up first; HIP events around the device work, median of --reps;
the profile and the count walk are timed alternately, call by call.  Prints one JSON line per box."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

import torch  # noqa: E402
from bench_similarity import _once, clustered_rows, timed, timed_alternately  # noqa: E402

BS = (1, 16, 64, 256)


def table(B, dev):
    e = [0.999] if B == 1 else [-1.0 + 2.0 * k / (B - 1) for k in range(B - 1)] + [0.999]
    return torch.tensor(e, dtype=torch.float32, device=dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops, similarity
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H = 64
    g = torch.Generator(device=dev).manual_seed(0)

    def box(graphs, tag, reps, max_pairs):
        n = a.graph_n
        N = graphs * n
        x = clustered_rows(graphs, n, H, g, dev)
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        y = ops.row_unit(x)
        n_sel = torch.empty(N, dtype=torch.int32, device=dev)
        count = lambda thr=0.999: _hip.call('mgv_sim_select_count', H, N, ptr(y), H, ptr(gp), graphs, thr, ptr(n_sel))
        out = {'case': tag, 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'reps': reps}
        above = {}
        for B in BS:
            e = table(B, dev)
            hist = torch.empty((graphs, B + 1), dtype=torch.int64, device=dev)
            walk = lambda: _hip.call('mgv_sim_hist', H, N, ptr(y), H, ptr(gp), graphs, ptr(e), B, ptr(hist))
            out['hist_%d_ms' % B], c = timed_alternately(walk, count, reps)
            out.setdefault('count_ms', c)
            out['count_ms'] = min(out['count_ms'], c)
            above[B] = int(ops.counts_above(hist)[:, -1].sum())
        pairs = int(n_sel.sum(dtype=torch.int64))
        out['pairs_above_0.999'] = pairs
        out['profiles_agree_with_count'] = all(v == pairs for v in above.values())

        def sixteen():
            for _ in range(16):
                count()
        out['count_x16_ms'] = timed(sixteen, max(1, reps // 2), warm=0)
        for B in BS:
            out['hist%d_over_count' % B] = out['hist_%d_ms' % B] / out['count_ms']
            out['hist%d_over_%d_counts' % (B, B)] = out['hist_%d_ms' % B] / (B * out['count_ms'])
        # the torch route at B = 64
        e64 = table(64, dev)
        blk = 4096
        low = torch.ones(blk, blk, dtype=torch.bool, device=dev).tril()
        tp = [None]

        def torch_profile():
            h = torch.zeros((graphs, 66), dtype=torch.int64, device=dev)
            for gi in range(graphs):
                lo = gi * n
                for b0 in range(lo, lo + n, blk):
                    b1 = min(b0 + blk, lo + n)
                    c = torch.mm(y[b0:b1], y[b0:lo + n].T)
                    m = low[:b1 - b0, :b1 - b0]
                    c[:, :b1 - b0][m] = float('-inf')
                    h[gi] += torch.bincount(torch.bucketize(c, e64).flatten(), minlength=66)
                    h[gi, 0] -= int(m.sum())
            tp[0] = h[:, :65]
        out['torch_64_ms'] = timed(torch_profile, max(1, reps // 2 if graphs > 1 else reps), warm=1 if graphs == 1 else 0)
        hist = ops.sim_profile(x, e64, graph_ptr=gp)
        out['torch_pairs_above_0.999'] = int(tp[0][:, -1].sum())
        out['torch_bins_that_differ'] = int((tp[0] != hist).sum())          # torch.mm is another arithmetic: a few pairs near an edge
        out['torch_over_hist64'] = out['torch_64_ms'] / out['hist_64_ms']
        # threshold by count: the profile search against a bisection of count walks
        res, steps, walks = [None], [0], [0]
        real_profile = similarity._unit_profile

        def counted_profile(*args):
            walks[0] += 1
            return real_profile(*args)

        def search():
            walks[0] = 0
            similarity._unit_profile = counted_profile
            try:
                res[0] = ops.sim_threshold_for(x, max_pairs, graph_ptr=gp)
            finally:
                similarity._unit_profile = real_profile

        def bisect():
            yy = ops.row_unit(x)
            lo, hi, steps[0] = similarity._f32_key(0.0), similarity._f32_key(2.0), 0
            val = lambda k: float(torch.tensor(k, dtype=torch.int32).view(torch.float32))

            def total(thr):
                steps[0] += 1
                _hip.call('mgv_sim_select_count', H, N, ptr(yy), H, ptr(gp), graphs, thr, ptr(n_sel))
                return int(n_sel.sum(dtype=torch.int64))
            if total(val(lo)) <= max_pairs:
                res.append((val(lo), None))
                return
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if total(val(mid)) <= max_pairs:
                    hi = mid
                else:
                    lo = mid
            res.append((val(hi), total(val(hi))))
        out['search_ms'], out['bisect_ms'] = timed_alternately(search, bisect, max(1, reps // 2))
        r = res[0]
        out.update({'max_pairs': max_pairs, 'threshold': r['threshold'], 'pairs': r['pairs'], 'lower': r['lower'], 'pairs_lower': r['pairs_lower'],
                    'tight': r['tight'], 'search_walks': walks[0], 'bisect_steps': steps[0], 'bisect_threshold': res[-1][0], 'bisect_pairs': res[-1][1],
                    'same_answer': res[-1][0] == r['threshold'] and res[-1][1] in (None, r['pairs']),
                    'bisect_over_search': out['bisect_ms'] / out['search_ms']})
        print(json.dumps(out), flush=True)

    box(1, 'one_graph', a.reps, 100000)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', 1, 6400000)


if __name__ == '__main__':
    main()
