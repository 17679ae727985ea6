#!/usr/bin/env python3
"""Time the all-pairs decoder entries (csrc/pair_scores.hip) against the torch routes on the same device.

    python tools/bench_pair_scores.py                      # dense N = 16,384; top-k at one 65,536-node graph and at a config-2 batch
    python tools/bench_pair_scores.py --skip-batch         # without the 64 x 65,536-node batch

dense : mgv_pair_scores_fwd (sigmoid, H = 64, a 1 GiB output)           baseline torch.sigmoid(s @ t.T)
top-k : mgv_pair_topk (k = 8, sigmoid, threshold 0.5)                   baseline (s[blk] @ t.T).topk(8) per 4,096 rows of each graph
One process; warm-up first; HIP events around the device work, median of --reps; operands 0.3 randn.  The arithmetic floor printed with
each line is 2 N^2 H flop (per graph) at the 157 TF/s fp32-matrix peak.  Prints one JSON line per case."""
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
    ap.add_argument('--dense-n', type=int, default=16384)
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H, K = 64, 8
    g = torch.Generator(device=dev).manual_seed(0)

    # ---- dense
    n = a.dense_n
    st = 0.3 * torch.randn(n, 2 * H, generator=g, device=dev)
    s, t = st[:, :H], st[:, H:]
    out = torch.empty(n, n, device=dev)
    hip = timed(lambda: _hip.call('mgv_pair_scores_fwd', H, n, n, ptr(s), 2 * H, ptr(t), 2 * H, 1, ptr(out), n), a.reps)
    sc, tc = s.contiguous(), t.contiguous()
    ref = torch.empty(n, n, device=dev)

    def torch_dense():
        torch.mm(sc, tc.T, out=ref)
        torch.sigmoid_(ref)
    base = timed(torch_dense, a.reps)
    diff = float((out - ref).abs().max())
    print(json.dumps({'case': 'dense', 'N': n, 'H': H, 'out_GiB': 4.0 * n * n / 2 ** 30, 'hip_ms': hip, 'torch_ms': base, 'torch_over_hip': base / hip,
                      'mfma_floor_ms': 2.0 * n * n * H / PEAK_F32_MATRIX * 1e3, 'max_abs_diff': diff}))
    del out, ref, st, s, t, sc, tc

    # ---- top-k
    def topk_case(graphs, tag, reps):
        N = graphs * a.graph_n
        st = 0.3 * torch.randn(N, 2 * H, generator=g, device=dev)
        s, t = st[:, :H], st[:, H:]
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * a.graph_n
        idx = torch.empty(N, K, dtype=torch.int32, device=dev)
        score = torch.empty(N, K, device=dev)
        na = torch.empty(N, dtype=torch.int32, device=dev)
        hip = timed(lambda: _hip.call('mgv_pair_topk', H, N, ptr(s), 2 * H, ptr(t), 2 * H, ptr(gp), graphs, K, 1, 0.5, 0, ptr(idx), ptr(score),
                                      ptr(na)), reps)
        sc, tc = s.contiguous(), t.contiguous()
        ridx = torch.empty(N, K, dtype=torch.int64, device=dev)

        def torch_chunks():
            for gi in range(graphs):
                lo = gi * a.graph_n
                tg = tc[lo:lo + a.graph_n].T
                for b0 in range(lo, lo + a.graph_n, 4096):
                    ridx[b0:b0 + 4096] = torch.mm(sc[b0:b0 + 4096], tg).topk(K).indices + lo
        base = timed(torch_chunks, max(1, reps // 2 if graphs > 1 else reps))
        same = float((ridx == idx.long()).float().mean())
        print(json.dumps({'case': tag, 'graphs': graphs, 'nodes_per_graph': a.graph_n, 'N': N, 'H': H, 'k': K, 'hip_ms': hip, 'torch_chunked_ms': base,
                          'torch_over_hip': base / hip, 'mfma_floor_ms': 2.0 * graphs * a.graph_n ** 2 * H / PEAK_F32_MATRIX * 1e3,
                          'indices_equal_to_torch_share': same}))

    topk_case(1, 'topk_one_graph', a.reps)
    if not a.skip_batch:
        topk_case(a.batch_graphs, 'topk_config2_batch', 1)


if __name__ == '__main__':
    main()
