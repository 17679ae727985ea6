#!/usr/bin/env python3
"""Time the fan-in decode (mgv_fanin_decode, csrc/pair_scores.hip) against mgv_pair_topk on the same batch and against a chunked torch
route on the same device.

    python tools/bench_fanin_decode.py                      # one 65,536-node graph and a config-2 batch (64 such graphs)
    python tools/bench_fanin_decode.py --skip-batch         # without the batch

H = 64, K = 3, every node wants 3.  Keys: ascending with the node id inside each graph (a levelised netlist in topological order), and
the same keys shuffled inside each graph.  Each way with and without tile_min (the per-tile key minima by which a workgroup steps over
column tiles that hold no candidate).
  pair_topk : mgv_pair_topk at k = 3 with the operands swapped (rows = targets), raw scores: the same walk without the key.
  torch     : per graph and 4,096 target rows: dense scores, masked_fill of the columns whose key is not below the row's, topk(3).
One process; warm-up first; HIP events around the device work, median of --reps; operands 0.3 randn.  The arithmetic floor printed with
each line is 2 N^2 H flop (per graph) at the 157 TF/s fp32-matrix peak, for the WHOLE square; ascending keys need half of it.  Prints one
JSON line per case."""
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
    from deepgate import _hip
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H, K = 64, 3
    g = torch.Generator(device=dev).manual_seed(0)

    def case(graphs, tag, reps):
        n = a.graph_n
        N = graphs * n
        st = 0.3 * torch.randn(N, 2 * H, generator=g, device=dev)
        s, t = st[:, :H], st[:, H:]
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        want = torch.full((N,), K, dtype=torch.int32, device=dev)
        local = torch.arange(n, dtype=torch.int32, device=dev)
        keys = {'ascending': local.repeat(graphs),
                'shuffled': torch.cat([local[torch.randperm(n, generator=g, device=dev)] for _ in range(graphs)])}
        idx = torch.empty(N, K, dtype=torch.int32, device=dev)
        score = torch.empty(N, K, device=dev)
        nc = torch.empty(N, dtype=torch.int32, device=dev)
        tile_min = torch.empty((N + 63) // 64, dtype=torch.int32, device=dev)
        # rows = targets: t is the row operand, s the column operand
        topk = timed(lambda: _hip.call('mgv_pair_topk', H, N, ptr(t), 2 * H, ptr(s), 2 * H, ptr(gp), graphs, K, 0, 0.0, 0, ptr(idx), ptr(score),
                                       ptr(nc)), reps)
        sc, tc = s.contiguous(), t.contiguous()
        ridx = torch.empty(N, K, dtype=torch.int64, device=dev)
        for kname, key in keys.items():
            ms = {}
            for skip in (False, True):
                ms[skip] = timed(lambda: _hip.call('mgv_fanin_decode', H, N, ptr(t), 2 * H, ptr(s), 2 * H, ptr(gp), graphs, ptr(key), ptr(want), K,
                                                   ptr(tile_min) if skip else None, ptr(idx), ptr(score), ptr(nc)), reps)

            def torch_chunks():
                for gi in range(graphs):
                    lo = gi * n
                    sg, kg = sc[lo:lo + n].T, key[lo:lo + n]
                    for b0 in range(lo, lo + n, 4096):
                        d = torch.mm(tc[b0:b0 + 4096], sg)
                        d.masked_fill_(kg[None, :] >= key[b0:b0 + 4096, None], float('-inf'))
                        ridx[b0:b0 + 4096] = d.topk(K).indices + lo
            base = timed(torch_chunks, max(1, reps // 2 if graphs > 1 else reps))
            full = nc >= K                                   # rows with fewer candidates list -1 where torch lists masked columns
            same = float((ridx[full] == idx[full].long()).float().mean())
            print(json.dumps({'case': tag, 'keys': kname, 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'K': K,
                              'fanin_ms': ms[False], 'fanin_tile_min_ms': ms[True], 'plain_over_tile_min': ms[False] / ms[True],
                              'pair_topk_k3_ms': topk, 'fanin_over_pair_topk': ms[False] / topk, 'tile_min_over_pair_topk': ms[True] / topk,
                              'torch_chunked_ms': base, 'torch_over_fanin_tile_min': base / ms[True],
                              'mfma_floor_full_square_ms': 2.0 * graphs * n ** 2 * H / PEAK_F32_MATRIX * 1e3,
                              'indices_equal_to_torch_share': same}))

    case(1, 'one_graph', a.reps)
    if not a.skip_batch:
        case(a.batch_graphs, 'config2_batch', 1)


if __name__ == '__main__':
    main()
