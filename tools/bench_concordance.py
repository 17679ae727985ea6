#!/usr/bin/env python3
"""Time the comparison-count entry (mgv_concord_counts of csrc/concordance.hip, ops.concord_counts) against a chunked torch route on
the same device, in the same process, and compare the integer counts of the two.

    python tools/bench_concordance.py                      # one 65,536-node graph (16,384 listed pairs) and a config-2 batch of 64
    python tools/bench_concordance.py --skip-batch

gt   : the truth-table distances of a synthetic AIG's listed pairs (synthetic.make_graph), repeated per graph of the batch
pred : gt + 0.2 randn in float32, a quarter of the entries copied from others (ties in the prediction)
hip  : ops.concord_counts on the segment table, B = 1 (gap 0.05) and B = 8 (0, 0.05, 0.1 .. 0.35)
torch: per circuit and per --chunk rows of its comparison matrix, dd = gt[None, :] - gt[rows, None] and de likewise as dense float32
       blocks, the upper-triangle mask from two aranges, and per gap three masked sums (a P x P boolean block per chunk and gap)
One process; a warm-up of both routes first; then --reps rounds that time the two routes ALTERNATELY with HIP events around the device
work; medians.  Prints one JSON line per case and B; its `*_gap0` keys refer to the first gap of the list (0.05 at B = 1, 0 at B = 8)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GAPS = {1: (0.05,), 8: (0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35)}


def torch_counts(gt, pred, seg, gaps32, chunk):
    """int64 [G, B, 3] by dense blocks; seg a host list."""
    dev = gt.device
    out = torch.zeros((len(seg) - 1, gaps32.numel(), 3), dtype=torch.int64, device=dev)
    for g in range(len(seg) - 1):
        a, b = gt[seg[g]:seg[g + 1]], pred[seg[g]:seg[g + 1]]
        n = a.numel()
        col = torch.arange(n, device=dev)
        for r0 in range(0, n, chunk):
            r1 = min(r0 + chunk, n)
            dd = a[None, :] - a[r0:r1, None]
            de = b[None, :] - b[r0:r1, None]
            live = (col[None, :] > col[r0:r1, None]) & (dd != 0)
            conc = ((dd > 0) & (de > 0)) | ((dd < 0) & (de < 0))
            tied = de == 0
            ad = dd.abs()
            for j in range(gaps32.numel()):
                el = live & (ad >= gaps32[j])
                out[g, j, 0] += el.sum()
                out[g, j, 1] += (el & conc).sum()
                out[g, j, 2] += (el & tied).sum()
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import ops, synthetic
    dev = torch.device('cuda:0')
    n = a.graph_n
    graph = synthetic.make_graph('aig', n, 63, 900, n_inputs=n // 64)
    gt1 = torch.as_tensor(np.asarray(graph['tt_sim'], dtype=np.float32)).to(dev)
    P1 = gt1.numel()
    g = torch.Generator(device=dev).manual_seed(0)
    pred1 = gt1 + 0.2 * torch.randn(P1, generator=g, device=dev)
    idx = torch.randint(0, P1, (P1 // 4,), generator=g, device=dev)
    pred1[idx] = pred1[torch.randint(0, P1, (P1 // 4,), generator=g, device=dev)]

    def box(graphs, tag, reps):
        gt, pred = gt1.repeat(graphs), pred1.repeat(graphs)
        seg = [k * P1 for k in range(graphs + 1)]
        sp = torch.tensor(seg, dtype=torch.int32, device=dev)
        for B, gaps in GAPS.items():
            g32 = torch.tensor(gaps, dtype=torch.float32, device=dev)
            hip = lambda: ops.concord_counts(gt, pred, sp, gaps)             # noqa: E731
            ref = lambda: torch_counts(gt, pred, seg, g32, a.chunk)           # noqa: E731
            hip(), ref()
            torch.cuda.synchronize()
            hip_ms, torch_ms = [], []
            for _ in range(reps):
                ms, got = event_ms(hip)
                hip_ms.append(ms)
                ms, want = event_ms(ref)
                torch_ms.append(ms)
            med = lambda v: sorted(v)[len(v) // 2]                            # noqa: E731
            el = got[:, :, 0].double()
            print(json.dumps({'case': tag, 'graphs': graphs, 'pairs_per_graph': P1, 'P': gt.numel(), 'B': B,
                              'comparisons': graphs * P1 * (P1 - 1) // 2, 'hip_ms': med(hip_ms), 'torch_chunked_ms': med(torch_ms),
                              'hip_ms_all': hip_ms, 'torch_ms_all': torch_ms, 'torch_over_hip': med(torch_ms) / med(hip_ms),
                              'counts_equal': bool(torch.equal(got, want)), 'eligible_gap0': int(got[:, 0, 0].sum()),
                              'mean_accuracy_gap0': float((got[:, 0, 1].double() / el[:, 0].clamp(min=1)).mean())}), flush=True)

    box(1, 'one_graph', a.reps)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', max(1, a.reps // 2))


if __name__ == '__main__':
    main()
