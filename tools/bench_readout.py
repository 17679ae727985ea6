"""Readout MLP (pred_prob: 64 -> 32 -> 32 -> 1, training mode) forward + backward, fused (ops.ReadoutMLPFn) against the per-layer
path (linear / BnReluDropFn / HeadFn), alternated in one process on the same inputs.  HIP-event time per forward + backward.

    python tools/bench_readout.py [--n 4194304] [--reps 30] [--rounds 5] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'multi-gate-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4194304)
    ap.add_argument('--reps', type=int, default=30, help='forward + backward passes per timed block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per path, alternated')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from deepgate import ops
    from deepgate.arch import mlp as mlp_mod
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = mlp_mod.MLP(64, 32, 1, num_layer=3, p_drop=0.2, norm_layer='batchnorm', act_layer='relu').to(dev).train()
    hf = torch.randn(a.n, 64, device=dev).requires_grad_(True)
    target = torch.rand(a.n, 1, device=dev)

    def one():
        hf.grad = None
        m.zero_grad(set_to_none=True)
        ops.l1_loss(m(hf, clamp01=True, seed=1), target).backward()

    def block(fused):
        mlp_mod.FUSED_READOUT = fused
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.reps):
            one()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.reps

    for fused in (False, True):           # warm-up: library load, workspaces, allocator
        mlp_mod.FUSED_READOUT = fused
        for _ in range(3):
            one()
    # the L1 loss (forward + backward) is in both; time it alone to report the readout's own share
    prob = torch.rand(a.n, 1, device=dev).requires_grad_(True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        prob.grad = None
        ops.l1_loss(prob, target).backward()
    e1.record()
    torch.cuda.synchronize()
    l1_ms = e0.elapsed_time(e1) / a.reps
    res = {'per_layer': [], 'fused': []}
    for _ in range(a.rounds):
        res['per_layer'].append(block(False))
        res['fused'].append(block(True))
    out = {'n': a.n, 'reps': a.reps, 'l1_loss_ms': round(l1_ms, 4)}
    for k, v in res.items():
        v = sorted(v)
        out[k + '_ms'] = [round(x, 4) for x in v]
        out[k + '_median_ms'] = round(v[len(v) // 2], 4)
    out['saving_ms'] = round(out['per_layer_median_ms'] - out['fused_median_ms'], 4)
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
