"""Backward of the two Linears at the seam between the losses and the encoders, through the C ABI: the fused launch
(mgv_linear_bwd_x3) against the separate launches it replaces (mgv_linear_wgrad_x3 + one mgv_linear_fwd_x3(_res) per input),
alternated in one process on the same inputs.  HIP-event time per backward, and GB/s against each route's own byte count.

  hs_linear     (M, K) = (64, 128): X1 | X2 two 64-column inputs, two input gradients, no residual
  hs_decompose  (M, K) = (128, 64): one input, the level sweep's gradient as residual

    python tools/bench_linear_bwd.py [--n 4194304] [--reps 20] [--rounds 5] [--json OUT]
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

# units of N * 64 * 4 bytes moved per backward: (separate, fused)
#   hs_linear:    wgrad reads dY 1 + X 2, two dgrads read dY 1 and write 1 each | fused reads dY 1 + X 2, writes 2
#   hs_decompose: wgrad reads dY 2 + X 1, the dgrad reads dY 2 + R 1, writes 1  | fused reads dY 2 + X 1 + R 1, writes 1
CASES = {'hs_linear': (64, 128, False, 7, 5), 'hs_decompose': (128, 64, True, 7, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4194304)
    ap.add_argument('--reps', type=int, default=20, help='backward passes per timed block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per route, alternated')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from deepgate import _hip as h, ops
    p = h.ptr
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    N = a.n
    out = {'n': N, 'reps': a.reps}
    for name, (M, K, with_res, u_sep, u_fused) in CASES.items():
        K1 = 64
        K2 = K - K1
        X1 = torch.randn(N, K1, device=dev)
        X2 = torch.randn(N, K2, device=dev) if K2 else None
        dY = torch.randn(N, M, device=dev)
        R = torch.randn(N, K1, device=dev) if with_res else None
        W = torch.randn(M, K, device=dev) / K ** 0.5
        dW, db = torch.zeros(M, K, device=dev), torch.zeros(M, device=dev)
        dX1 = torch.empty(N, K1, device=dev)
        dX2 = torch.empty(N, K2, device=dev) if K2 else None
        packs = []
        for Wv in (W, W[:, :K1], W[:, K1:]):
            if Wv.shape[1]:
                pk = torch.empty(2 * Wv.numel(), dtype=torch.bfloat16, device=dev)
                ops._pack_into(pk, 0, Wv, True)
                packs.append(pk)
        nws = h.call_value('mgv_linear_wgrad_x3_ws_floats', M, K, N)
        ws = torch.empty(nws, device=dev)
        xargs = (p(X1), K1, K1, p(X2), K2, K2)

        def separate():
            h.call('mgv_linear_wgrad_x3', N, *xargs, p(dY), M, M, p(dW), p(db), p(ws), nws)
            if with_res:
                h.call('mgv_linear_fwd_x3_res', N, p(dY), M, M, None, 0, 0, p(packs[1]), None, K1, p(R), K1, p(dX1), K1)
            else:
                h.call('mgv_linear_fwd_x3', N, p(dY), M, M, None, 0, 0, p(packs[1]), None, K1, p(dX1), K1)
            if K2:
                h.call('mgv_linear_fwd_x3', N, p(dY), M, M, None, 0, 0, p(packs[2]), None, K2, p(dX2), K2)

        def fused():
            h.call('mgv_linear_bwd_x3', N, *xargs, p(dY), M, M, p(packs[0]), p(dW), p(db), p(dX1), K1, p(dX2), K2, p(R), K1 if with_res else 0,
                   p(ws), nws)

        def block(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / a.reps

        for fn in (separate, fused):          # warm-up: library load, function attributes
            for _ in range(3):
                fn()
        res = {'separate': [], 'fused': []}
        for _ in range(a.rounds):
            res['separate'].append(block(separate))
            res['fused'].append(block(fused))
        unit = N * 64 * 4
        o = {'shape': [M, K], 'residual': with_res}
        for k, units in (('separate', u_sep), ('fused', u_fused)):
            v = sorted(res[k])
            o[k + '_ms'] = [round(x, 4) for x in v]
            o[k + '_median_ms'] = round(v[len(v) // 2], 4)
            o[k + '_units'] = units
            o[k + '_gbps'] = round(units * unit / (v[len(v) // 2] * 1e-3) / 1e9, 1)
        o['saving_ms'] = round(o['separate_median_ms'] - o['fused_median_ms'], 4)
        o['spread_ms'] = round(max(max(res[k]) - min(res[k]) for k in res), 4)
        out[name] = o
        del X1, X2, dY, R, dX1, dX2
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
