#!/usr/bin/env python3
"""DiGAE baseline encoder (DirectedGCNConvEncoder, alpha = 1, beta = 0, self loops, 6 -> 64 -> 64) on the config-2 batch
(64 x 65,536-node AIGs): HIP-event time of the encoder forward and of forward + backward, alternating in ONE process

  A  the composition a user could write before these kernels: ops.gather_sum + torch (agg + x) / (deg + 1) + ops.linear + torch ReLU
  B  the new path: class-table first layer, Linear + scaled sum second layer

plus, per launch over the same CSRs: the scaled sum, the class-table layer, the 64 x 64 Linear and k_struct_stage_fwd_x3
(same gather and store, plus a GRU and a LayerNorm), each against its compulsory bytes
2 N H 4 + 4 (N + E) + 8 N as a share of the HBM peak; and the full train step with the AE encoder.

  python tools/bench_digae.py [graphs=64] [iters=20]
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'multi-gate-vae_amd'))
import torch  # noqa: E402

import deepgate  # noqa: E402
from deepgate import _hip, ops, synthetic as syn  # noqa: E402
from deepgate._hip import ptr  # noqa: E402
from deepgate.digae_layer import DirectedGCNConvEncoder  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def time_alternating(fns, iters, warmup=3):
    """{name: median ms}: the variants take turns inside every iteration (clock drift and neighbours hit all of them alike)."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            ev[k].append((s, e))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        t = sorted(s.elapsed_time(e) for s, e in pairs)
        out[k] = (t[len(t) // 2], t[0], t[-1])
    return out


def composition_a(enc, x16, plan):
    """What could be written on the previous kernels: per layer neighbour sum, torch mean with the self loop, Linear, torch ReLU."""
    def layer(conv, h, reverse, relu):
        agg, deg = ops.gather_sum(h, plan=plan, reverse=reverse)
        m = (agg + h) / (deg + 1.0).unsqueeze(1)
        w = conv.lin.weight
        if w.shape[1] != h.shape[1]:
            w = torch.nn.functional.pad(w, (0, h.shape[1] - w.shape[1]))
        y = ops.linear(m, w, conv.lin.bias)
        return torch.relu(y) if relu else y
    s = layer(enc.source_conv.conv2, layer(enc.source_conv.conv1, x16, False, True), True, False)
    t = layer(enc.target_conv.conv2, layer(enc.target_conv.conv1, x16, True, True), False, False)
    return s, t


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device('cuda:0')
    arrays = syn.make_batch(2, batch=B)
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=DirectedGCNConvEncoder(6, 64, 64, 1.0, 0.0, True, False), dim_hidden=64).to(dev).train()
    enc = model.struct_encoder
    plan = deepgate.data.plan_of(batch, [g for _, g in model.GATES])
    N, E, H = plan.N, plan.E, 64
    xcls = plan.xcls
    rows = torch.eye(6, device=dev)
    x16 = torch.nn.functional.pad(rows[xcls.long()], (0, 10)).contiguous()
    ws_, wt_ = torch.randn(N, H, device=dev), torch.randn(N, H, device=dev)
    for rev in (False, True):
        plan.heavy(rev)
    print('N=%d E=%d (config 2, %d graphs), heavy lists: in %d, out %d' % (N, E, B, plan.heavy(False)[0], plan.heavy(True)[0]))

    def new_path():
        return enc(None, None, None, plan=plan, classes=(rows, xcls))

    def fwd(f):
        def g():
            with torch.no_grad():
                f()
        return g

    def fwd_bwd(f):
        def g():
            enc.zero_grad(set_to_none=True)
            s, t = f()
            ((s * ws_).sum() + (t * wt_).sum()).backward()
        return g

    variants = {'A composition': lambda: composition_a(enc, x16, plan), 'B new path': new_path}
    with torch.no_grad():
        sa, ta = variants['A composition']()
        sb, tb = variants['B new path']()
    print('A vs B: max |s| deviation %.2e, max |t| deviation %.2e (scale %.2f)' % (float((sa - sb).abs().max()), float((ta - tb).abs().max()), float(sa.abs().max())))
    res_f = time_alternating({k: fwd(f) for k, f in variants.items()}, iters)
    res_b = time_alternating({k: fwd_bwd(f) for k, f in variants.items()}, iters)
    print('encoder forward            median (min .. max) ms')
    for k, (m, lo, hi) in res_f.items():
        print('  %-24s %8.3f (%.3f .. %.3f)' % (k, m, lo, hi))
    print('encoder forward + backward median (min .. max) ms')
    for k, (m, lo, hi) in res_b.items():
        print('  %-24s %8.3f (%.3f .. %.3f)' % (k, m, lo, hi))

    # ---- single launches over the same CSRs
    h = torch.randn(N, H, device=dev)
    out = torch.empty_like(h)
    W, b = torch.randn(H, H, device=dev) * 0.1, torch.randn(H, device=dev) * 0.1
    T = torch.randn(6, H, device=dev)
    xtab = torch.randn(6, 3 * H, device=dev) * 0.1
    Wc, Whh = torch.randn(3 * H, H, device=dev) * 0.1, torch.randn(3 * H, H, device=dev) * 0.1
    bc, bhh = torch.randn(3 * H, device=dev) * 0.1, torch.randn(3 * H, device=dev) * 0.1
    lw, lb = torch.rand(H, device=dev) + 0.5, torch.randn(H, device=dev) * 0.1
    spack = ops.stage_wpack(Wc, Whh)
    stats = torch.empty(N, 2, device=dev)
    launches = {}
    for rev in (False, True):
        p, i = plan.csr(rev)
        r, c = ops.digcn_scales(plan, rev, 1.0, 0.0, True)
        tag = 'out-CSR' if rev else 'in-CSR'
        hn, hnodes = plan.heavy(rev)
        hws = ops.workspace(max(2 * hn * H, 1), dev)
        launches['scaled sum %s' % tag] = (lambda p=p, i=i, r=r, c=c, hn=hn, hnodes=hnodes: _hip.call(
            'mgv_digcn_gather', H, N, ptr(h), ptr(p), ptr(i), ptr(r), ptr(c), None, 1, 1, hn, ptr(hnodes) if hn else None, ptr(out)))
        launches['class layer %s' % tag] = (lambda p=p, i=i, r=r, c=c: _hip.call(
            'mgv_digcn_class_fwd', H, N, ptr(xcls), ptr(T), 6, ptr(p), ptr(i), ptr(r), ptr(c), 1, 1, ptr(out)))
        launches['struct stage fwd x3 %s' % tag] = (lambda p=p, i=i, hn=hn, hnodes=hnodes: _hip.call(
            'mgv_struct_stage_fwd_x3', H, N, ptr(h), ptr(p), ptr(i), ptr(xcls), ptr(xtab), 6, ptr(spack), ptr(bc), ptr(bhh), ptr(lw), ptr(lb), 1e-5,
            ptr(out), hn, ptr(hnodes) if hn else None, ptr(hws) if hn else None, None, 0, ptr(stats)))
    launches['linear 64x64 x3'] = lambda: ops._lin_fwd(h, None, W, b, H)
    res_l = time_alternating(launches, iters)
    full = 2 * N * H * 4 + 4 * (N + E) + 8 * N          # rows in, rows out, the CSR, the two scales
    cls_bytes = N * H * 4 + 4 * (N + E) + 8 * N + N + E  # no rows in: one class byte per list entry and per node
    print('per launch                     median ms   compulsory MB   share of %.1f TB/s' % (HBM_PEAK / 1e12))
    for k, (m, lo, hi) in res_l.items():
        by = cls_bytes if k.startswith('class') else (2 * N * H * 4 if k.startswith('linear') else full)
        print('  %-28s %8.3f (%.3f .. %.3f) %10.1f %10.1f %%' % (k, m, lo, hi, by / 1e6, 100.0 * by / (m * 1e-3) / HBM_PEAK))

    # ---- the whole train step with the AE encoder
    tr = deepgate.Trainer(types.SimpleNamespace(model='AE'), model, training_id='bench_ae', save_dir='/tmp/mgv_bench_ae', lr=1e-4,
                          rc_prob_func_weight=[1.0, 4.0, 4.0], device='cuda:0', batch_size=B, distributed=False)
    res_s = time_alternating({'train_step (AE encoder)': lambda: tr.train_step(batch)}, max(iters // 2, 5))
    m, lo, hi = res_s['train_step (AE encoder)']
    print('train_step with the AE encoder:  %.2f ms median (%.2f .. %.2f), %.0f graphs/s' % (m, lo, hi, B / (m * 1e-3)))


if __name__ == '__main__':
    main()
