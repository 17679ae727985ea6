"""The variational link heads on st [N, 2H]: the fused pair (mgv_var_head_fwd_x3 / mgv_var_head_bwd_x3, ops.VarHeadFn) against the
composed route of the operators it replaces (four ops.linear + two ops.ReparamFn and their backwards), alternated in one process on
the same inputs, through ops.var_head under autograd as the training step calls it.  HIP-event time of forward and backward per
route; then, with --step, the training step on a resident config-2 batch: DG_AE against --variational on either route.

    python tools/bench_var_head.py [--n 4194304] [--reps 5] [--rounds 5] [--step] [--json OUT]
"""
import argparse
import contextlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'multi-gate-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

H = 64
# units of N * 64 * 4 bytes, from the code (var_head_x3.hip's header comment; ISSUE: 16 + 30 chained): forward reads st 2, writes z 2;
# backward reads st 2 and gZ 2, writes dst 2
UNITS = {'fused': (4, 6), 'composed': (16, 30)}


def summary(v):
    v = sorted(v)
    return {'median_ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4)}


def head_pair(a, dev):
    from deepgate import ops
    N = a.n
    g = torch.Generator(device=dev).manual_seed(0)
    st = torch.randn(N, 2 * H, device=dev, generator=g).requires_grad_(True)
    gz = torch.randn(N, 2 * H, device=dev, generator=g)
    gkl = torch.tensor([-0.5 / N, -0.5 / N], device=dev)
    heads = []
    for _ in range(4):
        heads += [(torch.randn(H, H, device=dev, generator=g) * 0.3 / H ** 0.5).requires_grad_(True), torch.zeros(H, device=dev, requires_grad=True)]
    heads = tuple(heads)

    def block(fused):
        ops.VAR_HEAD_FUSED = fused
        tf = tb = 0.0
        for _ in range(a.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            st.grad = None
            for p in heads:
                p.grad = None
            ev[0].record()
            z, kl = ops.var_head(st, heads, seed=7, sample=True)
            ev[1].record()
            torch.autograd.backward([z, kl], [gz, gkl])
            ev[2].record()
            torch.cuda.synchronize()
            tf += ev[0].elapsed_time(ev[1])
            tb += ev[1].elapsed_time(ev[2])
            del z, kl
        return tf / a.reps, tb / a.reps

    for fused in (True, False):
        block(fused)                      # warm-up: library load, function attributes, allocator
    res = {'fused': ([], []), 'composed': ([], [])}
    for _ in range(a.rounds):
        for name, fused in (('composed', False), ('fused', True)):
            f, b = block(fused)
            res[name][0].append(f); res[name][1].append(b)
    ops.VAR_HEAD_FUSED = True
    unit = N * 64 * 4
    out = {'n': N, 'H': H, 'reps': a.reps, 'rounds': a.rounds}
    for name, (f, b) in res.items():
        tot = [x + y for x, y in zip(f, b)]
        o = {'fwd': summary(f), 'bwd': summary(b), 'pair': summary(tot)}
        o['fwd_gbps'] = round(UNITS[name][0] * unit / (o['fwd']['median_ms'] * 1e-3) / 1e9, 1)
        o['bwd_gbps'] = round(UNITS[name][1] * unit / (o['bwd']['median_ms'] * 1e-3) / 1e9, 1)
        out[name] = o
    out['fused_over_composed'] = round(out['fused']['pair']['median_ms'] / out['composed']['pair']['median_ms'], 4)
    out['spread_ms'] = round(max(out[k]['pair']['max_ms'] - out[k]['pair']['min_ms'] for k in ('fused', 'composed')), 4)
    return out


def step_times(a, dev):
    """ms per training step on a resident config-2 batch: the DG_AE step, and the variational step on either route (kl_weight 0.5)."""
    import deepgate
    from deepgate import ops, synthetic as syn
    from deepgate.data import plan_of
    cfg = syn.CONFIGS[2]
    rounds = 4
    arrays = syn.collate(syn.make_graphs(2, batch=cfg['batch'], first_graph=0))
    batch = deepgate.CircuitBatch.from_arrays(arrays, device=dev)
    del batch.neg_edge_index
    trainers = {}
    for name, variational in (('dg_ae', False), ('variational', True)):
        torch.manual_seed(0)
        enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=rounds, t_rounds=rounds, layernorm=True)
        model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H, variational=variational)
        with contextlib.redirect_stdout(sys.stderr):
            trainers[name] = deepgate.Trainer(types.SimpleNamespace(model='DG_AE', kl_weight=0.5), model, training_id='bench_var', save_dir='/tmp/mgv_bench_var',
                                              lr=1e-4, rc_prob_func_weight=[1.0, 4.0, 4.0], device=str(dev), batch_size=cfg['batch'], distributed=False)
        model.train()
    pl = plan_of(batch, [g for _, g in trainers['dg_ae'].model.GATES])
    pl.warm(pl.xcls, quotient_stages=2 * rounds)
    routes = (('dg_ae', 'dg_ae', True), ('variational_fused', 'variational', True), ('variational_composed', 'variational', False))

    def block(tr, fused, steps):
        ops.VAR_HEAD_FUSED = fused
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.enqueue_metrics(tr.train_step(batch))
        tr.flush_metrics()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for _, t, fused in routes:
        block(trainers[t], fused, 3)
    res = {name: [] for name, _, _ in routes}
    for _ in range(a.rounds):
        for name, t, fused in routes:
            res[name].append(block(trainers[t], fused, a.steps))
    ops.VAR_HEAD_FUSED = True
    return {'steps_per_block': a.steps, 'rounds': a.rounds, **{k: summary(v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4194304)
    ap.add_argument('--reps', type=int, default=5, help='forward + backward pairs per timed block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per route, alternated')
    ap.add_argument('--step', action='store_true', help='also time the training step on a resident config-2 batch')
    ap.add_argument('--steps', type=int, default=4, help='steps per timed block of --step')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'head': head_pair(a, dev)}
    torch.cuda.empty_cache()
    if a.step:
        out['step'] = step_times(a, dev)
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
