#!/usr/bin/env python3
"""Time the device ranking of link-prediction scores (csrc/link_metrics.hip) against the route it replaces.

    python tools/bench_link_metrics.py                     # config 2's pair counts, random pairs, H = 64
    python tools/bench_link_metrics.py --val-phase         # + a val phase of resident config-2 batches with / without the ranking
    python tools/bench_link_metrics.py --pos 100000 --neg 170000 --nodes 65536      # any other size

One process; warm-up first; HIP events around each phase of the device path (score keys, rocPRIM radix sort — a library call —,
rank pass), a device synchronise before every host clock read.  The host route is the reference's (digvae_model.py:177-189):
decode both edge sets, copy the scores to the host, rank them there (the numpy restatement the tests use, and sklearn where it is
installed).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def device_phases(ops, _hip, st, pos, neg, reps):
    """Per-phase device times (ms, median of `reps`) of one ranking, through the C ABI as ops.link_record calls it."""
    ptr = _hip.ptr
    dev = st.device
    H = st.shape[1] // 2
    P, Q = pos.shape[1], neg.shape[1]
    n = P + Q
    ps, pd, ns, nd = pos[0].contiguous(), pos[1].contiguous(), neg[0].contiguous(), neg[1].contiguous()
    rec = torch.zeros(8, dtype=torch.float64, device=dev)
    buf = torch.empty(3, n + (-n) % 4, dtype=torch.int32, device=dev)
    keys, skey, order = buf[0, :n], buf[1, :n], buf[2, :n]
    t_i, w_i = _hip.call_value('mgv_sort_pairs_temp_ints', 4, n), _hip.call_value('mgv_link_rank_work_ints', n)
    temp = torch.empty(t_i + w_i + 2, dtype=torch.int32, device=dev)
    work = temp[t_i + (t_i & 1):]
    status = rec.view(torch.int32)[12:13]
    rows = []
    for _ in range(reps + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _hip.call('mgv_link_keys', H, ptr(st), ptr(st[:, H:]), 2 * H, ptr(ps), ptr(pd), P, ptr(ns), ptr(nd), Q, ptr(keys), None, ptr(status))
        ev[1].record()
        _hip.call('mgv_sort_pairs', 4, n, ptr(keys), ptr(skey), ptr(order), 32, ptr(temp), t_i)
        ev[2].record()
        _hip.call('mgv_link_rank', n, P, ptr(skey), ptr(order), ptr(rec), ptr(work), work.numel())
        ev[3].record()
        torch.cuda.synchronize()
        rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)] + [ev[0].elapsed_time(ev[3])])
    med = np.median(np.array(rows[2:]), axis=0)
    return {'keys_ms': float(med[0]), 'sort_rocprim_ms': float(med[1]), 'rank_ms': float(med[2]), 'total_ms': float(med[3]),
            'work_bytes': int(4 * (buf.numel() + temp.numel())), 'auc': float(rec[0]), 'ap': float(rec[1])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--pos', type=int, default=6558720)
    ap.add_argument('--neg', type=int, default=10753024)
    ap.add_argument('--nodes', type=int, default=4194304)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the host route')
    ap.add_argument('--val-phase', action='store_true', help='also time eval steps of a resident BASELINE config-2 batch with / without the ranking')
    ap.add_argument('--val-batches', type=int, default=10)
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    from deepgate.digae_layer import DirectedInnerProductDecoder
    dev = torch.device('cuda:0')
    H = 64
    g = torch.Generator(device=dev).manual_seed(0)
    st = 0.3 * torch.randn(a.nodes, 2 * H, generator=g, device=dev)
    pos = torch.randint(0, a.nodes, (2, a.pos), generator=g, device=dev)
    neg = torch.randint(0, a.nodes, (2, a.neg), generator=g, device=dev)
    out = {'P': a.pos, 'Q': a.neg, 'nodes': a.nodes, 'H': H}
    out['device'] = device_phases(ops, _hip, st, pos, neg, a.reps)
    # the whole op as a caller sees it (allocations included), host clock around a synchronised call
    for _ in range(2):
        ops.link_record(st, None, pos, neg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        rec = ops.link_record(st, None, pos, neg)
    torch.cuda.synchronize()
    out['device']['op_wall_ms'] = (time.perf_counter() - t0) * 1e3 / a.reps
    if not a.no_host:
        from link_metrics_ref import rank_stats
        s, t = st[:, :H].contiguous(), st[:, H:].contiguous()
        dec = DirectedInnerProductDecoder()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            scores = torch.cat([dec(s, t, pos, sigmoid=True).cpu(), dec(s, t, neg, sigmoid=True).cpu()]).numpy()
        t1 = time.perf_counter()
        r = rank_stats(scores, a.pos)
        t2 = time.perf_counter()
        host = {'decode_and_copy_ms': (t1 - t0) * 1e3, 'numpy_rank_ms': (t2 - t1) * 1e3, 'auc': r['auc'], 'ap': r['ap']}
        try:
            from sklearn import metrics
            y = np.concatenate([np.ones(a.pos, dtype=np.float32), np.zeros(a.neg, dtype=np.float32)])
            t3 = time.perf_counter()
            sk = (metrics.roc_auc_score(y, scores), metrics.average_precision_score(y, scores))
            host['sklearn_rank_ms'] = (time.perf_counter() - t3) * 1e3
            host['sklearn_auc'], host['sklearn_ap'] = float(sk[0]), float(sk[1])
        except ImportError:
            host['sklearn_rank_ms'] = None
        out['host_route'] = host
        out['agree'] = {'auc_diff': abs(float(rec[0]) - r['auc']), 'ap_diff': abs(float(rec[1]) - r['ap'])}
    del st, pos, neg
    if a.val_phase:
        import deepgate
        from deepgate import synthetic as syn
        batch = deepgate.CircuitBatch.from_arrays(syn.make_batch(2), device=dev)
        del batch.neg_edge_index                 # negatives sampled on the device, as in training
        torch.manual_seed(0)
        enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=4, t_rounds=4, layernorm=True)
        model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H)
        tr = deepgate.Trainer(types.SimpleNamespace(model='DG_AE'), model, training_id='bench_link', save_dir='/tmp/mgv_bench_link', lr=1e-4,
                              device='cuda:0', batch_size=64, distributed=False)
        model.eval()
        res = {}
        with torch.no_grad():
            for tag, kw in (('plain', {}), ('val_auc', {'want_rank': True}), ('plain_again', {})):
                for _ in range(2):
                    tr.run_batch(batch, want_pred=False, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                recs = [tr.run_batch(batch, want_pred=False, **kw).get('link_metrics') for _ in range(a.val_batches)]
                if kw:
                    ops.read_link_records(recs)          # the phase's single host read
                torch.cuda.synchronize()
                res[tag + '_ms_per_batch'] = (time.perf_counter() - t0) * 1e3 / a.val_batches
        res['added_ms_per_batch'] = res['val_auc_ms_per_batch'] - 0.5 * (res['plain_ms_per_batch'] + res['plain_again_ms_per_batch'])
        res['added_share_of_eval_step'] = res['added_ms_per_batch'] / (0.5 * (res['plain_ms_per_batch'] + res['plain_again_ms_per_batch']))
        out['val_phase_config2'] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
