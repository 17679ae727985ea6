#!/usr/bin/env python3
"""Time the candidate classes (mgv_sim_union of csrc/pair_scores.hip, the union-find and class table of csrc/components.hip,
ops.sim_classes on both routes) against the symmetric count on the same rows (mgv_sim_select_count: the same tiles without the unions) and
against the host route they replace, on the same device, in the same process.

    python tools/bench_components.py                       # one 65,536-node graph and a config-2 batch of 64 such graphs
    python tools/bench_components.py --skip-batch

H = 64, rows and the two regimes of tools/bench_similarity.py (clusters of 9 at threshold 0.999; the 0.99 quantile of a sample of the
cosines: about 1 % of the pairs, where nearly every pair is redundant for the classes).
count      : mgv_sim_select_count                          union : mgv_sim_union on a freshly initialised forest (mgv_cc_init not timed),
             the two timed alternately, call by call
walk       : ops.sim_classes(route='walk')  (unit rows, init, union, labels, class table, one read-back)
pairs      : ops.sim_classes(route='pairs') (unit rows, count, scan, read-back, fill, pair_index, union over the list, labels, table);
             skipped with its reason where sim_pairs refuses or the list passes --max-list pairs
host       : ops.sim_pairs -> .cpu() -> min-label propagation with pointer jumping in numpy -> classes; skipped above --max-host pairs
One process; every shape warmed up first; HIP events around the device work (wall clock for the host route), median of --reps.
Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT, os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_similarity import _once, clustered_rows, timed  # noqa: E402


def host_labels(pairs, N):
    """Components on the host: min-label propagation with pointer jumping (numpy; scipy is not assumed)."""
    a, b = pairs[0], pairs[1]
    label = np.arange(N, dtype=np.int64)
    while True:
        m = np.minimum(label[a], label[b])
        new = label.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-batch', action='store_true')
    ap.add_argument('--max-list', type=int, default=400_000_000, help='route=\'pairs\' is not timed above this many pairs')
    ap.add_argument('--max-host', type=int, default=40_000_000, help='the host route is not timed above this many pairs')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H = 64
    g = torch.Generator(device=dev).manual_seed(0)

    def box(graphs, tag, reps):
        n = a.graph_n
        N = graphs * n
        x = clustered_rows(graphs, n, H, g, dev)
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        y = ops.row_unit(x)
        m = min(2048, n)
        sample = torch.mm(y[:m], y[:m].T).flatten()
        dense = float(sample.kthvalue(int(0.99 * sample.numel())).values)
        del sample
        for regime, thr in (('sparse', 0.999), ('dense', dense)):
            sym = (H, N, ptr(y), H, ptr(gp), graphs, thr)
            n_sym = torch.empty(N, dtype=torch.int32, device=dev)
            parent = torch.empty(N, dtype=torch.int32, device=dev)
            status = torch.empty(4, dtype=torch.int32, device=dev)

            def count():
                _hip.call('mgv_sim_select_count', *sym, ptr(n_sym))

            def union_once():
                _hip.call('mgv_cc_init', N, ptr(parent), ptr(status))
                torch.cuda.synchronize()
                return _once(lambda: _hip.call('mgv_sim_union', *sym, ptr(parent), ptr(status)))
            count()
            union_once()
            mc, mu = [], []
            for _ in range(reps):
                mc.append(_once(count))
                mu.append(union_once())
            count_ms, union_ms = sorted(mc)[reps // 2], sorted(mu)[reps // 2]
            assert status.tolist() == [0, 0, 0, 0], status.tolist()
            pairs = int(n_sym.sum(dtype=torch.int64))
            walk_ms = timed(lambda: ops.sim_classes(x, graph_ptr=gp, threshold=thr), reps)
            label, class_ptr, members = ops.sim_classes(x, graph_ptr=gp, threshold=thr)
            out = {'case': '%s_%s' % (tag, regime), 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'threshold': thr, 'pairs': pairs,
                   'pairs_per_row': pairs / N, 'classes': class_ptr.numel() - 1, 'members': members.numel(),
                   'largest_class': int((class_ptr[1:] - class_ptr[:-1]).max()) if class_ptr.numel() > 1 else 0,
                   'count_ms': count_ms, 'union_ms': union_ms, 'union_over_count': union_ms / count_ms, 'walk_ms': walk_ms,
                   'pairs_ms': None, 'pairs_skipped': None, 'host_ms': None, 'host_skipped': None}
            if pairs > a.max_list:
                out['pairs_skipped'] = 'more than --max-list pairs'
            else:
                try:
                    out['pairs_ms'] = timed(lambda: ops.sim_classes(x, graph_ptr=gp, threshold=thr, route='pairs'), reps)
                    via = ops.sim_classes(x, graph_ptr=gp, threshold=thr, route='pairs')
                    out['routes_agree'] = all(torch.equal(p, q) for p, q in zip((label, class_ptr, members), via))
                    out['walk_over_pairs'] = walk_ms / out['pairs_ms']
                    del via
                except _hip.HipLibraryError as e:
                    out['pairs_skipped'] = str(e)[:120]
            if pairs > a.max_host or out['pairs_ms'] is None:
                out['host_skipped'] = 'more than --max-host pairs' if pairs > a.max_host else 'no pair list'
            else:
                def host():
                    pi = ops.sim_pairs(x, graph_ptr=gp, threshold=thr)[0].cpu().numpy()
                    return host_labels(pi, N)
                host()
                ts = []
                for _ in range(max(1, reps // 2)):
                    t0 = time.perf_counter()
                    hl = host()
                    ts.append((time.perf_counter() - t0) * 1e3)
                out['host_ms'] = sorted(ts)[len(ts) // 2]
                out['host_agrees'] = bool(np.array_equal(hl, label.cpu().numpy().astype(np.int64)))
                out['host_over_walk'] = out['host_ms'] / walk_ms
            print(json.dumps(out), flush=True)

    box(1, 'one_graph', a.reps)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', 1)


if __name__ == '__main__':
    main()
