#!/usr/bin/env python3
"""Time the negative sampler's partition entries on one device, in one process, in alternating blocks:

    mgv_neg_partition            of another build of the library (--parent-lib PATH: the parent commit's libmgvae_hip.so), when given
    mgv_neg_partition            of this tree
    mgv_neg_partition_local      of this tree at reverse = 0      (the batch's graph table, no reversed slot)
    mgv_neg_partition_local      of this tree at reverse = 0.25

    python tools/bench_neg_local.py --parent-lib /path/to/parent/libmgvae_hip.so
    python tools/bench_neg_local.py --graphs 8 --nodes 65536        # a smaller batch

The batch is config 2's shape: --graphs circuits of --nodes gates (64 x 65,536 = 4,194,304 nodes), --edges random positives inside
the graphs with a fan-out span of 4,096 ids (6,558,720), and the count rule's E - self loops + N slots (10,753,024).  The plan, the
graph table and the workspace are built once by this tree; the parent's library is loaded beside it with ctypes and only its
mgv_neg_partition is called.  Per block and variant: --warmup calls, then --calls calls with HIP events around each; the block's
median.  The report: per variant the median of the block medians and their spread, every local time against the parent's, and whether
the unchanged entry stayed inside the largest block-to-block spread of the parent's own time.  One JSON line at the end."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--graphs', type=int, default=64)
    ap.add_argument('--nodes', type=int, default=65536)
    ap.add_argument('--edges', type=int, default=6558720)
    ap.add_argument('--span', type=int, default=4096)
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated places in the list above (0 = the first line): time these alone, '
                    'e.g. under a kernel trace, where the two local variants share their kernels\' names')
    a = ap.parse_args()

    from deepgate import _hip, sampling
    from deepgate._hip import ptr
    from deepgate.graph_plan import GraphPlan
    dev = torch.device('cuda:0')
    G, n = a.graphs, a.nodes
    N = G * n
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, N, (a.edges,), device=dev, generator=g)
    hop = 1 + torch.randint(0, min(a.span, n - 1), (a.edges,), device=dev, generator=g)
    dst = (src // n) * n + (src % n + hop) % n                # inside the source's graph, never the source itself
    plan = GraphPlan(torch.stack([src, dst]), N)
    plan._check_status()
    E = plan.E - plan.count_self_loops() + N
    shift = sampling.partition_shift(N, E)
    gp_host = torch.arange(G + 1, dtype=torch.int64) * n
    gp, _ = sampling.device_graph_ptr(plan, gp_host)
    i32 = dict(dtype=torch.int32, device=dev)
    n_ws = _hip.call_value('mgv_neg_partition_ws_ints', N, E)
    ws = torch.empty(n_ws, **i32)
    srt = torch.empty(2, E, dtype=torch.int64, device=dev)
    ptrs, out_dst, in_src = torch.empty(2, N + 1, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
    outs = (ptr(srt), ptr(ptrs[0]), ptr(out_dst), ptr(ptrs[1]), ptr(in_src), ptr(ws), n_ws)
    head = (N, E, 0x2545F4914F6CDD1D, shift, ptr(plan.out_ptr), ptr(plan.out_dst))
    print('N = %d (%d graphs of %d), %d positives, E = %d slots, shift %d, %d chunks' % (N, G, n, plan.E, E, shift, -(-E // 16384)))

    def local(rev):
        R = sampling.reverse_count(rev, E)
        return lambda: _hip.call('mgv_neg_partition_local', *head, R, G, ptr(gp), plan.E, ptr(plan.in_src), ptr(plan.in_dst), *outs)

    variants = []
    if a.parent_lib:
        fn = ctypes.CDLL(a.parent_lib).mgv_neg_partition
        fn.argtypes, fn.restype = _hip.parse_header()['mgv_neg_partition'], ctypes.c_int

        def parent():
            rc = fn(*head, *outs, _hip.stream())
            assert rc == 0, rc
        variants.append(('parent mgv_neg_partition', parent))
    variants += [('tree mgv_neg_partition', lambda: _hip.call('mgv_neg_partition', *head, *outs)),
                 ('tree mgv_neg_partition_local reverse 0', local(0.0)),
                 ('tree mgv_neg_partition_local reverse 0.25', local(0.25))]

    if a.only:
        labels = ['parent mgv_neg_partition', 'tree mgv_neg_partition', 'tree mgv_neg_partition_local reverse 0', 'tree mgv_neg_partition_local reverse 0.25']
        keep = {labels[int(k)] for k in a.only.split(',')}
        variants = [v for v in variants if v[0] in keep]
    status = {}
    meds = {name: [] for name, _ in variants}
    for b in range(a.blocks):
        for name, run in variants:
            for _ in range(a.warmup):
                run()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
            for s, e in ev:
                s.record()
                run()
                e.record()
            torch.cuda.synchronize()
            t = sorted(s.elapsed_time(e) for s, e in ev)
            meds[name].append(statistics.median(t))
            status[name] = ws[:4].tolist()
            print('block %d  %-44s %.3f ms  (%.3f .. %.3f)' % (b + 1, name, meds[name][-1], t[0], t[-1]))
    out = {'N': N, 'E': E, 'shift': shift, 'graphs': G}
    for name, m in meds.items():
        out[name] = {'median_ms': statistics.median(m), 'min_ms': min(m), 'max_ms': max(m), 'status': status[name]}
        print('%-46s median %.3f ms (spread %.3f, %.3f .. %.3f)  status %s' % (name, statistics.median(m), max(m) - min(m), min(m), max(m), status[name]))
    if a.parent_lib and not a.only:
        p = out['parent mgv_neg_partition']
        spread = p['max_ms'] - p['min_ms']
        t = out['tree mgv_neg_partition']
        out['unchanged_entry_inside_parent_spread'] = abs(t['median_ms'] - p['median_ms']) <= spread
        print('unchanged entry: %+.3f ms against the parent, the parent\'s spread %.3f' % (t['median_ms'] - p['median_ms'], spread))
        for name in list(meds)[2:]:
            print('%-46s %.3fx the parent\'s mgv_neg_partition' % (name, out[name]['median_ms'] / p['median_ms']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
