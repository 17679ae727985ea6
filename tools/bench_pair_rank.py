#!/usr/bin/env python3
"""Time the rank entry (mgv_pair_rank_counts of csrc/pair_scores.hip, ops.link_ranks) against mgv_pair_select_count at one threshold —
the floor: the same walk with no lists — and against the chunked torch route on the same device, in the same process.

    python tools/bench_pair_rank.py                      # one 65,536-node graph and a config-2 batch of 64 such graphs
    python tools/bench_pair_rank.py --skip-batch

All true links of a synthetic AIG, ranked by target (every true fan-in of a gate among all gates of its circuit), H = 64, two inputs:
  fitted : free embeddings s, t fitted to the graph's links for --fit-steps Adam steps of the decoder's loss (E links + E sampled
           non-links): true links score high and nearly every candidate leaves at the row's smallest threshold
  random : 0.3 randn: the worst case, about half of all candidates pass the row's smallest threshold and take the search
rank   : mgv_pair_rank_counts on lists built beforehand       whole : ops.link_ranks (scores, lists, walk, filter)
count  : mgv_pair_select_count(sigmoid = 0, threshold = 0)    the floor
torch  : per 1,024 target rows a dense chunk of scores, compared with the gathered link scores and summed
         (for the batch: measured on its first graph and multiplied by the number of graphs)
One process; warm-up first; HIP events around the device work, median of --reps.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bench_pair_select import PEAK_F32_MATRIX, timed  # noqa: E402


def fit(ei, n, H, steps, g, dev):
    """Free embeddings after `steps` Adam steps of -log sigma(<s_u, t_v>) over the links and -log(1 - sigma) over as many random pairs."""
    st = (0.3 * torch.randn(n, 2 * H, generator=g, device=dev)).requires_grad_(True)
    opt = torch.optim.Adam([st], lr=0.05)
    for _ in range(steps):
        neg = torch.randint(0, n, ei.shape, generator=g, device=dev)
        pos = (st[ei[0], :H] * st[ei[1], H:]).sum(1)
        non = (st[neg[0], :H] * st[neg[1], H:]).sum(1)
        loss = torch.nn.functional.softplus(-pos).mean() + torch.nn.functional.softplus(non).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return st.detach()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--graph-n', type=int, default=65536)
    ap.add_argument('--batch-graphs', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fit-steps', type=int, default=60)
    ap.add_argument('--skip-batch', action='store_true')
    a = ap.parse_args(argv)
    from deepgate import _hip, ops, synthetic
    ptr = _hip.ptr
    dev = torch.device('cuda:0')
    H = 64
    n = a.graph_n
    g = torch.Generator(device=dev).manual_seed(0)
    graph = synthetic.make_graph('aig', n, 63, 900, n_inputs=n // 64)        # n a multiple of 64: n / 64 inputs, 63 levels of n / 64 gates
    ei1 = torch.as_tensor(graph['edge_index']).long().to(dev)
    inputs = {'fitted': fit(ei1, n, H, a.fit_steps, g, dev), 'random': 0.3 * torch.randn(n, 2 * H, generator=g, device=dev)}

    def box(graphs, tag, reps):
        N = graphs * n
        ei = torch.cat([ei1 + k * n for k in range(graphs)], 1)
        gp = torch.arange(graphs + 1, dtype=torch.int32, device=dev) * n
        for kind, st1 in inputs.items():
            st = st1.repeat(graphs, 1)
            s, t = st[:, :H], st[:, H:]
            score = ops.pair_scores_at(s, t, ei, sigmoid=False)
            lists = ops.link_rank_lists(ei, score, N, graph_ptr=gp, by='dst')
            E = ei.shape[1]
            n_gt = torch.empty(E, dtype=torch.int32, device=dev)
            n_eq = torch.empty(E, dtype=torch.int32, device=dev)
            # by target: the rows are t, the candidates s
            common = (H, N, ptr(t), 2 * H, ptr(s), 2 * H, ptr(gp), graphs)
            rank_ms = timed(lambda: _hip.call('mgv_pair_rank_counts', *common, 0, ptr(lists.thr_ptr), ptr(lists.thr), ptr(n_gt), ptr(n_eq)),
                            reps)
            n_sel = torch.empty(N, dtype=torch.int32, device=dev)
            count_ms = timed(lambda: _hip.call('mgv_pair_select_count', *common, 0, 0.0, 0, ptr(n_sel)), reps)
            keep = [None]

            def whole():
                keep[0] = ops.link_ranks(s, t, ei, graph_ptr=gp, by='dst')
            whole_ms = timed(whole, reps)
            ranks = keep[0]
            sc, tc = s[:n].contiguous(), t[:n].contiguous()
            order = torch.sort(ei1[1], stable=True).indices
            dst, src = ei1[1][order], ei1[0][order]
            got = torch.empty(dst.numel(), dtype=torch.int64, device=dev)

            def torch_chunks():
                for b0 in range(0, n, 1024):
                    lo, hi = torch.searchsorted(dst, torch.tensor([b0, b0 + 1024], device=dev)).tolist()
                    chunk = torch.mm(tc[b0:b0 + 1024], sc.T)
                    rows = dst[lo:hi] - b0
                    thr = chunk[rows, src[lo:hi]]
                    got[lo:hi] = (chunk[rows] > thr[:, None]).sum(1)
            torch_ms = timed(torch_chunks, max(1, reps // 2), warm=1) * graphs
            unf = ops.link_ranks(s[:n], t[:n], ei1, by='dst', filtered=False)
            diff = int((unf.rank_lo[order] - 1 - got).abs().max())        # torch.mm adds in another order: a few places at most
            lo_f = ranks.rank_lo[ranks.valid].double()
            print(json.dumps({'case': '%s_%s' % (tag, kind), 'graphs': graphs, 'nodes_per_graph': n, 'N': N, 'H': H, 'links': E,
                              'longest_list': int((lists.thr_ptr[1:] - lists.thr_ptr[:-1]).max()),
                              'mrr_lo': float((1.0 / lo_f).mean()), 'mean_rank_lo': float(lo_f.mean()),
                              'rank_ms': rank_ms, 'count_ms': count_ms, 'whole_ms': whole_ms, 'torch_chunked_ms': torch_ms,
                              'rank_over_count': rank_ms / count_ms, 'torch_over_rank': torch_ms / rank_ms, 'torch_over_whole': torch_ms / whole_ms,
                              'mfma_floor_ms': 2.0 * graphs * float(n) ** 2 * H / PEAK_F32_MATRIX * 1e3,
                              'torch_vs_walk_largest_rank_difference': diff}), flush=True)

    box(1, 'one_graph', a.reps)
    if not a.skip_batch:
        box(a.batch_graphs, 'config2_batch', 1)


if __name__ == '__main__':
    main()
