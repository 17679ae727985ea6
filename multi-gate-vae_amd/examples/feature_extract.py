"""Embedding extraction with the MI355X path (the role of the reference's DG_VAE/examples/feature_extract*.py:9-34):
build the per-type Model, optionally load a checkpoint written by `Trainer.save` (or a reference `.pth`: same
state_dict keys), run `model(G) -> (hs, hf)` over a dataset and save the embeddings.

    python examples/feature_extract.py --type aig --data_dir DIR [--checkpoint exp/e/stage_3.pth] --out emb.npz
    python examples/feature_extract.py --type aig --synthetic 4 --out emb.npz
    python examples/feature_extract.py --type aig --synthetic 4 --link_metrics      # + ROC-AUC / AP of the decoder per batch
    python examples/feature_extract.py --type aig --synthetic 4 --predict_links 8   # + every gate's 8 most probable fan-out targets
    python examples/feature_extract.py --type aig --synthetic 4 --reconstruct 0.5   # + the decoded edge list of every graph
    python examples/feature_extract.py --type aig --synthetic 4 --similar 8         # + every gate's 8 functionally closest gates
    python examples/feature_extract.py --type aig --synthetic 4 --equivalences 0.999   # + the gate pairs with cos(hf) above 0.999
    python examples/feature_extract.py --type aig --synthetic 4 --match 8           # + every gate's 8 closest gates in the NEXT/PREVIOUS graph
    python examples/feature_extract.py --type aig --synthetic 4 --cross_equivalences 0.999   # + the gate pairs ACROSS graphs 2i, 2i + 1
    python examples/feature_extract.py --type aig --synthetic 4 --cross_equivalences_max 1000   # the same, at most 1000 pairs per batch
    python examples/feature_extract.py --type aig --synthetic 4 --cross_classes 0.999   # + the classes that may span graphs 2i, 2i + 1
    python examples/feature_extract.py --type aig --synthetic 4 --equivalences_max 1000   # --equivalences, at most 1000 pairs per batch
    python examples/feature_extract.py --type aig --synthetic 4 --similarity_profile 12   # + pairs per graph above 1 - 2^-j, j = 1..12
    python examples/feature_extract.py --type aig --synthetic 4 --recon_curve 9        # + the decoder's confusion at 0.1, 0.2 .. 0.9
    python examples/feature_extract.py --type aig --synthetic 4 --link_ranking 1,10    # + exact MRR / Hits@1 / Hits@10 of the true fan-ins
    python examples/feature_extract.py --type aig --synthetic 4 --function_acc 0.05,0.1   # + exact functional ordering accuracy per circuit
    python examples/feature_extract.py --type aig --synthetic 4 --decode_circuit dec.npz  # + a legal circuit decoded from every graph's hs
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepgate  # noqa: E402
from deepgate import synthetic  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--type', required=True, choices=['aig', 'mig', 'xmg', 'xag'])
    ap.add_argument('--data_dir', default='')
    ap.add_argument('--synthetic', type=int, default=0)
    ap.add_argument('--checkpoint', default='')
    ap.add_argument('--dim_hidden', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--out', default='embeddings.npz')
    ap.add_argument('--link_metrics', action='store_true', help='also print ROC-AUC / average precision of the decoder: every batch\'s '
                    'edges ranked against sampled non-edges (Model.link_metrics)')
    ap.add_argument('--predict_links', type=int, default=0, metavar='K', help='also store every node\'s K most probable successors inside '
                    'its graph (name/pred_dst, ids local to the graph, -1 past the end; name/pred_score) and print the mean precision and '
                    'recall of the decoder against the FULL adjacency (Model.predict_links / reconstruction_counts; 1 <= K <= 32)')
    ap.add_argument('--reconstruct', type=float, default=None, metavar='THR', help='also store the graph the decoder reconstructs: every '
                    'pair inside a graph scored above THR (name/rec_edge_index [2, E\'], ids local to the graph, listed per source in '
                    'ascending target order) with its precision and recall against the true edges (name/rec_precision, name/rec_recall; '
                    'Model.reconstruct_edges / reconstruction_counts)')
    ap.add_argument('--similar', type=int, default=0, metavar='K', help='also store every gate\'s K functionally closest gates inside its '
                    'graph by cosine of hf (name/sim_idx, ids local to the graph, -1 past the end; name/sim_cos; Model.similar_gates; '
                    '1 <= K <= 32).  Primary inputs have hf = 0 and cosine 0 with everything')
    ap.add_argument('--equivalences', type=float, default=None, metavar='THR', help='also store the unordered gate pairs of every graph '
                    'whose hf have a cosine above THR, the candidates for equivalence checking (name/eq_pairs [2, P], local ids, first < '
                    'second; name/eq_cos; Model.equivalence_candidates).  Equal rows score within (2H + 6) 2^-24 of 1, not exactly 1: '
                    'use 0.999 rather than 1.0; primary inputs (hf = 0) are never reported at a positive THR')
    ap.add_argument('--match', type=int, default=0, metavar='K', help='match gates ACROSS circuits: the consecutive graphs (2i, 2i + 1) of '
                    'every batch are each other\'s peer (a golden design and its revision; an odd last graph has none), and every gate '
                    'gets its K closest gates of the peer graph by cosine of hf (name/match_idx, ids local to the PEER graph, -1 past '
                    'the end; name/match_cos; Model.match_gates; 1 <= K <= 32).  Primary inputs have hf = 0 and match nothing')
    ap.add_argument('--cross_equivalences', type=float, default=None, metavar='THR', help='with the pairing of --match, also store for '
                    'every graph the pairs (its gate, a gate of its peer graph) whose hf have a cosine above THR, the candidate '
                    'equivalence points between two circuits (name/xeq_pairs [2, P]: row 0 local to the graph, row 1 local to its '
                    'peer, listed per gate in ascending order; name/xeq_cos; Model.cross_equivalence_candidates).  A pair appears in '
                    'both graphs\' lists; use 0.999 rather than 1.0')
    ap.add_argument('--cross_equivalences_max', type=int, default=None, metavar='P', help='choose the threshold of --cross_equivalences by '
                    'count: the lowest one (not below --cross_equivalences when that is given too, else 0) at which a batch lists at most '
                    'P cross pairs, a pair counted once from each side as the lists hold it (Model.cross_equivalence_threshold), then '
                    'store the pairs as --cross_equivalences does and the threshold used (name/xeq_threshold)')
    ap.add_argument('--cross_classes', type=float, default=None, metavar='THR', help='with the pairing of --match, also store the candidate '
                    'classes that may span a graph and its peer: the connected components of "cos(hf) above THR" over the pairs inside '
                    'each graph and across each couple, straight from the tile walks without a pair list '
                    '(Model.cross_equivalence_classes(route=\'walk\')): name/xcl_label [n], the smallest id of a gate\'s class, local to '
                    'the couple (2i, 2i + 1) laid end to end — a label below the size of graph 2i is a gate of graph 2i — and the '
                    'number of classes that hold gates of both graphs is printed')
    ap.add_argument('--classes', type=float, default=None, metavar='THR', help='also store every graph\'s equivalence candidate classes, '
                    'what a SAT sweeper consumes: the connected components of "cos(hf) above THR" (name/eq_label [n], the smallest local '
                    'id of a gate\'s class; name/eq_class_ptr [C + 1] and name/eq_members [M], the classes with at least two gates, '
                    'members ascending, local ids; Model.equivalence_classes).  Single linkage: two gates of one class can have a '
                    'cosine below THR.  Primary inputs (hf = 0) are always singletons; use 0.999 rather than 1.0')
    ap.add_argument('--equivalences_max', type=int, default=None, metavar='P', help='choose the threshold of --equivalences by count: the '
                    'lowest one (not below --equivalences when that is given too, else 0) at which a batch lists at most P pairs '
                    '(Model.equivalence_threshold), then store the pairs as --equivalences does and the threshold used '
                    '(name/eq_threshold).  Equal gates share one cosine, which a threshold takes or leaves as a whole: fewer than P pairs '
                    'can come back')
    ap.add_argument('--similarity_profile', type=int, default=0, metavar='B', help='also store, per graph, the number of gate pairs whose '
                    'hf have a cosine above 1 - 2^-j, j = 1 .. B (B capped at 20): name/sim_thresholds [B] and name/sim_counts_above [B] '
                    '(Model.similarity_profile, one walk for all B).  Primary inputs (hf = 0) score 0; equal rows score within '
                    '(2H + 6) 2^-24 of 1')
    ap.add_argument('--recon_curve', type=int, default=0, metavar='B', help='also store the decoder\'s confusion against the FULL '
                    'adjacency at B evenly spaced thresholds in (0, 1), i / (B + 1): name/recon_thresholds [B] and name/recon_curve '
                    '[B, 4] = true positives, predicted positives, edges, ordered pairs (Model.reconstruction_curve, one walk; '
                    '1 <= B <= 256)')
    ap.add_argument('--link_ranking', default='', metavar='K1,K2,...', help='also print, per circuit, where its true links stand among ALL '
                    'candidates by target — every true fan-in of a gate ranked against all gates of the circuit, the gate\'s other fan-ins '
                    'left out: links ranked, MRR, Hits@K for every K (for the best and the worst place a tie allows) and the mean rank '
                    '(Model.link_ranking; exact, no sampled negatives)')
    ap.add_argument('--function_acc', nargs='?', const='0.05', default='', metavar='GAP,...', help='also store, per circuit, the share of '
                    'ALL comparisons of two listed truth-table pairs whose distances differ by at least GAP (up to 8 gaps, default 0.05) '
                    'that 1 - cos(hf) orders the way the truth-table distance does: name/func_acc [B] (-1 where no comparison is '
                    'eligible) and name/func_counts [B, 3] = eligible, concordant, tied (Model.function_accuracy; exact counts of what '
                    'get_function_acc samples)')
    ap.add_argument('--decode_circuit', default='', metavar='OUT.npz', help='also decode every graph\'s embeddings into a legal circuit of the '
                    'gate library — every gate its arity\'s best fan-ins among the gates of lower level, acyclic whatever the scores are '
                    '(Model.decode_circuit) — and write it to OUT.npz: name/edge_index [2, E\'] (sources on row 0, ids local to the graph, by '
                    'target, then by rank), name/fanin [n, K] (-1 past the end), name/score [n, K], name/short [n] (fewer candidates than '
                    'the arity) and, where the graph has edges, name/recovery [5] = gates, exact, hits, true_total, decoded_total '
                    '(Model.circuit_recovery); the mean exact-recovery rate is printed')
    ap.add_argument('--variational', action='store_true', help='the checkpoint is of a model trained with train.py --variational: build '
                    'the four heads fc_{s,t}_{mu,logstd} so that it loads in full; the link tools then decode the posterior means')
    a = ap.parse_args(argv)
    acc_gaps = [float(g) for g in a.function_acc.split(',') if g.strip()]
    rank_ks = [int(k) for k in a.link_ranking.split(',') if k.strip()]
    sim_thr = [1.0 - 2.0 ** -j for j in range(1, min(a.similarity_profile, 20) + 1)]
    rc_thr = [float(np.float32(i / (a.recon_curve + 1.0))) for i in range(1, a.recon_curve + 1)]
    dev = torch.device('cuda:0')
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=a.dim_hidden, s_rounds=a.rounds, t_rounds=a.rounds,
                                                     enable_reverse=True, layernorm=True)
    model = getattr(deepgate, 'dg_ae_model_' + a.type).Model(struct_encoder=enc, dim_hidden=a.dim_hidden, variational=a.variational).to(dev)
    if a.checkpoint:
        model.load(a.checkpoint)
    model.eval()
    if a.synthetic > 0:
        graphs = [synthetic.make_graph(a.type, 1024, 30, 900 + i, n_inputs=64) for i in range(a.synthetic)]
    else:
        train, val = deepgate.NpzParser(a.data_dir, os.path.join(a.data_dir, 'graphs.npz'), os.path.join(a.data_dir, 'labels.npz'),
                                        a.type, random_shuffle=False, trainval_split=1.0).get_dataset()
        graphs = train + val
    out, t0, records, counts = {}, time.time(), [], []
    dec_out, dec_rates = {}, []
    with torch.no_grad():
        for b0 in range(0, len(graphs), a.batch_size):
            chunk = graphs[b0:b0 + a.batch_size]
            batch = deepgate.CircuitBatch.from_arrays(synthetic.collate(chunk), device=dev)
            hs, hf = model(batch)
            if a.link_metrics:
                records.append(model.link_metrics(hs, batch.edge_index, plan=getattr(batch, '_mgv_plan', None)))
            ptr = batch.graph_ptr.tolist()
            if a.predict_links:
                idx, score, _ = model.predict_links(hs, a.predict_links, graph_ptr=batch.graph_ptr)
                counts.append(model.reconstruction_counts(hs, batch.edge_index, batch.graph_ptr))
                idx, score = idx.cpu().numpy(), score.cpu().numpy()
            if a.reconstruct is not None:
                rec_ei, rec_ptr, _ = model.reconstruct_edges(hs, graph_ptr=batch.graph_ptr, threshold=a.reconstruct)
                rc = model.reconstruction_counts(hs, batch.edge_index, batch.graph_ptr, threshold=a.reconstruct).double().cpu()
                rec_ei, eptr = rec_ei.cpu().numpy(), rec_ptr[batch.graph_ptr.to(rec_ptr.device).long()].tolist()      # the graphs' places in the list
            if a.similar:
                sim_idx, sim_cos, _ = model.similar_gates(hf, a.similar, graph_ptr=batch.graph_ptr)
                sim_idx, sim_cos = sim_idx.cpu().numpy(), sim_cos.cpu().numpy()
            xeq_thr = a.cross_equivalences
            if a.match or xeq_thr is not None or a.cross_equivalences_max is not None or a.cross_classes is not None:
                G = len(chunk)
                peer = [g ^ 1 if (g ^ 1) < G else -1 for g in range(G)]          # (2i, 2i + 1); an odd last graph has no peer
                pbase = [ptr[q] if q >= 0 else 0 for q in peer]
            if a.match:
                m_idx, m_cos, _ = model.match_gates(hf, a.match, batch.graph_ptr, peer)
                m_idx, m_cos = m_idx.cpu().numpy(), m_cos.cpu().numpy()
            if a.cross_equivalences_max is not None:
                xeq_thr = model.cross_equivalence_threshold(hf, a.cross_equivalences_max, batch.graph_ptr, peer,
                                                            lo=0.0 if xeq_thr is None else xeq_thr)['threshold']
            if xeq_thr is not None:
                xeq, xeq_ptr, xeq_cos = model.cross_equivalence_candidates(hf, batch.graph_ptr, peer, threshold=xeq_thr, with_scores=True)
                xeq, xeq_cos = xeq.cpu().numpy(), xeq_cos.cpu().numpy()
                xptr = xeq_ptr[batch.graph_ptr.to(xeq_ptr.device).long()].tolist()             # the graphs' places in the list
            if a.cross_classes is not None:
                xcl_label, xcl_ptr, xcl_mem = (x.cpu().numpy() for x in model.cross_equivalence_classes(
                    hf, batch.graph_ptr, peer, threshold=a.cross_classes, route='walk'))
                # members ascend inside a class: its first and last member lie in its lowest and highest graph
                g_lo = np.searchsorted(ptr[1:], xcl_mem[xcl_ptr[:-1]], side='right')
                g_hi = np.searchsorted(ptr[1:], xcl_mem[xcl_ptr[1:] - 1], side='right')
                xcl_span = np.bincount(g_lo[g_lo != g_hi], minlength=G)                        # counted at the lower graph of a couple
            eq_thr = a.equivalences
            if a.equivalences_max is not None:
                eq_thr = model.equivalence_threshold(hf, a.equivalences_max, graph_ptr=batch.graph_ptr,
                                                     lo=0.0 if a.equivalences is None else a.equivalences)['threshold']
            if sim_thr:
                sim_above = model.similarity_profile(hf, sim_thr, graph_ptr=batch.graph_ptr).cpu().numpy()
            if rc_thr:
                curve = model.reconstruction_curve(hs, batch.edge_index, batch.graph_ptr, rc_thr).cpu().numpy()
            if rank_ks:
                rm = [x.cpu() for x in model.link_ranking(hs, batch.edge_index, batch.graph_ptr, ks=rank_ks, by='dst',
                                                          plan=getattr(batch, '_mgv_plan', None))[0]]
            if acc_gaps:
                f_acc, f_cnt = (x.cpu().numpy() for x in model.function_accuracy(hf, batch['tt_pair_index'], batch['tt_sim'],
                                                                                  graph_ptr=batch.graph_ptr, min_gap=acc_gaps))
            if eq_thr is not None:
                eq, eq_ptr, eq_cos = model.equivalence_candidates(hf, graph_ptr=batch.graph_ptr, threshold=eq_thr, with_scores=True)
                eq, eq_cos = eq.cpu().numpy(), eq_cos.cpu().numpy()
                qptr = eq_ptr[batch.graph_ptr.to(eq_ptr.device).long()].tolist()               # the graphs' places in the list
            if a.classes is not None:
                cl_label, cl_ptr, cl_mem = (x.cpu().numpy() for x in model.equivalence_classes(hf, graph_ptr=batch.graph_ptr,
                                                                                               threshold=a.classes))
                cptr = np.searchsorted(cl_mem[cl_ptr[:-1]], ptr).tolist()      # classes come by label and never cross graphs
            if a.decode_circuit:
                recov, dec = model.circuit_recovery(hs, batch)
                d_ei, d_fanin, d_score, d_short = (x.cpu().numpy() for x in dec)
                d_rec = recov.counts.cpu().numpy()
                eptr_d = np.searchsorted(d_ei[1], ptr).tolist()                                # listed by target: the graphs' places
            for k, g in enumerate(chunk):
                name = g.get('name') or 'graph%d' % (b0 + k)
                if a.decode_circuit:
                    loc = d_fanin[ptr[k]:ptr[k + 1]]
                    dec_out[name + '/edge_index'] = (d_ei[:, eptr_d[k]:eptr_d[k + 1]] - ptr[k]).astype(np.int32)
                    dec_out[name + '/fanin'] = np.where(loc >= 0, loc - ptr[k], -1).astype(np.int32)
                    dec_out[name + '/score'] = d_score[ptr[k]:ptr[k + 1]]
                    dec_out[name + '/short'] = d_short[ptr[k]:ptr[k + 1]]
                    if d_rec[k, 0] > 0:
                        dec_out[name + '/recovery'] = d_rec[k]
                        dec_rates.append(d_rec[k, 1] / d_rec[k, 0])
                if rank_ks:
                    n = max(int(rm[0][k]), 1)
                    hits = ' '.join('Hits@%d %.4f..%.4f' % (K, int(rm[2][k, j]) / n, int(rm[1][k, j]) / n) for j, K in enumerate(rank_ks))
                    print('[INFO] %s: link ranking by target: %d links ranked, MRR %.6f, %s, mean rank %.2f..%.2f'
                          % (name, int(rm[0][k]), float(rm[5][k]), hits, int(rm[3][k]) / n, int(rm[4][k]) / n))
                if acc_gaps:
                    out[name + '/func_acc'] = f_acc[k]
                    out[name + '/func_counts'] = f_cnt[k]
                    print('[INFO] %s: functional ordering accuracy %s' % (name, ', '.join(
                        '%.4f at gap %g (%d of %d comparisons, %d tied)' % (f_acc[k, j], gap, f_cnt[k, j, 1], f_cnt[k, j, 0], f_cnt[k, j, 2])
                        for j, gap in enumerate(acc_gaps))))
                if a.classes is not None:
                    cp = cl_ptr[cptr[k]:cptr[k + 1] + 1]
                    out[name + '/eq_label'] = (cl_label[ptr[k]:ptr[k + 1]] - ptr[k]).astype(np.int32)
                    out[name + '/eq_class_ptr'] = (cp - cp[0]).astype(np.int64)
                    out[name + '/eq_members'] = (cl_mem[cp[0]:cp[-1]] - ptr[k]).astype(np.int32)
                    print('[INFO] %s: %d classes of %d gates with cos(hf) > %g' % (name, cptr[k + 1] - cptr[k], cp[-1] - cp[0], a.classes))
                if a.similar:
                    loc = sim_idx[ptr[k]:ptr[k + 1]]
                    out[name + '/sim_idx'] = np.where(loc >= 0, loc - ptr[k], -1).astype(np.int32)
                    out[name + '/sim_cos'] = sim_cos[ptr[k]:ptr[k + 1]]
                if a.match:
                    loc = m_idx[ptr[k]:ptr[k + 1]]
                    out[name + '/match_idx'] = np.where(loc >= 0, loc - pbase[k], -1).astype(np.int32)
                    out[name + '/match_cos'] = m_cos[ptr[k]:ptr[k + 1]]
                if xeq_thr is not None:
                    pr = xeq[:, xptr[k]:xptr[k + 1]]
                    out[name + '/xeq_pairs'] = np.stack([pr[0] - ptr[k], pr[1] - pbase[k]]).astype(np.int32)
                    out[name + '/xeq_cos'] = xeq_cos[xptr[k]:xptr[k + 1]]
                    print('[INFO] %s: %d gate pairs with %s at cos(hf) > %s' % (name, xptr[k + 1] - xptr[k], 'graph %d' % (b0 + peer[k])
                                                                              if peer[k] >= 0 else 'no peer',
                                                                              ('%g' if a.cross_equivalences_max is None else '%.9g') % xeq_thr))
                if a.cross_equivalences_max is not None:
                    out[name + '/xeq_threshold'] = np.float32(xeq_thr)
                if a.cross_classes is not None:
                    out[name + '/xcl_label'] = (xcl_label[ptr[k]:ptr[k + 1]] - ptr[k & ~1]).astype(np.int32)
                    if peer[k] > k:
                        print('[INFO] %s: %d classes hold gates of it and of graph %d at cos(hf) > %g'
                              % (name, int(xcl_span[k]), b0 + peer[k], a.cross_classes))
                if eq_thr is not None:
                    out[name + '/eq_pairs'] = (eq[:, qptr[k]:qptr[k + 1]] - ptr[k]).astype(np.int32)
                    out[name + '/eq_cos'] = eq_cos[qptr[k]:qptr[k + 1]]
                    print('[INFO] %s: %d gate pairs with cos(hf) > %s' % (name, qptr[k + 1] - qptr[k],
                                                                         ('%g' if a.equivalences_max is None else '%.9g') % eq_thr))
                if a.equivalences_max is not None:
                    out[name + '/eq_threshold'] = np.float32(eq_thr)
                if sim_thr:
                    out[name + '/sim_thresholds'] = np.asarray(sim_thr, dtype=np.float32)
                    out[name + '/sim_counts_above'] = sim_above[k]
                if rc_thr:
                    out[name + '/recon_thresholds'] = np.asarray(rc_thr, dtype=np.float32)
                    out[name + '/recon_curve'] = curve[k]
                if a.reconstruct is not None:
                    out[name + '/rec_edge_index'] = (rec_ei[:, eptr[k]:eptr[k + 1]] - ptr[k]).astype(np.int32)
                    out[name + '/rec_precision'] = np.float64(rc[k, 0] / max(float(rc[k, 1]), 1.0))
                    out[name + '/rec_recall'] = np.float64(rc[k, 0] / max(float(rc[k, 2]), 1.0))
                if a.predict_links:
                    loc = idx[ptr[k]:ptr[k + 1]]
                    out[name + '/pred_dst'] = np.where(loc >= 0, loc - ptr[k], -1).astype(np.int32)
                    out[name + '/pred_score'] = score[ptr[k]:ptr[k + 1]]
                out[name + '/hs'] = hs[ptr[k]:ptr[k + 1]].cpu().numpy()
                out[name + '/hf'] = hf[ptr[k]:ptr[k + 1]].cpu().numpy()
    torch.cuda.synchronize()
    np.savez(a.out, **out)
    print('[INFO] %d graphs embedded in %.2f s -> %s' % (len(graphs), time.time() - t0, a.out))
    if a.decode_circuit:
        np.savez(a.decode_circuit, **dec_out)
        print('[INFO] decoded circuits of %d graphs -> %s; exact gate recovery over the %d graphs with edges: %s'
              % (len(graphs), a.decode_circuit, len(dec_rates), '%.4f' % (sum(dec_rates) / len(dec_rates)) if dec_rates else 'n/a'))
    if a.link_metrics:
        pairs = deepgate.metrics.read_link_records(records)      # one host read for all batches
        print('[INFO] link prediction over %d batches: AUC %.4f, AP %.4f' % (len(pairs), sum(x for x, _ in pairs) / len(pairs),
                                                                             sum(y for _, y in pairs) / len(pairs)))
    if a.predict_links:
        c = torch.cat(counts).double().cpu()                     # [graphs, 4]: TP, predicted positives, edges, ordered pairs
        prec, rec = c[:, 0] / c[:, 1].clamp(min=1), c[:, 0] / c[:, 2].clamp(min=1)
        print('[INFO] full-adjacency reconstruction over %d graphs (all n^2 ordered pairs, threshold 0.5): precision %.4f, recall %.4f'
              % (c.shape[0], float(prec.mean()), float(rec.mean())))


if __name__ == '__main__':
    main()
