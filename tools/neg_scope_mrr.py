#!/usr/bin/env python3
"""An observation, not a test: Model.link_ranking's MRR (by target, filtered, over all candidates of a link's own circuit) after two
short synthetic trainings from the same seeds, one with the reference's batch-wide negatives and one with --neg_scope graph
--neg_reverse FRAC.

    python tools/neg_scope_mrr.py [--graphs 8 --nodes 1024 --levels 16 --steps 60 --reverse 0.25]

Trains on one batch of --graphs synthetic AIGs for --steps steps per setting and ranks the links of a second, held-out batch.  Prints
one JSON line per setting: mean MRR and Hits@1 / Hits@10 over the held-out circuits, and the sampled AUC of link_metrics under the
batch-wide draw and under the local one."""
import argparse
import itertools
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'multi-gate-vae_amd'), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=8)
    ap.add_argument('--nodes', type=int, default=1024)
    ap.add_argument('--levels', type=int, default=16)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--reverse', type=float, default=0.25)
    a = ap.parse_args()
    import deepgate
    from deepgate import sampling, synthetic as syn
    dev = torch.device('cuda:0')

    def batch_of(first):
        graphs = [syn.make_graph('aig', a.nodes, a.levels, first + i, n_inputs=a.nodes // 16) for i in range(a.graphs)]
        for g in graphs:
            g.pop('neg_edge_index', None)
        return deepgate.CircuitBatch.from_arrays(syn.collate(graphs), device=dev)

    train, held = batch_of(31000), batch_of(32000)
    for scope, rev in (('batch', 0.0), ('graph', 0.0), ('graph', a.reverse)):
        torch.manual_seed(5)
        sampling._CALLS = itertools.count()
        enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=64, s_rounds=2, t_rounds=2, layernorm=True)
        model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=64).to(dev).train()
        args = types.SimpleNamespace(model='DG_AE', neg_scope=scope, neg_reverse=rev)
        tr = deepgate.Trainer(args, model, training_id='mrr', save_dir=tempfile.mkdtemp(), lr=1e-3, rc_prob_func_weight=[1.0, 4.0, 4.0],
                              device='cuda:0', batch_size=a.graphs, distributed=False)
        for _ in range(a.steps):
            ls = tr.train_step(train)
        model.eval()
        with torch.no_grad():
            hs, _ = model(held)
            m, _ = model.link_ranking(hs, held.edge_index, held.graph_ptr, ks=(1, 10), by='dst', plan=held._mgv_plan)
            model.set_negative_sampling('batch', 0.0)
            auc_batch = model.link_metrics(hs, held.edge_index, plan=held._mgv_plan)[0].item()
            model.set_negative_sampling('graph', 0.0)
            auc_graph = model.link_metrics(hs, held.edge_index, plan=held._mgv_plan, graph_ptr=held.graph_ptr)[0].item()
        ranked = m.ranked.double()
        print(json.dumps({'scope': scope, 'reverse': rev, 'steps': a.steps, 'recon_loss': float(ls['recon_loss']),
                          'mrr': float(m.mrr.mean()), 'hits1': float((m.hits_lo[:, 0] / ranked).mean()),
                          'hits10': float((m.hits_lo[:, 1] / ranked).mean()), 'sampled_auc_batch_negatives': auc_batch,
                          'sampled_auc_graph_negatives': auc_graph}))


if __name__ == '__main__':
    main()
