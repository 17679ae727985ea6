"""DirectedGAE (reference: DG_VAE/deepgate/digae_model.py:106-168): an encoder that returns (s, t), the directed inner-product
decoder, the reconstruction loss and the link-prediction test on the HIP kernels.  The undirected GAE of the same file is not
part of the DG_AE / AE training paths and is left out."""
import torch

from . import metrics, ops, pairs, similarity
from ._model_base import DecodedCircuit
from .digae_layer import DirectedInnerProductDecoder
from .sampling import negative_sampling


class DirectedGAE(torch.nn.Module):
    def __init__(self, encoder, decoder=None):
        super().__init__()
        self.encoder = encoder
        self.decoder = DirectedInnerProductDecoder() if decoder is None else decoder

    def forward(self, data):
        """sigmoid(s t^T) over all node pairs (digae_model.py:118-122), at any size the device can hold (ops.pair_scores)."""
        s, t = self.encoder(data.x, data.x, data.edge_index)
        return self.decoder.forward_all(s, t)

    def predict_links(self, s, t, k, graph_ptr=None, skip_self=True):
        """(idx [N, k] int32, score [N, k], n_above [N] int32): every node's k most probable successors inside its own graph and the
        number of candidates the decoder calls an edge (score > 0.5), streamed (ops.pair_topk).  Added functionality."""
        with torch.no_grad():
            return pairs.pair_topk(s, t, k, graph_ptr=graph_ptr, sigmoid=True, threshold=0.5, skip_self=skip_self)

    def reconstruction_counts(self, s, t, edge_index, graph_ptr, threshold=0.5):
        """int64 [G, 4] per graph: true positives, predicted positives over all n_g^2 ordered pairs, edges, ordered pairs
        (ops.reconstruction_counts); precision and recall against the full adjacency are the caller's two divisions."""
        with torch.no_grad():
            return pairs.reconstruction_counts(s, t, edge_index, graph_ptr, threshold)

    def reconstruction_curve(self, s, t, edge_index, graph_ptr, thresholds):
        """int64 [G, B, 4]: reconstruction_counts at every one of `thresholds` (strictly ascending, at most 256) from one all-pairs
        walk (ops.reconstruction_curve).  Added functionality."""
        with torch.no_grad():
            return pairs.reconstruction_curve(s, t, edge_index, graph_ptr, thresholds)

    def link_ranking(self, s, t, edge_index, graph_ptr, ks=(1, 3, 10, 50), by='dst', filtered=True, plan=None):
        """(RankMetrics, LinkRanks): exact MRR, Hits@K and rank sums per graph over the FULL candidate set, and the per-link ranks
        behind them (ops.rank_metrics of ops.link_ranks) — by='dst': every true link among all nodes of its graph that could feed its
        target; `test` ranks against sampled non-edges only.  Added functionality."""
        with torch.no_grad():
            ranks = metrics.link_ranks(s, t, edge_index, graph_ptr=graph_ptr, by=by, filtered=filtered, plan=plan)
            return metrics.rank_metrics(ranks, edge_index, graph_ptr, ks=ks, by=by), ranks

    def reconstruct_edges(self, s, t, graph_ptr=None, threshold=0.5, skip_self=False, by='src', with_scores=False, max_edges=None):
        """(edge_index int64 [2, E'], row_ptr int64 [N + 1], score [E'] or None): every pair inside a graph that the decoder calls an
        edge (score > threshold) as (source, target) rows, listed per source or (by='dst') per target (ops.reconstruct_edges).  Added
        functionality."""
        with torch.no_grad():
            return pairs.reconstruct_edges(s, t, graph_ptr=graph_ptr, threshold=threshold, skip_self=skip_self, by=by,
                                           with_scores=with_scores, max_edges=max_edges)

    def decode_circuit(self, s, t, key, want, graph_ptr=None, K=None):
        """DecodedCircuit(edge_index int64 [2, E'], fanin int32 [N, K], score [N, K], short bool [N]): every node's `want` best fan-ins
        among the nodes of its own graph with a smaller order `key` (a level), so the result has the asked in-degrees and is acyclic
        whatever the scores are (ops.fanin_decode).  short: fewer candidates than wanted.  Added functionality."""
        with torch.no_grad():
            want = torch.as_tensor(want).to(s.device).flatten()
            idx, score, n_cand = pairs.fanin_decode(s, t, key, want, graph_ptr=graph_ptr, K=K)
            return DecodedCircuit(pairs.fanin_edges(idx), idx, score, n_cand < want.to(torch.int32))

    def circuit_recovery(self, s, t, edge_index, key, want='degree', graph_ptr=None, K=None):
        """(FaninRecovery, DecodedCircuit): decode_circuit counted against edge_index per graph — {gates, exact, hits, true_total,
        decoded_total} and exact / gates (ops.fanin_recovery); want='degree': the true in-degree.  Added functionality."""
        with torch.no_grad():
            if isinstance(want, str):
                if want != 'degree':
                    raise ValueError("want must be 'degree' (true in-degree) or a tensor, got %r" % (want,))
                want = torch.bincount(edge_index[1].to(s.device), minlength=s.shape[0])
            dec = self.decode_circuit(s, t, key, want, graph_ptr=graph_ptr, K=K)
            return metrics.fanin_recovery(dec.fanin, edge_index, graph_ptr=graph_ptr), dec

    def reconstructed_components(self, edge_index, N):
        """label int32 [N]: the weakly connected components of a decoded link list (reconstruct_edges' edge_index, direction ignored) —
        label[i] is the smallest id of i's component (ops.components, a union-find on the device).  Added functionality."""
        return similarity.components(edge_index, N)

    def encode(self, *args, **kwargs):
        return self.encoder(*args, **kwargs)

    def decode(self, *args, **kwargs):
        return self.decoder(*args, **kwargs)

    def recon_loss(self, s, t, pos_edge_index, neg_edge_index=None):
        """(pos_loss + neg_loss, pred_bin, gt_bin) of digae_model.py:133-154 in one fused loss kernel (ops.ReconLossFn)."""
        if neg_edge_index is None:
            neg_edge_index = negative_sampling(pos_edge_index, s.shape[0])
        st = torch.cat([s, t], dim=1)
        loss, _, pred_bin = ops.ReconLossFn.apply(st, pos_edge_index, neg_edge_index, True)
        Ep, En = pos_edge_index.shape[1], neg_edge_index.shape[1]
        gt_bin = torch.zeros(Ep + En, dtype=torch.int32, device=s.device)
        gt_bin[:Ep] = 1
        return loss, pred_bin, gt_bin

    def test(self, s, t, pos_edge_index, neg_edge_index):
        """(ROC-AUC, average precision) of the decoder's scores (digae_model.py:156-168), ranked on the device (ops.link_record)."""
        return metrics.read_link_records([metrics.link_record(s, t, pos_edge_index, neg_edge_index)])[0]
