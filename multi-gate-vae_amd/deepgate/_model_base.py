"""Shared implementation of the four reference `Model` classes
(DG_VAE/deepgate/dg_ae_model_{aig,mig,xag,xmg}.py): structural encoding -> hs_linear -> levelised
per-gate-type attention + GRU sweep -> (hs, hf); readout, reconstruction loss, checkpoint loading.
Sub-module names and construction order follow the reference so state_dicts and seeded
initialisation line up."""
import os
from collections import namedtuple

import torch
from torch import nn

from . import metrics, ops, pairs, similarity
from .arch.mlp import MLP
from .arch.tfmlp import TFMlpAggr
from .data import plan_of
from .digae_layer import DirectedInnerProductDecoder
from .sampling import NegativeEdges, negative_sampling, negative_sampling_device

EPS = 1e-15
DEVICE_SAMPLER = True             # fused device sampler whenever the batch has a plan (the torch rejection sampler serves callers without one)
MAX_LOGSTD = 10


DecodedCircuit = namedtuple('DecodedCircuit', 'edge_index fanin score short')


class FunctionalModel(nn.Module):
    ENCODER_ATTR = 'struct_encoder'
    GATES = ()            # ((name, gate id), ...) in the order the reference creates aggr_*/update_* modules
    ARITY = {'and': 2, 'or': 2, 'xor': 2, 'not': 1, 'maj': 3}           # fan-ins per gate of the libraries (decode_circuit)

    VAR_HEADS = ('fc_s_mu', 'fc_s_logstd', 'fc_t_mu', 'fc_t_logstd')      # DirectedGVAE's names (digvae_model.py:112-115)

    def __init__(self, struct_encoder, num_rounds=1, dim_hidden=128, enable_encode=True, enable_reverse=True, variational=False):
        super().__init__()
        setattr(self, self.ENCODER_ATTR, struct_encoder)
        self.decoder = DirectedInnerProductDecoder()
        self.hs_linear = nn.Linear(dim_hidden * 2, dim_hidden)
        self.hs_decompose = nn.Linear(dim_hidden, dim_hidden * 2)
        self.num_rounds = num_rounds
        self.enable_encode = enable_encode
        self.enable_reverse = enable_reverse
        self.dim_hidden = dim_hidden
        self.dim_mlp = 32
        for name, _ in self.GATES:
            setattr(self, 'aggr_%s_func' % name, TFMlpAggr(dim_hidden * 2, dim_hidden))
        for name, _ in self.GATES:
            setattr(self, 'update_%s_func' % name, nn.GRU(dim_hidden, dim_hidden))
        self.readout_prob = MLP(dim_hidden, self.dim_mlp, 1, num_layer=3, p_drop=0.2, norm_layer='batchnorm',
                                act_layer='relu')
        # variational link heads on st = hs_decompose(hs) (added functionality: the reference's DG_VAE path never ran, SURVEY.md
        # §3.4).  Registered AFTER the reference's modules, so their seeded values and state_dict keys do not move.
        self.variational = bool(variational)
        if self.variational:
            for name in self.VAR_HEADS:
                setattr(self, name, nn.Linear(dim_hidden, dim_hidden))
        self._klsum, self._kl_n = None, 0                      # the last recon_loss's two KL sums (device) and its node count
        self.last_confusion = None
        self.last_link_metrics = None
        self._neg_scope, self._neg_reverse = 'batch', 0.0      # set_negative_sampling

    # ---- forward ---------------------------------------------------------------------------------
    def _sweep_params(self):
        parts = [getattr(self, 'aggr_%s_func' % n).composed(getattr(self, 'update_%s_func' % n)) for n, _ in self.GATES]
        return [torch.stack([p[i] for p in parts]) for i in range(5)]

    def forward(self, G, branch=None):
        """`branch` (step_branch.StepBranch, optional): recon_loss runs on the branch's stream once hs exists and BEFORE the level
        sweep's nodes are created; the sweep consumes hs as it comes back through the hs_decompose node."""
        if self.num_rounds < 1:
            raise ValueError('num_rounds must be >= 1')
        plan = plan_of(G, [gid for _, gid in self.GATES])
        dev = self.hs_linear.weight.device
        rows = torch.eye(6, dtype=torch.float32, device=dev)          # one_hot(x[:,1], 6) rows
        enc = getattr(self, self.ENCODER_ATTR)
        s, t = enc(None, None, G.edge_index, plan=plan, classes=(rows, plan.xcls))
        st = None
        if branch is not None and ops.linear_pair_ok(s, t, self.hs_linear.weight, self.hs_decompose.weight):
            # hs and st = hs_decompose(hs) in one pass in front of the fork (ops.LinearPairFn): the branch starts at the sampler
            # (of a variational model, at its link heads)
            hs, st = ops.linear_pair(s, t, self.hs_linear.weight, self.hs_linear.bias, self.hs_decompose.weight, self.hs_decompose.bias)
        else:
            hs = ops.linear(s, self.hs_linear.weight, self.hs_linear.bias, x2=t)
        hs_in = hs
        if branch is not None:
            with branch.fork(hs if st is None else st):
                hs_in = branch.took(*self.recon_loss(hs, plan=plan, return_hs=True, st=st, **branch.recon_args))
        hf = ops.FuncSweepFn.apply(plan, hs_in, *self._sweep_params())
        if branch is not None:
            hf = branch.sweep_out(hf)
        # further rounds (dg_ae_model_aig.py:70; the reference default and train.py use 1): every gate is updated again, its GRU
        # starting from the gate's previous state, on the same level kernels (b_hh is inside gh)
        for _ in range(self.num_rounds - 1):
            au, Wvc, bvc, bih, _ = self._sweep_params()
            hf = ops.FuncSweepFn.apply(plan, hs_in, au, Wvc, bvc, bih, None, hf, self._round_gh(plan, hf))
        return hs, hf

    def _round_gh(self, plan, hf):
        """gh[N, 3H] = W_hh h_prev + b_hh with each updated node's OWN aggregator weights (nn.GRU gate order r, z, n): at H = 64 in bf16x3
        mode one grouped Linear launch over the sweep's tiles; otherwise on the plain linear kernels: the rows of every gate type are
        gathered, multiplied per gate block and put back (index moves only)."""
        H = self.dim_hidden
        if hf.is_cuda and H == 64 and ops.use_x3(H) and ops.GROUPED_ROUND:
            # one grouped Linear over the sweep's (level, slot) tiles, each tile with its slot's weights (ops.RoundGhFn)
            grus = [getattr(self, 'update_%s_func' % name) for name, _ in self.GATES]
            return ops.RoundGhFn.apply(plan, hf, torch.stack([g.weight_hh_l0 for g in grus]), torch.stack([g.bias_hh_l0 for g in grus]))
        gh = torch.zeros(hf.shape[0], 3 * H, dtype=hf.dtype, device=hf.device)
        for (name, _), idx in zip(self.GATES, plan.slot_nodes()):
            if idx.numel() == 0:
                continue
            gru = getattr(self, 'update_%s_func' % name)
            rows = hf.index_select(0, idx)
            parts = [ops.linear(rows, gru.weight_hh_l0[g * H:(g + 1) * H], gru.bias_hh_l0[g * H:(g + 1) * H]) for g in range(3)]
            gh = gh.index_copy(0, idx, torch.cat(parts, dim=1))
        return gh

    def pred_prob(self, hf, seed=None):
        return self.readout_prob(hf, clamp01=True, seed=seed)

    def set_negative_sampling(self, scope='batch', reverse=0.0):
        """Which negatives recon_loss and link_metrics draw.  scope='batch' (the default, the reference's draw, dg_ae_model_aig.py:115-119):
        both ends uniform over the nodes of the batch; scope='graph': the destination uniform over the source's own circuit, the
        candidates predict_links, reconstruct_edges and link_ranking rank a link against (recon_loss / link_metrics then need
        graph_ptr).  reverse: the share in [0, 1] of the negatives that are reversals (v, u) of true links (u, v), the hard negatives
        of a directed decoder.  Added functionality; a setting of the model object, not part of its state_dict."""
        if scope not in ('batch', 'graph'):
            raise ValueError("scope must be 'batch' or 'graph', got %r" % (scope,))
        reverse = float(reverse)
        if not 0.0 <= reverse <= 1.0:
            raise ValueError('reverse must lie in [0, 1], got %r' % reverse)
        self._neg_scope, self._neg_reverse = scope, reverse
        return self

    def _draw_negatives(self, hs, pos_edge_index, plan, edge_keys=None, graph_ptr=None):
        """Negative pairs as recon_loss draws them: with the batch's plan the fused device sampler (pairs bucketed for an atomic-free
        backward), else the torch rejection sampler; under set_negative_sampling the local draw of either."""
        scope, reverse = getattr(self, '_neg_scope', 'batch'), getattr(self, '_neg_reverse', 0.0)
        if scope == 'graph' and graph_ptr is None:
            raise ValueError("set_negative_sampling(scope='graph') needs the batch's graph_ptr: pass graph_ptr= to recon_loss / link_metrics")
        local = {} if scope == 'batch' and reverse == 0.0 else dict(graph_ptr=graph_ptr if scope == 'graph' else None, reverse=reverse)
        if plan is not None and hs.is_cuda and hs.shape[0] >= 2 and DEVICE_SAMPLER:
            return negative_sampling_device(plan, **local)
        return negative_sampling(pos_edge_index, hs.shape[0], keys=edge_keys, **local)

    def link_metrics(self, hs, pos_edge_index, neg_edge_index=None, plan=None, graph_ptr=None):
        """ROC-AUC and average precision of the decoder on st = hs_decompose(hs): `pos_edge_index` ranked against `neg_edge_index`
        (drawn as recon_loss draws them when None).  Added functionality: the reference's DG_AE Models have no such method, only
        DirectedGAE / DirectedGVAE.test (digvae_model.py:177-189), whose definition of the two numbers this follows.  Returns the
        device record of ops.link_record (float64[8]: AUC, AP, then the integer words) without a host synchronisation; `.tolist()`
        or ops.read_link_records is the caller's."""
        with torch.no_grad():
            if self.variational:
                st = torch.cat(self._decoder_halves(hs), dim=1)          # the posterior means
            else:
                st = ops.linear(hs.detach(), self.hs_decompose.weight, self.hs_decompose.bias)
            if plan is not None and (plan.E != pos_edge_index.shape[1] or plan.N != hs.shape[0]):
                plan = None
            if neg_edge_index is None:
                neg_edge_index = self._draw_negatives(hs, pos_edge_index, plan, graph_ptr=graph_ptr)
            return metrics.link_record(st, None, pos_edge_index, neg_edge_index)

    def _decoder_halves(self, hs):
        """(s, t): the two column halves of st = hs_decompose(hs), as views (the pair kernels take a row stride); of a variational
        model the posterior means (mu_s, mu_t) of those halves."""
        if self.variational:
            mu_s, _, mu_t, _ = self.latent(hs)
            return mu_s, mu_t
        st = ops.linear(hs.detach(), self.hs_decompose.weight, self.hs_decompose.bias)
        H = st.shape[1] // 2
        return st[:, :H], st[:, H:]

    # ---- variational link heads ----------------------------------------------------------------------
    def _var_heads(self):
        return tuple(p for name in self.VAR_HEADS for p in (getattr(self, name).weight, getattr(self, name).bias))

    def latent(self, hs):
        """(mu_s, logstd_s, mu_t, logstd_t) [N, H] each, of a variational model: the four heads on st = hs_decompose(hs), without
        gradients (column views of one array on the fused route)."""
        if not self.variational:
            raise ValueError('latent() needs Model(variational=True)')
        with torch.no_grad():
            st = ops.linear(hs.detach(), self.hs_decompose.weight, self.hs_decompose.bias)
            return ops.var_head_latent(st, self._var_heads())

    def kl_loss(self):
        """(s_kl, t_kl) of the last recon_loss exactly as trainer.py:146-147 writes them: -0.5/N * mean_i sum_d(1 + 2 logstd - mu^2 -
        exp(logstd)^2), i.e. -0.5 / N^2 times each half's sum (the double 1/N is the reference's)."""
        if self._klsum is None:
            raise ValueError('kl_loss() follows recon_loss() of a variational model')
        c = -0.5 / self._kl_n / self._kl_n
        return c * self._klsum[0], c * self._klsum[1]

    def predict_links(self, hs, k, graph_ptr=None, skip_self=True):
        """(idx [N, k] int32, score [N, k], n_above [N] int32) on st = hs_decompose(hs): every gate's k most probable fan-out targets
        inside its own graph (batch-wide ids, -1 / -inf past the end) and the number of candidates the decoder calls an edge
        (sigma > 0.5), streamed by ops.pair_topk without an N x N array.  Added functionality: the reference can only form the dense
        matrix (digae_layer.py:31-33)."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            return pairs.pair_topk(s, t, k, graph_ptr=graph_ptr, sigmoid=True, threshold=0.5, skip_self=skip_self)

    def reconstruction_counts(self, hs, edge_index, graph_ptr, threshold=0.5):
        """int64 [G, 4] per graph on the device: true positives, predicted positives over all n_g^2 ordered pairs, edges, ordered pairs
        (ops.reconstruction_counts) — the confusion of the decoder against the FULL adjacency, where recon_loss's counters see only
        sampled non-edges.  Precision and recall are the caller's two divisions."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            return pairs.reconstruction_counts(s, t, edge_index, graph_ptr, threshold)

    def reconstruction_curve(self, hs, edge_index, graph_ptr, thresholds):
        """int64 [G, B, 4] on the device: reconstruction_counts at every one of `thresholds` (strictly ascending, at most 256) — the
        precision-recall curve of the decoder against the FULL adjacency from ONE all-pairs walk instead of one per threshold
        (ops.reconstruction_curve: the score distribution of ops.pair_profile), entry for entry what reconstruction_counts gives at
        each threshold.  Added functionality: the reference can only form the dense matrix (digae_layer.py:31-33)."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            return pairs.reconstruction_curve(s, t, edge_index, graph_ptr, thresholds)

    def link_ranking(self, hs, edge_index, graph_ptr, ks=(1, 3, 10, 50), by='dst', filtered=True, plan=None):
        """(RankMetrics, LinkRanks) on st = hs_decompose(hs): where every true link stands among ALL candidates of its node — by='dst',
        the reconstruction question, every true fan-in of a gate among all gates of its circuit — as exact MRR, Hits@K (for both ends
        of a tie) and rank sums per graph (ops.rank_metrics), with the per-link ranks in edge_index's order (ops.link_ranks: one
        all-pairs walk per 32 links of a tile's busiest node, no N x N array).  filtered: a gate's other true links do not count
        against a link.  Added functionality: link_metrics and the reference's `test` rank against sampled non-edges, whose AUC
        saturates; reconstruction_counts sees the full adjacency only in aggregate at a threshold."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            ranks = metrics.link_ranks(s, t, edge_index, graph_ptr=graph_ptr, by=by, filtered=filtered, plan=plan)
            return metrics.rank_metrics(ranks, edge_index, graph_ptr, ks=ks, by=by), ranks

    def reconstruct_edges(self, hs, graph_ptr=None, threshold=0.5, skip_self=False, by='src', with_scores=False, max_edges=None):
        """(edge_index int64 [2, E'], row_ptr int64 [N + 1], score [E'] or None) on st = hs_decompose(hs): the graph the decoder
        reconstructs, every pair inside a graph with sigma > threshold, as (source, target) rows listed per source in ascending target
        order (by='dst': per target in ascending source order, the in-neighbour lists); row_ptr delimits the lists
        (ops.reconstruct_edges, streamed by ops.pair_select).  E' = reconstruction_counts(...)[:, 1].sum().  Added functionality."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            return pairs.reconstruct_edges(s, t, graph_ptr=graph_ptr, threshold=threshold, skip_self=skip_self, by=by,
                                           with_scores=with_scores, max_edges=max_edges)

    def similar_gates(self, hf, k, graph_ptr=None, threshold=0.999):
        """(idx [N, k] int32, cos [N, k], n_above [N] int32) on the functional embeddings hf: every gate's k functionally closest gates
        inside its own graph by cosine (batch-wide ids, -1 / -inf past the end) and the number of gates whose cosine with it is
        > threshold (ops.sim_topk, streamed without an N x N array).  Added functionality: it mirrors the functional loss,
        1 - cosine_similarity(hf[a], hf[b], eps=1e-8) regressed on truth-table distance (trainer.py:158-160), which the reference only
        evaluates on the listed training pairs.  Primary inputs and other never-updated nodes have hf = 0: their cosine is 0 with
        everything, so no positive threshold ever reports them.  Bit-identical or power-of-two-scaled rows score within
        (2H + 6) 2^-24 of 1 and are not clamped to it: threshold = 1.0 selects nothing reliably, hence the default 0.999."""
        return similarity.sim_topk(hf, k, graph_ptr=graph_ptr, threshold=threshold)

    def equivalence_candidates(self, hf, graph_ptr=None, threshold=0.999, with_scores=False, max_pairs=None):
        """(pair_index int64 [2, P] with pair_index[0] < pair_index[1], row_ptr int64 [N + 1], cos [P] or None): every unordered pair
        of gates of one graph whose functional embeddings have a cosine > threshold, once — the candidates for SAT sweeping and
        equivalence checking (ops.sim_pairs: unit rows, then the symmetric count / scan / fill; nothing of size N^2).  Added
        functionality: the search side of the functional loss 1 - cosine_similarity(hf[a], hf[b], eps=1e-8) (trainer.py:158-160).  More
        than `max_pairs` pairs raise HipLibraryError before anything is filled.  Primary inputs and other never-updated nodes have
        hf = 0 (cosine 0 with everything) and are never reported at a positive threshold; equal rows score within (2H + 6) 2^-24 of
        1, not exactly 1, so threshold = 1.0 selects nothing reliably and the default is 0.999."""
        return similarity.sim_pairs(hf, graph_ptr=graph_ptr, threshold=threshold, with_scores=with_scores, max_pairs=max_pairs)

    def equivalence_classes(self, hf, graph_ptr=None, threshold=0.999, min_size=2):
        """(label int32 [N], class_ptr int64 [C + 1], members int32 [M]): the equivalence candidate CLASSES of a batch, what a SAT sweeper
        consumes — the connected components of equivalence_candidates' relation (same graph, cosine of hf > threshold), computed on the
        device without the pair list (ops.sim_classes, route='walk': memory O(N); a class of 5,000 equal gates is 5,000 integers, not
        12.5 M pairs).  label[i] is the smallest id of gate i's class, so label[i] == i marks the representative the others are checked
        against; class c of the table is members[class_ptr[c] : class_ptr[c + 1]], ascending, for the classes with at least min_size
        gates.  Added functionality: the search side of the functional loss 1 - cosine_similarity(hf[a], hf[b], eps=1e-8)
        (trainer.py:158-160).  Single linkage: two gates of one class can have a cosine below the threshold.  Primary inputs and other
        never-updated nodes have hf = 0 (cosine 0 with everything) and are always singletons at a positive threshold, as are rows with
        a NaN; classes never cross graphs; equal rows score within (2H + 6) 2^-24 of 1, not exactly 1, so threshold = 1.0 is unreliable
        and the default is 0.999.  Exact and the same bits from run to run: equal to ops.components of equivalence_candidates."""
        return similarity.sim_classes(hf, graph_ptr=graph_ptr, threshold=threshold, min_size=min_size)

    def match_gates(self, hf, k, graph_ptr, peer, threshold=0.999):
        """(idx [N, k] int32, cos [N, k], n_above [N] int32) ACROSS circuits: every gate's k functionally closest gates in the PEER of
        its circuit by cosine of hf — peer [G]: the candidates of a gate of graph g are all gates of graph peer[g], -1 for none, g
        itself allowed (a gate is then its own candidate), many graphs may name one peer — as batch-wide ids, -1 / -inf past the
        end, and the number of the peer's gates whose cosine with it is > threshold (ops.cross_topk, streamed without an N x N
        array).  Added functionality: the candidate internal equivalence points between a golden design and its revision, where
        similar_gates looks inside one circuit; hf depends only on a circuit's own structure, so two circuits embedded by one model
        are comparable as they stand (trainer.py:158-160).  Primary inputs have hf = 0 (cosine 0 with everything) and are matched by
        name in practice; equal rows score within (2H + 6) 2^-24 of 1, not exactly 1, hence the default 0.999."""
        return similarity.cross_topk(hf, k, graph_ptr, peer, threshold=threshold)

    def cross_equivalence_candidates(self, hf, graph_ptr, peer, threshold=0.999, mutual=False, with_scores=False, max_pairs=None):
        """(pair_index int64 [2, P], row_ptr int64 [N + 1], cos [P] or None): every pair (gate u, gate v of the peer of u's circuit)
        whose hf have a cosine > threshold, listed per u in ascending v (ops.cross_pairs; peer as in match_gates).  With an
        involutive peer a pair appears once from each side.  mutual=True: only the reciprocal best matches — v is u's closest gate
        and u is v's — each once with u in the lower-indexed circuit (ops.cross_mutual), returned as (pair_index [2, M], None, cos
        [M] or None); it is defined where peer[peer[g]] = g and has no list to refuse.  More than `max_pairs` pairs raise
        HipLibraryError before anything is filled.  Added functionality (trainer.py:158-160): the cut points of combinational
        equivalence checking.  Primary inputs (hf = 0) are never reported at a positive threshold; use 0.999 rather than 1.0."""
        if mutual:
            pi, cos = similarity.cross_mutual(hf, graph_ptr, peer, threshold=threshold)
            return pi, None, (cos if with_scores else None)
        return similarity.cross_pairs(hf, graph_ptr, peer, threshold=threshold, with_scores=with_scores, max_pairs=max_pairs)

    def cross_equivalence_classes(self, hf, graph_ptr, peer, threshold=0.999, min_size=2, route='pairs'):
        """(label int32 [N], class_ptr int64 [C + 1], members int32 [M]) as equivalence_classes returns them, but the classes may span
        a circuit and its peer: the connected components of "cosine of hf > threshold" over the pairs of
        cross_equivalence_candidates together with those of equivalence_candidates (ops.cross_classes; peer as in match_gates).  A
        class that holds gates of both circuits is a set of candidate equivalence points a checker can merge.  Added functionality
        (trainer.py:158-160).  Single linkage; primary inputs (hf = 0) and rows with a NaN are always singletons; circuits share a
        class only through peer links; use 0.999 rather than 1.0.  route='pairs' builds both pair lists first and can refuse for
        their size; route='walk' unites the pairs where the two tile walks find them, in O(N) memory, and gives the same classes."""
        return similarity.cross_classes(hf, graph_ptr, peer, threshold=threshold, min_size=min_size, route=route)

    def cross_similarity_profile(self, hf, thresholds, graph_ptr, peer):
        """int64 [G, B] on the device: per graph g, the number of (gate of g, gate of graph peer[g]) pairs whose cosine of hf is > each
        of `thresholds` (strictly ascending, at most 256) — what cross_equivalence_candidates would list for g's gates at each of
        them, as integers, from ONE walk (ops.counts_above of ops.cross_profile; peer as in match_gates).  With an involutive peer a
        pair counts once in each of the two circuits' rows.  Added functionality (trainer.py:158-160): the distribution by which a
        threshold for matching a golden design against its revision is chosen instead of guessed.  Rows with hf = 0 score 0 with
        everything; equal rows score within (2H + 6) 2^-24 of 1, not exactly 1."""
        return pairs.counts_above(similarity.cross_profile(hf, thresholds, graph_ptr, peer))

    def cross_equivalence_threshold(self, hf, max_pairs, graph_ptr, peer, lo=0.0):
        """{'threshold', 'pairs', 'lower', 'pairs_lower', 'tight'}: the lowest cosine threshold above `lo` at which
        cross_equivalence_candidates lists at most `max_pairs` pairs for the whole batch, and exactly `pairs` of them
        (ops.cross_threshold_for: a few profile walks in place of a bisection of count walks; peer as in match_gates).  Pairs are
        counted as cross_equivalence_candidates lists them: with an involutive peer once from each side.  When `lower` is not None,
        cross_equivalence_candidates(threshold=lower, max_pairs=max_pairs) is refused: pairs_lower > max_pairs.  Added functionality
        (trainer.py:158-160).  Ties are the caller's to understand, as for equivalence_threshold: equal gates share ONE cosine value,
        which a threshold takes or leaves as a whole, so `pairs` can lie far below max_pairs."""
        return similarity.cross_threshold_for(hf, max_pairs, graph_ptr, peer, lo=lo)

    def similarity_profile(self, hf, thresholds, graph_ptr=None):
        """int64 [G, B] on the device: per graph, the number of unordered gate pairs whose cosine of hf is > each of `thresholds`
        (strictly ascending, at most 256) — what equivalence_candidates would list at each of them, as integers, from ONE walk
        (ops.counts_above of ops.sim_profile).  Added functionality: the distribution behind the functional loss
        1 - cosine_similarity(hf[a], hf[b], eps=1e-8) (trainer.py:158-160), by which a threshold is chosen instead of guessed.  Primary
        inputs and other never-updated nodes have hf = 0: they score 0 with everything.  Equal rows score within (2H + 6) 2^-24 of
        1, not exactly 1."""
        return pairs.counts_above(similarity.sim_profile(hf, thresholds, graph_ptr=graph_ptr))

    def equivalence_threshold(self, hf, max_pairs, graph_ptr=None, lo=0.0):
        """{'threshold', 'pairs', 'lower', 'pairs_lower', 'tight'}: the lowest cosine threshold above `lo` at which
        equivalence_candidates lists at most `max_pairs` pairs for the whole batch, and exactly `pairs` of them — "the 100,000 best
        candidates of this design" (ops.sim_threshold_for: a few profile walks in place of a bisection of count walks).  When `lower`
        is not None, equivalence_candidates(threshold=lower, max_pairs=max_pairs) is refused: pairs_lower > max_pairs.  Added
        functionality (trainer.py:158-160).  Ties are the caller's to understand: equal gates share ONE cosine value, which a threshold
        takes or leaves as a whole (5,000 equal gates are 12.5 M pairs), so `pairs` can lie far below max_pairs.  Rows with hf = 0
        score 0 with everything; equal rows score within (2H + 6) 2^-24 of 1, not exactly 1."""
        return similarity.sim_threshold_for(hf, max_pairs, graph_ptr=graph_ptr, lo=lo)

    def functional_similarity(self, hf, pair_index):
        """cos(hf[a], hf[b]) of the listed pairs [2, P]: 1 - this is the `dis` of the functional loss (trainer.py:158-160, eps = 1e-8 per
        row), in the arithmetic of similar_gates and equivalence_candidates — the same bits for the same pair.  Added functionality.
        A never-updated node (hf = 0) has cosine 0 with everything."""
        return similarity.sim_at(hf, pair_index)

    def function_accuracy(self, hf, tt_pair_index, tt_sim, graph_ptr=None, min_gap=0.05):
        """(acc float64 [G, B], counts int64 [G, B, 3] = eligible, concordant, tied) on the device: per circuit, the share of ALL
        comparisons of two listed truth-table pairs — those whose distances differ, and by at least min_gap (a float or up to 8 of
        them) — that 1 - functional_similarity orders the way the truth-table distance does (ops.function_accuracy, exact integer
        counts; G = 1 without graph_ptr).  It is what get_function_acc (utils/utils.py:111-147) estimates from 100 random draws per
        circuit; -1 where no comparison is eligible, as there.  A tie in the prediction is not correct, as there."""
        gaps = [min_gap] if isinstance(min_gap, (int, float)) else list(min_gap)
        return metrics.function_accuracy(hf, tt_pair_index, tt_sim, graph_ptr=graph_ptr, gaps=gaps)

    # ---- decode a legal circuit ------------------------------------------------------------------------
    def gate_arity(self, gate):
        """int32 like `gate`: the number of fan-ins the library gives each gate id (ARITY through this model's GATES); a primary input
        and an id the model does not know take none."""
        gate = torch.as_tensor(gate)
        ids = gate.flatten().to(torch.int64)
        table = torch.zeros(max([gid for _, gid in self.GATES] + [0]) + 1, dtype=torch.int32, device=ids.device)
        for name, gid in self.GATES:
            table[gid] = self.ARITY[name]
        known = (ids >= 0) & (ids < table.numel())
        return torch.where(known, table[ids.clamp(0, table.numel() - 1)], torch.zeros_like(ids, dtype=torch.int32)).view(gate.shape)

    def decode_circuit(self, hs, G, key=None, want=None, K=None):
        """DecodedCircuit(edge_index int64 [2, E'], fanin int32 [N, K], score [N, K], short bool [N]) on st = hs_decompose(hs) (of a
        variational model the posterior means): the embeddings of CircuitBatch G decoded into a circuit of this model's gate library —
        every gate gets its `want` best fan-ins among the nodes of its own circuit with a smaller `key`, so arities hold and the
        result is acyclic whatever the scores are (ops.fanin_decode, streamed without an N x N array).  key: G.forward_level by
        default (the plan's ASAP levels where the batch has none): every true fan-in of a levelised circuit is then a candidate.
        want: the library arity of each gate (gate_arity) by default, 'degree': the true in-degree, or a tensor.  fanin: -1 past a
        list's end; edge_index: sources on row 0, by target, then by rank; short: the gates with fewer candidates than they want.
        Added functionality: the reference decodes only scores (digae_layer.py:31-33)."""
        with torch.no_grad():
            s, t = self._decoder_halves(hs)
            N, dev = s.shape[0], s.device
            if key is None:
                if getattr(G, 'forward_level', None) is None:
                    plan_of(G, [gid for _, gid in self.GATES])            # levelises on the device and keeps the levels on the batch
                key = G.forward_level
            if want is None:
                want = self.gate_arity(G.gate.flatten())
            elif isinstance(want, str):
                if want != 'degree':
                    raise ValueError("want must be None (library arity), 'degree' (true in-degree) or a tensor, got %r" % (want,))
                want = torch.bincount(G.edge_index[1].to(dev), minlength=N)
            want = torch.as_tensor(want).to(dev)
            idx, score, n_cand = pairs.fanin_decode(s, t, torch.as_tensor(key).to(dev).flatten(), want, graph_ptr=getattr(G, 'graph_ptr', None),
                                                    K=K)
            return DecodedCircuit(pairs.fanin_edges(idx), idx, score, n_cand < want.flatten().to(torch.int32))

    def circuit_recovery(self, hs, G, key=None, want=None, K=None):
        """(FaninRecovery, DecodedCircuit): decode_circuit counted against G.edge_index — per circuit {gates, exact, hits, true_total,
        decoded_total} and the exact-recovery rate exact / gates (ops.fanin_recovery): whether the WHOLE fan-in set of a gate came
        back, the strictest reconstruction metric.  Added functionality."""
        with torch.no_grad():
            dec = self.decode_circuit(hs, G, key=key, want=want, K=K)
            return metrics.fanin_recovery(dec.fanin, G.edge_index, graph_ptr=getattr(G, 'graph_ptr', None)), dec

    def recon_loss(self, hs, pos_edge_index, neg_edge_index=None, want_pred=True, edge_keys=None, plan=None, want_rank=False,
                   expect_scale=1.0, graph_ptr=None, return_hs=False, sample=None, seed=None, eps=None, st=None):
        """`plan` (optional): the batch's GraphPlan when pos_edge_index is the batch's own edge set (any
        order) — the positive half of the backward then needs no atomics.  `return_hs`: a fourth result, hs passed through the
        hs_decompose node (ops.linear_passthrough; hs itself when it needs no gradient): a second consumer of hs that reads THAT
        tensor has its gradient added inside the Linear's input-gradient kernel.  `want_rank`: also rank the very pairs the loss
        uses (same st, same sampled negatives) and leave the ops.link_record tensor in `self.last_link_metrics`.  `expect_scale`: the
        upstream gradient this loss will meet in backward (its weight in the step's total), see ops.ReconLossFn.  `graph_ptr`: the
        batch's host graph table, read when negatives are drawn under set_negative_sampling(scope='graph').
        Variational model: the decoder reads z = VarHead(st) where it reads st otherwise, and the KL sums are kept for kl_loss().
        `sample`: add the noise (None: self.training, the VGAE convention; the reference's `sample` adds it in eval mode as well,
        DESIGN.md §7); `seed` fixes it (tests; by default one is drawn from torch's CPU generator, as pred_prob's); `eps` [N, 2H]
        injects it.  `st`: hs_decompose(hs) where the caller has it already (ops.linear_pair made it with hs); hs then has no
        consumer here and comes back as it is."""
        hs_pass = hs
        if st is None and return_hs and hs.requires_grad:
            st, hs_pass = ops.linear_passthrough(hs, self.hs_decompose.weight, self.hs_decompose.bias)
        elif st is None:
            st = ops.linear(hs, self.hs_decompose.weight, self.hs_decompose.bias)
        if self.variational:
            sample = self.training if sample is None else bool(sample)
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if sample and eps is None else 0
            st, self._klsum = ops.var_head(st, self._var_heads(), eps=eps, seed=seed, sample=sample)
            self._kl_n = hs.shape[0]
        if plan is not None and (plan.E != pos_edge_index.shape[1] or plan.N != hs.shape[0]):
            plan = None
        neg_csr = None
        if neg_edge_index is None:
            # with the batch's plan: fused device sampler, pairs bucketed for an atomic-free backward
            neg_edge_index = self._draw_negatives(hs, pos_edge_index, plan, edge_keys, graph_ptr)
        if plan is not None and hs.is_cuda and torch.is_tensor(neg_edge_index) and neg_edge_index.shape[1] > 0:
            # given negatives: bucket them once (cached on the tensor's identity) so that their gradient needs no atomics either
            # kept on the batch's plan (like its pair lists), not on the model: several batches with fixed negatives each keep theirs
            cache = getattr(plan, '_neg_cache', None)
            key = (neg_edge_index.data_ptr(), neg_edge_index._version, tuple(neg_edge_index.shape), hs.shape[0])
            if cache is None or cache[0] is not neg_edge_index or cache[1] != key:      # same tensor object, not written since
                from .sampling import bucket_negatives
                cache = plan._neg_cache = (neg_edge_index, key, bucket_negatives(neg_edge_index.long(), hs.shape[0]))
            neg_edge_index = cache[2]
        if isinstance(neg_edge_index, NegativeEdges):
            neg_csr, neg_edge_index = neg_edge_index.csr, neg_edge_index.edge_index
        loss, counts, pred_bin = ops.ReconLossFn.apply(st, pos_edge_index, neg_edge_index, want_pred, plan, neg_csr, expect_scale)
        self.last_confusion = counts        # {TP, FP, TN, FN} on device, no host copy needed for metrics
        self.last_link_metrics = metrics.link_record(st, None, pos_edge_index, neg_edge_index) if want_rank else None
        Ep, En = pos_edge_index.shape[1], neg_edge_index.shape[1]
        gt_bin = None
        if want_pred:
            gt_bin = torch.zeros(Ep + En, dtype=torch.int32, device=hs.device)
            gt_bin[:Ep] = 1
        return (loss, pred_bin if want_pred else None, gt_bin) + ((hs_pass,) if return_hs else ())

    # ---- checkpoints (dg_ae_model_aig.py:132-160) --------------------------------------------------
    def load(self, model_path):
        checkpoint = torch.load(model_path, map_location=lambda storage, loc: storage)
        src = checkpoint['state_dict']
        state = {}
        for k, v in src.items():
            state[k[7:] if k.startswith('module') and not k.startswith('module_list') else k] = v
        own = self.state_dict()
        for k in list(state):
            if k in own:
                if state[k].shape != own[k].shape:
                    print('Skip loading parameter {}, required shape{}, loaded shape{}.'.format(k, own[k].shape, state[k].shape))
                    state[k] = own[k]
            else:
                print('Drop parameter {}.'.format(k))
        for k in own:
            if k not in state:
                print('No param {}.'.format(k))
                state[k] = own[k]
        self.load_state_dict(state, strict=False)

    def load_pretrained(self, pretrained_model_path=''):
        if pretrained_model_path == '':
            pretrained_model_path = os.path.join(os.path.dirname(__file__), 'pretrained', 'model.pth')
        self.load(pretrained_model_path)
