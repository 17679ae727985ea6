"""Structural encoder / decoder surface of the reference (`DG_VAE/deepgate/digae_layer.py:26-33,
73-211, 232-297`) on top of the HIP kernels.  Module and parameter names, shapes, construction order
(hence seeded initialisation) and call signatures follow the reference, so its checkpoints load and
`train.py` builds the encoder the same way; the arithmetic is `ops.StructEncoderFn` for the multi-gate
encoder and `ops.DiGCNGatherFn` / `ops.DiGCNClassFn` around the linear kernels for the DiGAE baseline.
"""
import torch
import torch.nn as nn

from . import metrics, ops, pairs
from .arch.gcn_conv import AggConv
from .graph_plan import GraphPlan

MAX_FEATURE_CLASSES = 8


def feature_classes(x):
    """Distinct rows of the node-feature matrix and each node's row id.  The kernels add the GRU's
    feature term as a per-class table (`W_ih[:, H:] x_c + b_ih`), exact for any x with few distinct
    rows — the reference always feeds one-hot rows (dg_ae_model_aig.py:59)."""
    rows, inv = torch.unique(x, dim=0, return_inverse=True)
    if rows.shape[0] > MAX_FEATURE_CLASSES:
        return None                          # general features: MultiGCNEncoder.forward forms the term per node (_forward_rows)
    return rows.to(torch.float32), inv.to(torch.uint8).contiguous()


class DirectedInnerProductDecoder(nn.Module):
    """sigma(<s[src], t[dst]>) per edge (digae_layer.py:26-33)."""

    def forward(self, s, t, edge_index, sigmoid=True):
        return ops.edge_dot(s, t, edge_index, sigmoid)

    def forward_all(self, s, t, sigmoid=True):
        # dense M x N scores at any size that fits the device (ops.PairScoresFn, under autograd); beyond that: topk
        return pairs.pair_scores(s, t, sigmoid)

    def topk(self, s, t, k, graph_ptr=None, sigmoid=True, threshold=0.5, skip_self=False):
        """The streaming form of forward_all (added functionality: the reference has only the dense matrix): per node its k best
        links inside its own graph and the number of candidates scored above `threshold`, (idx, score, n_above) of ops.pair_topk."""
        return pairs.pair_topk(s, t, k, graph_ptr=graph_ptr, sigmoid=sigmoid, threshold=threshold, skip_self=skip_self)

    def select(self, s, t, graph_ptr=None, sigmoid=True, threshold=0.5, skip_self=False, by='src', with_scores=False, max_edges=None):
        """The decoded graph itself (added functionality): per node the list of ALL links inside its own graph scored above `threshold`,
        by source or (by='dst') by target, (row_ptr, col, score or None) of ops.pair_select; no N x N array and no cap per node."""
        return pairs.pair_select(s, t, graph_ptr=graph_ptr, sigmoid=sigmoid, threshold=threshold, skip_self=skip_self, by=by,
                                 with_scores=with_scores, max_edges=max_edges)

    def reconstruction_curve(self, s, t, edge_index, graph_ptr, thresholds):
        """The confusion of `select` against the full adjacency at every one of `thresholds` from one walk (added functionality):
        int64 [G, B, 4] of ops.reconstruction_curve — true positives, predicted positives, edges, ordered pairs per graph."""
        return pairs.reconstruction_curve(s, t, edge_index, graph_ptr, thresholds)

    def decode_fanins(self, s, t, key, want, graph_ptr=None, K=None, skip=True):
        """A legal circuit from the scores (added functionality): per node its `want` best fan-ins among the nodes of its own graph
        with a smaller order `key` — acyclic whatever the scores are — as (idx, score, n_cand) of ops.fanin_decode."""
        return pairs.fanin_decode(s, t, key, want, graph_ptr=graph_ptr, K=K, skip=skip)

    def rank(self, s, t, edge_index, graph_ptr=None, by='src', skip_self=False, filtered=True, plan=None):
        """Where every listed link stands among ALL candidates of its node by raw score (added functionality: the reference's `test`
        ranks against sampled non-edges): LinkRanks(rank_lo, rank_hi, valid) of ops.link_ranks, in the caller's edge order."""
        return metrics.link_ranks(s, t, edge_index, graph_ptr=graph_ptr, by=by, skip_self=skip_self, filtered=filtered, plan=plan)


def _classes_once(x, classes, width):
    """Integer one-hot rows -> (rows, ids) once per encoder call (feature_classes runs a torch.unique with a host read-back); float
    rows and rows of another width are left to the layer."""
    if classes is None and x is not None and not torch.is_floating_point(x) and x.shape[1] == width:
        return feature_classes(x)
    return classes


class DirectedGCNConv(nn.Module):
    """out_i = sum_{j in L(i)} din(i)^-alpha dout(j)^-beta (W x_j + b) (digae_layer.py:73-114).  The reference flips edge_index to turn
    the layer round; here `reverse` picks the plan's other CSR.  `classes` = (rows [C, F], row id per node uint8 [N]) stands in for x:
    the Linear is then applied to the C rows only.  `relu`: the F.relu the two-layer encoders put behind conv1, fused into the sum."""

    def __init__(self, in_channels, out_channels, alpha=1.0, beta=0.0, self_loops=True, adaptive=False):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels)
        self.alpha = alpha
        self.beta = beta
        self.self_loops = self_loops
        self.adaptive = adaptive             # stored, unused: the reference's adaptive branch is commented out (:78-83)

    def forward(self, x, edge_index, plan=None, reverse=False, classes=None, relu=False):
        F_ = self.lin.in_features
        args = (reverse, self.alpha, self.beta, self.self_loops is True, relu)
        if classes is None and not torch.is_floating_point(x) and x.shape[1] == F_:
            classes = feature_classes(x)     # integer one-hot rows, what the reference's Models build (None: too many distinct rows)
        if classes is not None:
            rows, xcls = classes
            if rows.shape[1] != F_:
                raise ValueError('expected %d node features, got %d' % (F_, rows.shape[1]))
            if plan is None:
                plan = GraphPlan(edge_index, xcls.shape[0])
            table = rows.to(self.lin.weight.device) @ self.lin.weight.t() + self.lin.bias      # [C, out]: weight space, autograd differentiates it
            return ops.DiGCNClassFn.apply(table, plan, xcls, *args)
        if x.shape[1] != F_:
            raise ValueError('expected %d node features, got %d' % (F_, x.shape[1]))
        if plan is None:
            plan = GraphPlan(edge_index, x.shape[0])
        pad = (-F_) % 16                     # the linear kernels' 16-column granule, as MultiGCNEncoder._forward_rows pads
        xp = torch.nn.functional.pad(x.to(torch.float32), (0, pad)) if pad else x.to(torch.float32)
        w = torch.nn.functional.pad(self.lin.weight, (0, pad)) if pad else self.lin.weight
        return ops.DiGCNGatherFn.apply(ops.linear(xp.contiguous(), w, self.lin.bias), plan, *args)


class SourceGCNConvEncoder(nn.Module):
    """conv2(relu(conv1(x, ei)), flip(ei)) (digae_layer.py:118-133)."""
    FIRST_REVERSE = False

    def __init__(self, in_channels, hidden_channels, out_channels, alpha=1.0, beta=0.0, self_loops=True, adaptive=False):
        super().__init__()
        self.conv1 = DirectedGCNConv(in_channels, hidden_channels, alpha, beta, self_loops, adaptive)
        self.conv2 = DirectedGCNConv(hidden_channels, out_channels, alpha, beta, self_loops, adaptive)

    def forward(self, x, edge_index, plan=None, classes=None):
        if plan is None:
            plan = GraphPlan(edge_index, (classes[1] if classes is not None else x).shape[0])
        h = self.conv1(x, edge_index, plan, self.FIRST_REVERSE, classes, relu=True)
        return self.conv2(h, edge_index, plan, not self.FIRST_REVERSE)


class TargetGCNConvEncoder(SourceGCNConvEncoder):
    """conv2(relu(conv1(x, flip(ei))), ei) (digae_layer.py:137-152)."""
    FIRST_REVERSE = True


class DirectedGCNConvEncoder(nn.Module):
    """The DiGAE baseline encoder of `--model AE` (digae_layer.py:156-165)."""

    def __init__(self, in_channels, hidden_channels, out_channels, alpha=1.0, beta=0.0, self_loops=True, adaptive=False):
        super().__init__()
        self.source_conv = SourceGCNConvEncoder(in_channels, hidden_channels, out_channels, alpha, beta, self_loops, adaptive)
        self.target_conv = TargetGCNConvEncoder(in_channels, hidden_channels, out_channels, alpha, beta, self_loops, adaptive)

    def forward(self, s, t, edge_index, plan=None, classes=None):
        if plan is None:
            plan = GraphPlan(edge_index, (classes[1] if classes is not None else s).shape[0])
        F_ = self.source_conv.conv1.lin.in_features
        cs = _classes_once(s, classes, F_)
        ct = cs if (classes is not None or t is s) else _classes_once(t, None, F_)
        return self.source_conv(s, edge_index, plan, cs), self.target_conv(t, edge_index, plan, ct)


class SingleLayerSourceGCNConvEncoder(nn.Module):
    """conv(x, flip(ei)) (digae_layer.py:174-184)."""
    REVERSE = True

    def __init__(self, in_channels, out_channels, alpha=1.0, beta=0.0, self_loops=True, adaptive=False):
        super().__init__()
        self.conv = DirectedGCNConv(in_channels, out_channels, alpha, beta, self_loops, adaptive)

    def forward(self, x, edge_index, plan=None, classes=None):
        return self.conv(x, edge_index, plan, self.REVERSE, classes)


class SingleLayerTargetGCNConvEncoder(SingleLayerSourceGCNConvEncoder):
    """conv(x, ei) (digae_layer.py:188-198)."""
    REVERSE = False


class SingleLayerDirectedGCNConvEncoder(nn.Module):
    """s_1 = source_conv(t_0), t_1 = target_conv(s_0): the reference's cross wiring (digae_layer.py:202-211)."""

    def __init__(self, in_channels, out_channels, alpha=1.0, beta=0.0, self_loops=True, adaptive=False):
        super().__init__()
        self.source_conv = SingleLayerSourceGCNConvEncoder(in_channels, out_channels, alpha, beta, self_loops, adaptive)
        self.target_conv = SingleLayerTargetGCNConvEncoder(in_channels, out_channels, alpha, beta, self_loops, adaptive)

    def forward(self, s_0, t_0, edge_index, plan=None, classes=None):
        if plan is None:
            plan = GraphPlan(edge_index, (classes[1] if classes is not None else s_0).shape[0])
        F_ = self.source_conv.conv.lin.in_features
        cs = _classes_once(s_0, classes, F_)
        ct = cs if (classes is not None or t_0 is s_0) else _classes_once(t_0, None, F_)
        return self.source_conv(t_0, edge_index, plan, ct), self.target_conv(s_0, edge_index, plan, cs)


class MultiGCNEncoder(nn.Module):
    def __init__(self, num_rounds, dim_hidden, dim_feature, enable_reverse, layernorm):
        super().__init__()
        self.num_rounds = num_rounds
        self.enable_reverse = True          # the reference forces this on (digae_layer.py:238)
        self.layernorm = layernorm
        self.dim_feature = dim_feature
        self.dim_hidden = dim_hidden
        self.aggr = AggConv(dim_hidden, dim_hidden)
        self.update = nn.GRU(dim_hidden + dim_feature, dim_hidden)
        self.aggr_r = AggConv(dim_hidden, dim_hidden)
        self.update_r = nn.GRU(dim_hidden + dim_feature, dim_hidden)
        if self.layernorm:
            self.ln = nn.LayerNorm(dim_hidden)

    def _composed(self, aggr, gru, feat_rows):
        """Fold the per-edge message Linear into the GRU input projection (tiny weight-space
        products; autograd differentiates them)."""
        H = self.dim_hidden
        w_ih = gru.weight_ih_l0
        w_m = w_ih[:, :H]
        Wc = w_m @ aggr.msg.weight
        bc = w_m @ aggr.msg.bias
        xtab = feat_rows @ w_ih[:, H:].t() + gru.bias_ih_l0
        return xtab, Wc, bc, gru.weight_hh_l0, gru.bias_hh_l0

    def _forward_rows(self, x, edge_index, plan):
        """General node features (more distinct rows than the class table holds; digae_layer.py:257-277 takes any x [N, F]): the GRU's
        feature term W_ih[:, H:] x_i + b_ih per node through the linear kernels (x zero-padded to their 16-column granule), every
        half round per node on the exact-fp32 stage kernels (ops.StructEncoderRowsFn)."""
        H, F_ = self.dim_hidden, self.dim_feature
        if plan is None:
            plan = GraphPlan(edge_index, x.shape[0])
        pad = (-F_) % 16
        xp = torch.nn.functional.pad(x.to(torch.float32), (0, pad)).contiguous()
        args = []
        for aggr, gru in ((self.aggr, self.update), (self.aggr_r, self.update_r)):
            w_ih = gru.weight_ih_l0
            w_m = w_ih[:, :H]
            w_x = torch.nn.functional.pad(w_ih[:, H:], (0, pad))
            # one Linear per gate block (the linear kernels serve M = H outputs, not 3H), side by side
            xrow = torch.cat([ops.linear(xp, w_x[g * H:(g + 1) * H], gru.bias_ih_l0[g * H:(g + 1) * H]) for g in range(3)], dim=1)
            args += [xrow, w_m @ aggr.msg.weight, w_m @ aggr.msg.bias, gru.weight_hh_l0, gru.bias_hh_l0]
        ln_w = self.ln.weight if self.layernorm else None
        ln_b = self.ln.bias if self.layernorm else None
        return ops.StructEncoderRowsFn.apply(plan, self.num_rounds, *args, ln_w, ln_b)

    def forward(self, x, edge_index, plan=None, classes=None):
        """`classes` = (distinct feature rows [C,F], row id per node uint8 [N]) may stand in for x."""
        if classes is None:
            if x.shape[1] != self.dim_feature:
                raise ValueError('expected %d node features, got %d' % (self.dim_feature, x.shape[1]))
            classes = feature_classes(x)
        if classes is None:
            return self._forward_rows(x, edge_index, plan)
        rows, xcls = classes
        if rows.shape[1] != self.dim_feature:
            raise ValueError('expected %d node features, got %d' % (self.dim_feature, rows.shape[1]))
        if plan is None:
            plan = GraphPlan(edge_index, xcls.shape[0])
        rows = rows.to(self.update.weight_ih_l0.device)
        f = self._composed(self.aggr, self.update, rows)
        r = self._composed(self.aggr_r, self.update_r, rows)
        ln_w = self.ln.weight if self.layernorm else None
        ln_b = self.ln.bias if self.layernorm else None
        return ops.StructEncoderFn.apply(plan, xcls, self.num_rounds, *f, *r, ln_w, ln_b)


class DirectMultiGCNEncoder(nn.Module):
    def __init__(self, dim_feature=3, dim_hidden=128, s_rounds=1, t_rounds=1, enable_reverse=True, layernorm=False):
        super().__init__()
        self.source_conv = MultiGCNEncoder(s_rounds, dim_hidden, dim_feature, enable_reverse, layernorm)
        self.target_conv = MultiGCNEncoder(t_rounds, dim_hidden, dim_feature, enable_reverse, layernorm)

    def forward(self, s, t, edge_index, plan=None, classes=None):
        if plan is None:
            plan = GraphPlan(edge_index, s.shape[0])
        cs = classes if classes is not None else feature_classes(s)
        ct = cs if (classes is not None or t is s) else feature_classes(t)
        # (None: more distinct feature rows than the class table holds -> the per-node feature path of MultiGCNEncoder)
        return self.source_conv(s, edge_index, plan, cs), self.target_conv(t, edge_index, plan, ct)
