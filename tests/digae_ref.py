"""Plain-torch restatement of the DiGAE baseline (DirectedGCNConv and the encoders built from it, DirectedGAE.recon_loss), test
infrastructure only: what the HIP path is held to, in whatever dtype the inputs have (the tests feed float64).  Written from the
layer's definition — a per-edge weight din(col)^-alpha * dout(row)^-beta on (W x_row + b), summed into col, one appended self loop
per node — and pinned to arrays recorded from the reference's own modules (tests/golden/g9_digae.npz, test_digae_spec.py)."""
import torch

EPS = 1e-15


def with_loops(ei, n, self_loops):
    if not self_loops:
        return ei
    loop = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei, torch.stack([loop, loop])], dim=1)


def _inv_pow(deg, a):
    out = torch.zeros_like(deg)
    nz = deg > 0
    out[nz] = deg[nz] ** (-a)
    return out


def scales(ei, n, alpha, beta, self_loops, dtype=torch.float64):
    """r[i] = din(i)^-alpha over col, c[j] = dout(j)^-beta over row (0 where the degree is 0)."""
    row, col = with_loops(ei, n, self_loops)
    din = torch.zeros(n, dtype=dtype).index_add_(0, col, torch.ones(col.shape[0], dtype=dtype))
    dout = torch.zeros(n, dtype=dtype).index_add_(0, row, torch.ones(row.shape[0], dtype=dtype))
    return _inv_pow(din, alpha), _inv_pow(dout, beta)


def propagate(y, ei, alpha, beta, self_loops):
    """out[col] += r[col] c[row] y[row] per edge."""
    n = y.shape[0]
    r, c = scales(ei, n, alpha, beta, self_loops, y.dtype)
    row, col = with_loops(ei, n, self_loops)
    return torch.zeros_like(y).index_add_(0, col, (r[col] * c[row]).unsqueeze(1) * y[row])


def conv(x, W, b, ei, alpha=1.0, beta=0.0, self_loops=True):
    """The per-edge form: the Linear first, as the layer is written."""
    return propagate(x @ W.t() + b, ei, alpha, beta, self_loops)


def conv_factored(x, W, b, ei, alpha=1.0, beta=0.0, self_loops=True):
    """agg_i = r_i sum c_j x_j, rho_i = r_i sum c_j, out_i = W agg_i + rho_i b."""
    agg = propagate(x, ei, alpha, beta, self_loops)
    rho = propagate(torch.ones(x.shape[0], 1, dtype=x.dtype), ei, alpha, beta, self_loops)
    return agg @ W.t() + rho * b


def flip(ei):
    return torch.flip(ei, [0])


def encoder(p, pre, x_s, x_t, ei, alpha=1.0, beta=0.0, self_loops=True, relu_mask=None):
    """DirectedGCNConvEncoder: s = conv2(relu(conv1(x, ei)), flip(ei)), t = conv2(relu(conv1(x, flip(ei))), ei) with four Linear
    layers p[pre + 'source_conv.conv1.lin.weight'] ...  Returns (s, t, hidden_s, hidden_t).  relu_mask = (mask_s, mask_t) replaces
    the ReLU decisions (comparisons on somebody else's mask)."""
    def act(v, k):
        return torch.relu(v) if relu_mask is None else v * relu_mask[k].to(v.dtype)
    g = lambda half, layer: (p['%s%s_conv.%s.lin.weight' % (pre, half, layer)], p['%s%s_conv.%s.lin.bias' % (pre, half, layer)])
    a = (alpha, beta, self_loops)
    hs = act(conv(x_s, *g('source', 'conv1'), ei, *a), 0)
    s = conv(hs, *g('source', 'conv2'), flip(ei), *a)
    ht = act(conv(x_t, *g('target', 'conv1'), flip(ei), *a), 1)
    t = conv(ht, *g('target', 'conv2'), ei, *a)
    return s, t, hs, ht


def single_layer_encoder(p, pre, s0, t0, ei, alpha=1.0, beta=0.0, self_loops=True):
    """SingleLayerDirectedGCNConvEncoder with its cross wiring: s_1 = source_conv(t_0) over flip(ei), t_1 = target_conv(s_0) over ei."""
    a = (alpha, beta, self_loops)
    s1 = conv(t0, p[pre + 'source_conv.conv.lin.weight'], p[pre + 'source_conv.conv.lin.bias'], flip(ei), *a)
    t1 = conv(s0, p[pre + 'target_conv.conv.lin.weight'], p[pre + 'target_conv.conv.lin.bias'], ei, *a)
    return s1, t1


def recon_loss(s, t, pos, neg):
    """(loss, pred_bin) of DirectedGAE.recon_loss with the negatives given."""
    pp = torch.sigmoid((s[pos[0]] * t[pos[1]]).sum(1))
    pn = torch.sigmoid((s[neg[0]] * t[neg[1]]).sum(1))
    loss = -torch.log(pp + EPS).mean() - torch.log(1 - pn + EPS).mean()
    return loss, (torch.cat([pp, pn]) > 0.5).int()
