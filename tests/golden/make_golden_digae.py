#!/usr/bin/env python3
"""Generate tests/golden/g9_digae.npz by running the REFERENCE's own DiGAE baseline modules on the CPU: DirectedGCNConvEncoder and
SingleLayerDirectedGCNConvEncoder (digae_layer.py:73-211) under DirectedGAE (digae_model.py:106-168).

Set up like make_golden_linkpred.py: runs only where the reference checkout is present (MGV_REFERENCE = its DG_VAE directory),
third-party modules the reference imports come from tests/oracle_stubs/; the output is plain data, no reference source is copied.
    MGV_REFERENCE=.../DG_VAE python tests/golden/make_golden_digae.py

Graph (shared by all cases): two DAGs of 100 and 104 nodes in one batch (edges run from lower to higher ids inside a graph), with
one edge listed twice, one isolated node, primary inputs, primary outputs and one input with 70 consumers.  x: a gate class 0..5
per node, fed as float one-hot rows [N, 6]; xf: float rows [N, 3].  Negatives: as many fixed random pairs as there are edges.

Cases (prefix): a1b0 / a05b05 / a0b1 = (alpha, beta) with self loops, a1b0_nl = (1, 0) without; each 6 -> 64 -> 64 on the one-hot
rows.  float = xf -> 32 -> 16 at (1, 0, loops).  single = SingleLayerDirectedGCNConvEncoder 6 -> 64 at (1, 0, loops).
Per case: <p>_keys (state_dict key list), <p>_param_<key>, <p>_grad_<key>, <p>_hs / <p>_ht (hidden activations after the ReLU; not
for `single`), <p>_s, <p>_t, <p>_loss, <p>_pred_bin, and float_dx.  Parameters are those of torch.manual_seed(0) before construction.

No ReLU decision in the fixture depends on rounding: in every case the smallest hidden pre-activation magnitude is at least 1e-4 of
the layer's largest (asserted).  A random draw does not give that (tens of thousands of values per case, a few of them land that
close to zero), so after the draw the inputs are repaired: while some row holds such a value, the class (or the float row) of one
node in that row's neighbourhood is drawn again and kept unless more such rows result.  Rows whose list is empty (no self loops: isolated nodes, inputs or outputs) are
exactly zero by structure on any implementation and are left out of that check.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('MGV_REFERENCE')
if not REF:
    sys.exit('set MGV_REFERENCE to the reference checkout\'s DG_VAE directory')
sys.path.insert(0, os.path.join(ROOT, 'tests', 'oracle_stubs'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepgate  # noqa: E402  (the reference)
import deepgate.digae_layer as L  # noqa: E402
import deepgate.digae_model as M  # noqa: E402

assert os.path.abspath(deepgate.__file__).startswith(os.path.abspath(REF)), deepgate.__file__
assert callable(getattr(M.DirectedGAE, 'test', None)) and hasattr(L, 'DirectedGCNConvEncoder')

CASES = (('a1b0', 1.0, 0.0, True), ('a05b05', 0.5, 0.5, True), ('a0b1', 0.0, 1.0, True), ('a1b0_nl', 1.0, 0.0, False))


def draw_graph(rng):
    edges, off = [], 0
    for n, n_in in ((100, 8), (104, 10)):
        for v in range(n_in, n - 1):                      # node n-1 stays isolated
            for u in rng.choice(v, size=2, replace=False):
                edges.append((off + int(u), off + v))
        if off == 0:
            for v in rng.choice(np.arange(n_in, n - 1), size=70, replace=False):   # a 70-consumer input
                edges.append((0, int(v)))
        off += n
    edges.append(edges[5])                                 # a duplicate edge
    ei = np.array(edges, dtype=np.int64).T.copy()
    ei = ei[:, rng.permutation(ei.shape[1])]
    N = off
    cls = rng.integers(0, 6, N)
    xf = rng.standard_normal((N, 3)).astype(np.float32)
    neg = rng.integers(0, N, (2, ei.shape[1])).astype(np.int64)
    return N, ei, cls, xf, neg


def offenders(enc, x, ei, loops):
    """Rows with a hidden pre-activation below 1e-4 of its layer's largest magnitude."""
    bad = set()
    with torch.no_grad():
        for conv1, e in ((enc.source_conv.conv1, ei), (enc.target_conv.conv1, torch.flip(ei, [0]))):
            pre = conv1(x, e)
            live = torch.ones(pre.shape[0], dtype=torch.bool)
            if not loops:
                live = torch.zeros(pre.shape[0], dtype=torch.bool)
                live[e[1]] = True
            small = (pre.abs() < 1e-4 * pre[live].abs().max()) & live.unsqueeze(1)
            bad |= set(torch.nonzero(small.any(1)).reshape(-1).tolist())
    return sorted(bad)


def make_encoder(p):
    torch.manual_seed(0)
    if p == 'float':
        return L.DirectedGCNConvEncoder(3, 32, 16, 1.0, 0.0, True, False), True
    if p == 'single':
        return L.SingleLayerDirectedGCNConvEncoder(6, 64, 1.0, 0.0, True, False), True
    a, b, loops = {c[0]: c[1:] for c in CASES}[p]
    return L.DirectedGCNConvEncoder(6, 64, 64, a, b, loops, False), loops


def run_case(out, p, x, ei, neg, want_dx=False):
    enc, loops = make_encoder(p)
    model = M.DirectedGAE(enc, L.DirectedInnerProductDecoder())
    out[p + '_keys'] = np.array(list(enc.state_dict().keys()))
    for k, v in enc.state_dict().items():
        out['%s_param_%s' % (p, k)] = v.detach().numpy().copy()
    x = x.clone().requires_grad_(want_dx)
    if p != 'single':
        assert not offenders(enc, x.detach(), ei, loops), p
        out[p + '_hs'] = torch.relu(enc.source_conv.conv1(x, ei)).detach().numpy()
        out[p + '_ht'] = torch.relu(enc.target_conv.conv1(x, torch.flip(ei, [0]))).detach().numpy()
    s, t = model.encode(x, x, ei)
    loss, pred_bin, gt_bin = model.recon_loss(s, t, ei, neg)
    loss.backward()
    out[p + '_s'], out[p + '_t'] = s.detach().numpy(), t.detach().numpy()
    out[p + '_loss'] = np.float64(loss.item())
    out[p + '_pred_bin'] = pred_bin.numpy().astype(np.int32)
    for k, v in enc.named_parameters():
        out['%s_grad_%s' % (p, k)] = v.grad.numpy().copy()
    if want_dx:
        out[p + '_dx'] = x.grad.numpy().copy()


def main():
    torch.set_num_threads(4)
    seed = 20261017
    rng = np.random.default_rng(seed)
    N, ei_np, cls, xf, neg_np = draw_graph(rng)
    ei, neg = torch.from_numpy(ei_np), torch.from_numpy(neg_np)
    one_hot = lambda: torch.nn.functional.one_hot(torch.from_numpy(cls), 6).float()
    near = lambda i: [i] + ei_np[0][ei_np[1] == i].tolist() + ei_np[1][ei_np[0] == i].tolist()
    def bad_rows(float_case):
        if float_case:
            return offenders(make_encoder('float')[0], torch.from_numpy(xf), ei, True)
        return [i for p, a, b, loops in CASES for i in offenders(make_encoder(p)[0], one_hot(), ei, loops)]

    for float_case, arr in ((False, cls), (True, xf)):     # repair (see the module docstring): a redraw is kept unless it leaves more such rows
        bad = bad_rows(float_case)
        for _ in range(20000):
            if not bad:
                break
            node = rng.choice(near(bad[rng.integers(len(bad))]))
            old = arr[node].copy()
            arr[node] = rng.standard_normal(3).astype(np.float32) if float_case else rng.integers(0, 6)
            now = bad_rows(float_case)
            if len(now) <= len(bad):
                bad = now
            else:
                arr[node] = old
        else:
            raise SystemExit('the repair did not converge')
    out = {'edge_index': ei_np, 'neg_edge_index': neg_np, 'cls': cls.astype(np.uint8), 'xf': xf, 'graph_seed': np.int64(seed)}
    for p, _, _, _ in CASES:
        run_case(out, p, one_hot(), ei, neg)
    run_case(out, 'float', torch.from_numpy(xf), ei, neg, want_dx=True)
    run_case(out, 'single', one_hot(), ei, neg)
    path = os.path.join(HERE, 'g9_digae.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print('wrote %s (%d bytes, graph seed %d, N = %d, E = %d)' % (path, size, seed, N, ei_np.shape[1]))


if __name__ == '__main__':
    main()
