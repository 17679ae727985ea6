#!/usr/bin/env python3
"""Generate tests/golden/g8_linkpred.npz by running the REFERENCE's own `DirectedGVAE.test` (digvae_model.py:177-189: decode both
edge sets with sigmoid=True, sklearn's roc_auc_score / average_precision_score) on the CPU.

Set up like make_golden.py: runs only where the reference checkout and sklearn are present, third-party modules the reference imports
come from tests/oracle_stubs/; the output is plain data, no reference source is copied.  Usage:
    python tests/golden/make_golden_linkpred.py

s, t [256, 64] fp32 drawn 0.3 * randn, 4,000 positive and 4,256 negative pairs, three cases (arrays <case>_s, _t, _pos, _neg, _auc, _ap):
  plain   random pairs; a pair is made positive with a probability that grows with its float64 logit, so AUC is clearly above 0.5
          (logits have a standard deviation of ~0.7 at this scale: no score saturates)
  ties    a quarter of the negatives are copies of positive pairs and a quarter of the positives are repeated: equal rows give
          bit-equal scores on any implementation, so the tie structure does not depend on rounding
  one     s = 0: every score is 0.5f, one tie group; AUC is exactly 0.5 and AP exactly P / n
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'oracle_stubs'))
sys.path.insert(0, '/root/reference/DG_VAE')

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepgate  # noqa: E402  (the reference)
import deepgate.digvae_model  # noqa: E402

assert deepgate.__file__.startswith('/root/reference'), deepgate.__file__

N, H, P, Q = 256, 64, 4000, 4256


def draw_case(case, rng):
    s = (0.3 * rng.standard_normal((N, H))).astype(np.float32)
    t = (0.3 * rng.standard_normal((N, H))).astype(np.float32)
    if case == 'one':
        s[:] = 0.0
    # candidate pairs, labelled by a Bernoulli draw whose probability grows with the float64 logit
    pos, neg = [], []
    while len(pos) < P or len(neg) < Q:
        u, v = rng.integers(0, N, 4096), rng.integers(0, N, 4096)
        logit = np.einsum('ij,ij->i', s[u].astype(np.float64), t[v].astype(np.float64))
        is_pos = rng.random(4096) < 1.0 / (1.0 + np.exp(-2.0 * logit))
        pos += list(zip(u[is_pos], v[is_pos]))
        neg += list(zip(u[~is_pos], v[~is_pos]))
    pos, neg = np.array(pos[:P], dtype=np.int64).T.copy(), np.array(neg[:Q], dtype=np.int64).T.copy()
    if case == 'ties':
        neg[:, :Q // 4] = pos[:, :Q // 4]                       # negatives that are copies of positive pairs
        pos[:, P - P // 4:] = pos[:, P // 4:P // 4 + P // 4]    # repeated positives
    return s, t, pos, neg


def main():
    rng = np.random.default_rng(20261016)
    model = deepgate.digvae_model.DirectedGVAE(torch.nn.Identity(), H)
    out = {}
    for case in ('plain', 'ties', 'one'):
        s, t, pos, neg = draw_case(case, rng)
        with torch.no_grad():
            auc, ap = model.test(torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(pos), torch.from_numpy(neg))
        out.update({case + '_s': s, case + '_t': t, case + '_pos': pos, case + '_neg': neg,
                    case + '_auc': np.float64(auc), case + '_ap': np.float64(ap)})
        print('%-5s AUC %.17g  AP %.17g' % (case, auc, ap))
    path = os.path.join(HERE, 'g8_linkpred.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
