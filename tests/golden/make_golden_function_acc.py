#!/usr/bin/env python3
"""Generate tests/golden/g10_function_acc.npz by running the REFERENCE's own `get_function_acc` (utils/utils.py:111-147) on the CPU
with the `random` that module sees replaced by an enumerator: `sample` hands out every unordered index pair of the circuit's listed
truth-table pairs once and a repeated index ever after (equal distances: the function skips it until its retries run out).  Every
circuit here lists at most 12 pairs, at most 66 comparisons, below the function's stop at 100 — so what it returns is exactly
concordant / eligible over ALL comparisons, or -1 when none is eligible.

Set up like make_golden.py: runs only where a checkout of the reference is present (its DG_VAE directory is the first argument or
$MGV_REFERENCE), third-party modules the reference imports come from tests/oracle_stubs/; the output is plain data, no reference
source is copied.  Usage:
    python tests/golden/make_golden_function_acc.py <reference>/DG_VAE

Arrays: hf [N, 16] float32, pairs int64 [2, P] (batch-wide node ids, grouped by circuit), tt_dis float32 [P], graph_ptr int64 [G + 1]
(nodes), seg_ptr int64 [G + 1] (pairs), acc float64 [G].  Circuits:
  0 - 3  random embeddings (one node of circuit 1 is a zero row: cosine 0 with everything) and random distances on a 0.01 grid
  4      planted ties in the prediction: one pair listed twice, and (a, b) beside (b, a), each with different distances
  5      planted distances: 0 beside float32(0.05) (exactly at the gap: eligible), beside the float32 one ulp below it (not eligible),
         two equal distances, and two more far away
  6      all distances equal: nothing is eligible, the function returns -1
Predicted distances of one circuit differ by more than 1e-3 wherever they are not bit-equal by construction (asserted), so an
implementation whose cosine differs in the last bits orders them the same way.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('MGV_REFERENCE', '')
assert REF and os.path.isdir(REF), 'give the reference checkout\'s DG_VAE directory (argument or $MGV_REFERENCE)'
sys.path.insert(0, os.path.join(ROOT, 'tests', 'oracle_stubs'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepgate  # noqa: E402  (the reference)
from deepgate.utils import utils as ref_utils  # noqa: E402

assert os.path.abspath(deepgate.__file__).startswith(os.path.abspath(REF)), deepgate.__file__

H = 16
F32 = np.float32


class Enumerator:
    """Stands in for the `random` module inside the reference's utils: every unordered pair of the population once, then (0, 0)."""

    def __init__(self):
        self.todo = None

    def sample(self, population, k):
        assert k == 2
        n = len(population)
        if self.todo is None:
            self.todo = [(p, q) for p in range(n) for q in range(p + 1, n)]
        return list(self.todo.pop(0)) if self.todo else [0, 0]


def circuits(rng):
    """[(hf [n, H], local pairs [2, p], tt_dis [p]), ...]"""
    out = []
    for c in range(4):
        n, p = 9 + c, (5, 12, 8, 11)[c]
        hf = rng.uniform(-1, 1, (n, H)).astype(F32)
        if c == 1:
            hf[0] = 0.0
        cand = [(a, b) for a in range(n) for b in range(a + 1, n)]
        pick = rng.choice(len(cand), p, replace=False)
        pairs = np.array([cand[i] for i in pick], dtype=np.int64).T.copy()
        if c == 1:
            pairs[:, 0] = (0, 3)                                  # the zero row is listed
        out.append((hf, pairs, (rng.integers(0, 100, p) * 0.01).astype(F32)))
    hf = rng.uniform(-1, 1, (8, H)).astype(F32)
    pairs = np.array([(1, 2), (3, 4), (1, 2), (5, 6), (4, 3), (0, 7), (2, 6)], dtype=np.int64).T.copy()
    out.append((hf, pairs, np.array([0.10, 0.40, 0.90, 0.25, 0.70, 0.55, 0.0], dtype=F32)))
    at = F32(0.05)
    hf = rng.uniform(-1, 1, (10, H)).astype(F32)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (0, 9), (1, 8)], dtype=np.int64).T.copy()
    out.append((hf, pairs, np.array([0.0, at, np.nextafter(at, F32(0)), 0.5, 0.5, 0.8, 0.3], dtype=F32)))
    hf = rng.uniform(-1, 1, (7, H)).astype(F32)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (1, 6)], dtype=np.int64).T.copy()
    out.append((hf, pairs, np.full(4, 0.375, dtype=F32)))
    return out


def main():
    rng = np.random.default_rng(20261020)
    hfs, prs, dis, gp, sp, acc = [], [], [], [0], [0], []
    for c, (hf, pairs, tt) in enumerate(circuits(rng)):
        assert pairs.shape[1] <= 12
        emb = torch.from_numpy(hf)
        pred = 1 - torch.cosine_similarity(emb[pairs[0]], emb[pairs[1]], eps=1e-8)
        gaps = (pred[:, None] - pred[None, :]).abs()
        assert bool(((gaps == 0) | (gaps > 1e-3)).all()), 'circuit %d: predicted distances too close for another arithmetic' % c
        ref_utils.random = Enumerator()
        g = types.SimpleNamespace(tt_pair_index=torch.from_numpy(pairs), tt_dis=torch.from_numpy(tt))
        with torch.no_grad():
            a = ref_utils.get_function_acc(g, emb)
        assert ref_utils.random.todo == [], 'the function stopped before every comparison was made'
        print('circuit %d: %d nodes, %d pairs, accuracy %.17g, %d tied predictions' % (c, hf.shape[0], pairs.shape[1], a,
                                                                                     (int((gaps == 0).sum()) - pairs.shape[1]) // 2))
        hfs.append(hf)
        prs.append(pairs + gp[-1])
        dis.append(tt)
        acc.append(float(a))
        gp.append(gp[-1] + hf.shape[0])
        sp.append(sp[-1] + pairs.shape[1])
    path = os.path.join(HERE, 'g10_function_acc.npz')
    np.savez_compressed(path, hf=np.concatenate(hfs), pairs=np.concatenate(prs, axis=1), tt_dis=np.concatenate(dis),
                        graph_ptr=np.array(gp, dtype=np.int64), seg_ptr=np.array(sp, dtype=np.int64), acc=np.array(acc, dtype=np.float64))
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
