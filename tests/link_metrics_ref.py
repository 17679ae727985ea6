"""Float64 / integer restatement of the link-prediction ranking metrics (numpy only): what csrc/link_metrics.hip computes, in the
words of its specification.  n = P + Q fp32 scores, the first P positive; a tie group is a maximal run of bit-equal scores; per
group g in descending score order: p_g, q_g its positives / negatives, TP_g, FP_g the counts through g.
    U2 = sum_g p_g (2 (Q - FP_g) + q_g)          AUC = U2 / (2 P Q)         (mid-rank Mann-Whitney)
    AP = sum_g p_g TP_g / (TP_g + FP_g) / P                                  (sklearn's step-wise definition)"""
import math

import numpy as np


def rank_stats(scores, P):
    """{'U2', 'P', 'Q', 'groups': Python ints, 'auc', 'ap': floats} of fp32 `scores` whose first P entries are the positives."""
    s = np.ascontiguousarray(scores, dtype=np.float32).ravel()
    n, P = int(s.size), int(P)
    Q = n - P
    if P <= 0 or Q <= 0:
        raise ValueError('Only one class present')
    if np.isnan(s).any():
        raise ValueError('Input contains NaN')
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))      # unsigned order = float order, ties = equal bits
    order = np.argsort(~key, kind='stable')                                        # highest score first
    k = key[order]
    pos = (order < P).astype(np.int64)
    ends = np.flatnonzero(np.append(k[1:] != k[:-1], True))                        # last element of every tie group
    TP = np.cumsum(pos)[ends]
    tot = ends.astype(np.int64) + 1
    FP = tot - TP
    p = np.diff(TP, prepend=0)
    q = np.diff(FP, prepend=0)
    U2 = int((p * (2 * (Q - FP) + q)).sum(dtype=np.int64))                         # exact: at most 2 P Q < 2^62
    ap = math.fsum(p.astype(np.float64) * (TP.astype(np.float64) / tot.astype(np.float64))) / P
    return {'U2': U2, 'P': P, 'Q': Q, 'groups': int(ends.size), 'auc': U2 / (2 * P * Q), 'ap': ap}
