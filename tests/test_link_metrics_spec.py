"""Specification of the link-prediction ranking metrics, checked without a GPU: the float64 restatement (tests/link_metrics_ref.py)
against the values the reference's own DirectedGVAE.test produced (tests/golden/g8_linkpred.npz, make_golden_linkpred.py) and against
sklearn; and the error cases of the Python surface that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
from link_metrics_ref import rank_stats  # noqa: E402

CASES = ('plain', 'ties', 'one')


def _cpu_scores(z, case):
    """The reference's route: fp32 gather, dot, torch.sigmoid on the CPU (digae_layer.py:26-29), positives first."""
    s, t = torch.from_numpy(z[case + '_s']), torch.from_numpy(z[case + '_t'])
    ei = torch.from_numpy(np.concatenate([z[case + '_pos'], z[case + '_neg']], axis=1))
    return torch.sigmoid((s[ei[0]] * t[ei[1]]).sum(dim=1)).numpy(), z[case + '_pos'].shape[1]


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_reference_values(case):
    z = load_golden('g8_linkpred')
    scores, P = _cpu_scores(z, case)
    r = rank_stats(scores, P)
    assert (r['P'], r['Q']) == (4000, 4256)
    assert abs(r['auc'] - float(z[case + '_auc'])) <= 1e-12
    assert abs(r['ap'] - float(z[case + '_ap'])) <= 1e-12
    if case == 'one':
        assert r['groups'] == 1 and r['auc'] == 0.5 and abs(r['ap'] - P / scores.size) <= 1e-15
    if case == 'ties':
        assert r['groups'] < scores.size - 1000          # the copied pairs do tie


@pytest.mark.parametrize('kind', ['random', 'quantised', 'saturated', 'negative_and_zero'])
def test_restatement_equals_sklearn(kind):
    metrics = pytest.importorskip('sklearn.metrics')
    rng = np.random.default_rng(7)
    P, Q = 2500, 4000
    y = np.concatenate([np.ones(P), np.zeros(Q)])
    x = rng.standard_normal(P + Q) + 0.8 * y
    if kind == 'random':
        s = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    elif kind == 'quantised':
        s = (np.round(16.0 / (1.0 + np.exp(-x))) / 16.0).astype(np.float32)
    elif kind == 'saturated':
        s = (1.0 / (1.0 + np.exp(-20.0 * x))).astype(np.float32)           # thousands of scores at exactly 1.0f and near 0
        assert (s == 1.0).sum() > 1000
    else:
        s = np.round(x * 4.0).astype(np.float32) / 4.0 + 0.0                # plain scores: negative values and exact zeros (+0.0f only:
                                                                            # a tie is a run of bit-equal scores, and a sigmoid gives no -0.0f)
        assert (s == 0.0).any() and (s < 0).any()
    r = rank_stats(s, P)
    assert abs(r['auc'] - metrics.roc_auc_score(y, s)) <= 1e-12
    assert abs(r['ap'] - metrics.average_precision_score(y, s)) <= 1e-12


def test_restatement_extremes():
    s = np.concatenate([np.linspace(0.6, 0.9, 30), np.linspace(0.1, 0.4, 50)]).astype(np.float32)
    r = rank_stats(s, 30)
    assert r['auc'] == 1.0 and r['ap'] == 1.0 and r['U2'] == 2 * 30 * 50
    r = rank_stats(s[::-1].copy(), 50)                  # every positive below every negative
    assert r['auc'] == 0.0 and r['U2'] == 0
    with pytest.raises(ValueError):
        rank_stats(np.array([0.5, np.nan], dtype=np.float32), 1)


def _pairs(n, num_nodes=8):
    g = torch.Generator().manual_seed(n)
    return torch.randint(0, num_nodes, (2, n), generator=g)


def test_one_class_raises_value_error_before_the_device_check():
    """P == 0 or Q == 0: sklearn's ValueError, from host sizes alone — CPU tensors never reach the device check."""
    from deepgate import digvae_model, ops
    s, t = torch.randn(8, 16), torch.randn(8, 16)
    empty = torch.zeros(2, 0, dtype=torch.long)
    model = digvae_model.DirectedGVAE(torch.nn.Identity(), 16)
    for pos, neg in ((empty, _pairs(5)), (_pairs(5), empty)):
        with pytest.raises(ValueError):
            ops.link_auc_ap(s, t, pos, neg)
        with pytest.raises(ValueError):
            ops.link_auc_ap(torch.cat([s, t], dim=1), None, pos, neg)
        with pytest.raises(ValueError):
            model.test(s, t, pos, neg)


def test_cpu_tensors_raise_hip_library_error():
    """Both classes present but the embeddings live on the host: no CPU implementation, like every other op."""
    from deepgate import digvae_model, ops
    from deepgate._hip import HipLibraryError
    s, t = torch.randn(8, 16), torch.randn(8, 16)
    with pytest.raises(HipLibraryError):
        ops.link_auc_ap(s, t, _pairs(5), _pairs(7))
    with pytest.raises(HipLibraryError):
        digvae_model.DirectedGVAE(torch.nn.Identity(), 16).test(s, t, _pairs(5), _pairs(7))


def test_val_auc_flag_defaults_off():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'multi-gate-vae_amd'))
    from config import get_parse_args
    assert get_parse_args(['--type', 'aig']).val_auc is False
    assert get_parse_args(['--type', 'aig', '--val_auc']).val_auc is True
