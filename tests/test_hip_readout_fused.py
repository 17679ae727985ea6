"""The fused training-mode readout (ops.ReadoutMLPFn, csrc/readout_fused_x3.hip) against the per-layer path it replaces
(linear / BnReluDropFn / HeadFn, arch/mlp.py with FUSED_READOUT off) on the same seeded inputs and parameters: the same dropout
masks, prob to reordering, every gradient and dhf to 1e-5 of its scale (the two noise-valued bias gradients bit for bit), the
running buffers to 1 ulp, and bit-identical gradients when a step is repeated."""
import copy

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on the path)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _mlp(p_drop, dev):
    from deepgate.arch.mlp import MLP
    torch.manual_seed(3)
    m = MLP(64, 32, 1, num_layer=3, p_drop=0.2, norm_layer='batchnorm', act_layer='relu')
    with torch.no_grad():
        for k in (1, 5):                  # non-trivial affine parameters and running buffers
            m.fc[k].weight.uniform_(0.5, 1.5)
            m.fc[k].bias.uniform_(-0.3, 0.3)
            m.fc[k].running_mean.uniform_(-0.1, 0.1)
            m.fc[k].running_var.uniform_(0.5, 1.5)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
    return m.to(dev).train()


def _close_prob(a, b):
    """Same clamp decisions, values to 1e-6 of the tensor's scale (the BatchNorm constants may differ in the last bit: the
    statistics are summed in another order, and a row's head is a sum of terms that can cancel)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal((a > 0) & (a < 1), (b > 0) & (b < 1))
    assert float(np.abs(a - b).max()) <= 1e-6 * max(float(np.abs(b).max()), 1e-6)


def _step(m, hf, target, fused, seed):
    from deepgate import ops
    from deepgate.arch import mlp as mlp_mod
    old = mlp_mod.FUSED_READOUT
    mlp_mod.FUSED_READOUT = fused
    try:
        x = hf.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        prob = m(x, clamp01=True, seed=seed)
        ops.l1_loss(prob, target).backward()
    finally:
        mlp_mod.FUSED_READOUT = old
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads['dhf'] = x.grad.detach().clone()
    bufs = {k: v.detach().clone() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}
    return prob.detach().clone(), grads, bufs


def _inputs(N, dev):
    g = torch.Generator(device='cpu').manual_seed(N)
    hf = (torch.randn(N, 64, generator=g) * 0.7 + 0.1).to(dev)
    target = torch.rand(N, 1, generator=g).to(dev)
    return hf, target


@pytest.mark.parametrize('p_drop', [0.0, 0.2])
@pytest.mark.parametrize('N', [1, 63, 64, 4099, 1 << 20])
def test_fused_readout_matches_per_layer_path(N, p_drop):
    dev = _dev()
    hf, target = _inputs(N, dev)
    base = _mlp(p_drop, dev)
    m_ref, m_fus = copy.deepcopy(base), copy.deepcopy(base)
    prob_r, g_r, b_r = _step(m_ref, hf, target, False, 1234)
    prob_f, g_f, b_f = _step(m_fus, hf, target, True, 1234)
    # identical dropout masks and decisions: prob agrees up to summation order
    _close_prob(prob_f, prob_r)
    for k, ref in g_r.items():
        ref = ref.cpu().numpy()
        scale = max(float(np.abs(ref).max()), 1e-30)
        if k in ('fc.0.bias', 'fc.4.bias'):
            # a bias in front of a BatchNorm gets sum(dy) = 0 up to rounding: its gradient is rounding noise, which Adam turns into
            # lr-sized steps, so the fused passes form it bit for bit as the per-layer kernels do
            assert torch.equal(g_f[k], g_r[k]), (k, g_f[k][:4], g_r[k][:4])
            continue
        err = float(np.abs(g_f[k].cpu().numpy() - ref).max()) / scale
        # N = 1: BatchNorm of one row gives xhat = 0 and gradients that are pure cancellation (0 up to rounding)
        bound = 1e-5 if N > 1 else 1e-5 + 1e-6 / scale
        assert err <= bound, (k, err)
    for k, ref in b_r.items():
        if 'num_batches' in k:
            assert torch.equal(b_f[k], ref), k
            continue
        a, r = b_f[k].cpu().numpy(), ref.cpu().numpy()
        ulp = np.spacing(np.abs(r).astype(np.float32))
        assert np.all(np.abs(a - r) <= ulp), (k, float(np.abs(a - r).max()))


def test_fused_readout_repeat_is_bit_identical():
    dev = _dev()
    hf, target = _inputs(1 << 20, dev)
    base = _mlp(0.2, dev)
    m1, m2 = copy.deepcopy(base), copy.deepcopy(base)
    p1, g1, b1 = _step(m1, hf, target, True, 99)
    p2, g2, b2 = _step(m2, hf, target, True, 99)
    assert torch.equal(p1, p2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k


def test_fused_readout_consumes_rng_like_per_layer_path():
    dev = _dev()
    hf, target = _inputs(4099, dev)
    base = _mlp(0.2, dev)
    m_ref, m_fus = copy.deepcopy(base), copy.deepcopy(base)
    torch.manual_seed(7)
    prob_r, _, _ = _step(m_ref, hf, target, False, None)
    after_r = torch.rand(4)
    torch.manual_seed(7)
    prob_f, _, _ = _step(m_fus, hf, target, True, None)
    after_f = torch.rand(4)
    assert torch.equal(after_r, after_f)
    _close_prob(prob_f, prob_r)
