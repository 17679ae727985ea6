"""The readout's dropout mask as a specification (csrc/mgv_dropout.h `mgv::drop_scale`), restated on the CPU by
`oracle.ref_cpu.drop_factors`: the vectorised restatement against a plain Python-integer one, the statistics a mask must have,
and the `drop=` / `taken=` hooks of the float64 readout that consume it.  No GPU here; tests/test_hip_readout_reference.py ties the
restatement to the device bit for bit.

Sigma multiples.  The masks are a fixed function of (seed, element), so nothing here is random from run to run; the bounds say what
a fair stream would satisfy.  Shares: 5 sigma of the binomial, because one (seed, p) case makes 1 + 32 + 64 comparisons and there are
9 cases, about 900 in all: a fair stream passes all of them at 5 sigma with probability 0.9995 (two-sided 5.7e-7 each), at 3 sigma
only with probability 0.09.  Correlations: 4 sigma of 1/sqrt(n), a handful of comparisons per case (two-sided 6.3e-5 each)."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

SEEDS = [0, 1, 1234, 1234 + 7919, 2 ** 62 - 5, 2 ** 62 - 1]


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
@pytest.mark.parametrize('seed', SEEDS)
def test_vectorised_mask_equals_the_scalar_restatement(seed, p):
    n_rows, C = 3001, 32
    f = R.drop_factors(seed, n_rows, C, p).numpy().reshape(-1)
    rng = np.random.Generator(np.random.PCG64(seed % 1000 + int(p * 10)))
    elems = sorted(set([0, 1, 31, 32, 33, n_rows * C - 1]) | set(int(e) for e in rng.integers(0, n_rows * C, size=300)))
    p32 = np.float32(p)
    ks = 1.0 / (1.0 - float(p32))
    for e in elems:
        h24 = R.drop_hash_scalar(seed, e)
        assert 0 <= h24 < (1 << 24)
        u = np.float32(h24) * np.float32(1.0 / 16777216.0)           # exact: 24 bits times a power of two
        want = 0.0 if u < p32 else ks
        assert f[e] == want, (seed, p, e, f[e], want)
    assert set(np.unique(f).tolist()) == {0.0, ks}


def test_element_number_is_row_times_width_plus_column():
    """The same stream cut into rows of another width: element (r, c) of width C is element r * C + c of the flat stream."""
    a = R.drop_factors(77, 64, 32, 0.2).reshape(-1)
    b = R.drop_factors(77, 128, 16, 0.2).reshape(-1)
    c = R.drop_factors(77, 2048, 1, 0.2).reshape(-1)
    assert torch.equal(a, b) and torch.equal(a, c)
    # a prefix of a longer mask: rows do not depend on how many follow
    assert torch.equal(R.drop_factors(77, 10, 32, 0.2), R.drop_factors(77, 64, 32, 0.2)[:10])


def test_no_dropout_gives_all_ones_and_p_is_compared_in_float32():
    assert torch.equal(R.drop_factors(5, 7, 8, 0.0), torch.ones(7, 8, dtype=torch.float64))
    assert torch.equal(R.drop_factors(5, 7, 8, -1.0), torch.ones(7, 8, dtype=torch.float64))
    # u takes the values k / 2^24; float32(0.2) = 3355443.25 / 2^24 lies between two of them, and so does the double 0.2, so the share of
    # dropped elements is the same, but the factor is formed from the float32 value the kernels receive
    f = R.drop_factors(5, 7, 8, 0.2)
    assert float(f.max()) == 1.0 / (1.0 - float(np.float32(0.2)))


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
@pytest.mark.parametrize('seed', [1234, 1234 + 7919, 2 ** 62 - 5])
def test_kept_share_overall_per_column_and_per_row_block(seed, p):
    n_rows, C, blocks = 1 << 16, 32, 64
    keep = (R.drop_factors(seed, n_rows, C, p) != 0).numpy()
    q = 1.0 - float(np.float32(p))

    def sigma(n):
        return np.sqrt(q * (1 - q) / n)

    assert abs(keep.mean() - q) <= 5 * sigma(keep.size), (keep.mean(), q)
    col = keep.mean(axis=0)
    assert np.abs(col - q).max() <= 5 * sigma(n_rows), np.abs(col - q).max()
    blk = keep.reshape(blocks, -1).mean(axis=1)
    assert np.abs(blk - q).max() <= 5 * sigma(keep.size // blocks), np.abs(blk - q).max()


def _corr(a, b):
    a = a.astype(np.float64) - a.mean()
    b = b.astype(np.float64) - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('seed', [1234, 2 ** 62 - 5])
def test_masks_of_the_two_layers_and_neighbouring_elements_are_uncorrelated(seed, p):
    n_rows, C = 1 << 16, 32                                   # n = 2^21 elements
    m1 = (R.drop_factors(seed, n_rows, C, p) != 0).numpy()
    m2 = (R.drop_factors(seed + 7919, n_rows, C, p) != 0).numpy()          # the second layer's seed of the same step (arch/mlp.py)
    bound = 4.0 / np.sqrt(m1.size)
    assert not np.array_equal(m1, m2)
    assert abs(_corr(m1.ravel(), m2.ravel())) <= bound
    f = m1.ravel()
    assert abs(_corr(f[:-1], f[1:])) <= 4.0 / np.sqrt(f.size - 1)          # next element (next column)
    assert abs(_corr(m1[:-1].ravel(), m1[1:].ravel())) <= 4.0 / np.sqrt(m1[1:].size)       # same column, next row
    # the next step's seed is another draw; neighbouring SEEDS must not give shifted copies of one stream either
    m3 = (R.drop_factors(seed + 1, n_rows, C, p) != 0).numpy()
    assert abs(_corr(m1.ravel(), m3.ravel())) <= bound
    assert abs(_corr(f[1:], m3.ravel()[:-1])) <= 4.0 / np.sqrt(f.size - 1)


# ---------------------------------------------------------------------------------------------- the float64 readout's hooks
def _params(dt):
    g = torch.Generator().manual_seed(11)
    name = 'readout_prob.fc'
    p = {}
    for lin, (o, i) in ((0, (32, 64)), (4, (32, 32)), (8, (1, 32))):
        p['%s.%d.weight' % (name, lin)] = (torch.randn(o, i, generator=g) / np.sqrt(i)).to(dt).requires_grad_(True)
        p['%s.%d.bias' % (name, lin)] = (0.1 * torch.randn(o, generator=g)).to(dt).requires_grad_(True)
    for bn in (1, 5):
        p['%s.%d.weight' % (name, bn)] = (0.5 + torch.rand(32, generator=g)).to(dt).requires_grad_(True)
        p['%s.%d.bias' % (name, bn)] = (0.3 * torch.randn(32, generator=g)).to(dt).requires_grad_(True)
        p['%s.%d.running_mean' % (name, bn)] = torch.zeros(32, dtype=dt)
        p['%s.%d.running_var' % (name, bn)] = torch.ones(32, dtype=dt)
    with torch.no_grad():
        p[name + '.8.bias'].fill_(0.4)
    return p


def _bn(p):
    return {k: v.clone() for k, v in p.items() if 'running_' in k}


def test_readout_hooks_absent_or_neutral_change_nothing():
    p = _params(torch.float64)
    hf = torch.randn(97, 64, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    b0, b1, b2 = _bn(p), _bn(p), _bn(p)
    plain = R.readout_prob(p, hf, True, b0, p_drop=0.0)
    taken = {}
    ones = [torch.ones(97, 32, dtype=torch.float64)] * 2
    hooked = R.readout_prob(p, hf, True, b1, p_drop=0.0, drop=ones, taken=taken)
    assert torch.equal(plain, hooked)
    for k in b0:
        assert torch.equal(b0[k], b1[k])
    assert len(taken['relu']) == 2 and taken['relu'][0].shape == (97, 32) and taken['relu'][0].dtype == torch.bool
    assert torch.equal(torch.clamp(taken['pre_clamp'], 0.0, 1.0), plain.detach())
    # imposing a run's own decisions reproduces it, and `taken` still reports what the run would have decided by itself
    dec = {'relu': taken['relu'], 'inside': (taken['pre_clamp'] > 0) & (taken['pre_clamp'] < 1)}
    taken2 = {}
    again = R.readout_prob(p, hf, True, b2, p_drop=0.0, decisions=dec, drop=ones, taken=taken2)
    assert torch.equal(again, plain)
    assert all(torch.equal(a, b) for a, b in zip(taken['relu'], taken2['relu']))
    # eval mode ignores the factors, as it ignores dropout
    zeros = [torch.zeros(97, 32, dtype=torch.float64)] * 2
    assert torch.equal(R.readout_prob(p, hf, False, _bn(p), drop=zeros), R.readout_prob(p, hf, False, _bn(p)))


def test_readout_with_factors_is_inverted_dropout_with_that_mask():
    """drop=[f1, f2] multiplies each block's ReLU output by its factors: checked against the formula written out, and the gradient
    of the second Linear's weight column of a unit that layer 1 dropped in every row is zero."""
    p = _params(torch.float64)
    N = 50
    hf = torch.randn(N, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    f1, f2 = R.drop_factors(9, N, 32, 0.2), R.drop_factors(9 + 7919, N, 32, 0.5)
    f1[:, 7] = 0.0
    prob = R.readout_prob(p, hf, True, _bn(p), drop=[f1, f2])
    name = 'readout_prob.fc'

    def bn(v, k):
        m, var = v.mean(0), v.var(0, unbiased=False)
        return (v - m) / torch.sqrt(var + 1e-5) * p['%s.%d.weight' % (name, k)] + p['%s.%d.bias' % (name, k)]

    a1 = torch.relu(bn(R.linear(p, name + '.0', hf), 1)) * f1
    a2 = torch.relu(bn(R.linear(p, name + '.4', a1), 5)) * f2
    want = torch.clamp(R.linear(p, name + '.8', a2), 0.0, 1.0)
    assert float((prob - want).detach().abs().max()) <= 1e-12
    (prob * torch.randn(N, 1, generator=torch.Generator().manual_seed(4), dtype=torch.float64)).sum().backward()
    gW2 = p[name + '.4.weight'].grad
    assert float(gW2.abs().max()) > 0 and float(gW2[:, 7].abs().max()) == 0.0
    assert float(p[name + '.1.weight'].grad[7]) == 0.0 and float(p[name + '.1.bias'].grad[7]) == 0.0
