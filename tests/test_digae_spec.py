"""DiGAE baseline (--model AE) without a GPU: the float64 restatement tests/digae_ref.py pinned to the arrays recorded from the
reference's own modules (tests/golden/g9_digae.npz, make_golden_digae.py), the agg / rho factorisation of the layer, the
module surface (names, shapes, seeded values, strict checkpoint load) and train.py's wiring up to the first device call."""
import types

import numpy as np
import pytest
import torch

import digae_ref as R
from conftest import load_golden

CASES = {'a1b0': (1.0, 0.0, True), 'a05b05': (0.5, 0.5, True), 'a0b1': (0.0, 1.0, True), 'a1b0_nl': (1.0, 0.0, False),
         'float': (1.0, 0.0, True), 'single': (1.0, 0.0, True)}
SHAPES = {'float': (3, 32, 16), 'single': (6, 64)}


def fixture_case(z, p, dtype=torch.float64):
    ei = torch.from_numpy(z['edge_index'])
    neg = torch.from_numpy(z['neg_edge_index'])
    if p == 'float':
        x = torch.from_numpy(z['xf']).to(dtype)
    else:
        x = torch.nn.functional.one_hot(torch.from_numpy(z['cls']).long(), 6).to(dtype)
    params = {str(k): torch.from_numpy(z['%s_param_%s' % (p, k)]).to(dtype).requires_grad_(True) for k in z[p + '_keys']}
    return x, ei, neg, params


def run_ref(z, p, dtype=torch.float64):
    """The restatement on a fixture case -> dict of the arrays the fixture records."""
    x, ei, neg, params = fixture_case(z, p, dtype)
    x.requires_grad_(p == 'float')
    out = {}
    if p == 'single':
        s, t = R.single_layer_encoder(params, '', x, x, ei, *CASES[p])
    else:
        s, t, out['hs'], out['ht'] = R.encoder(params, '', x, x, ei, *CASES[p])
    loss, pred = R.recon_loss(s, t, ei, neg)
    loss.backward()
    out.update(s=s, t=t, loss=loss, pred_bin=pred)
    out.update({'grad_' + k: v.grad for k, v in params.items()})
    if p == 'float':
        out['dx'] = x.grad
    return out


def rel_err(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    a = a.detach().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    return float(np.abs(a - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.mark.parametrize('p', list(CASES))
def test_restatement_equals_every_fixture_array(p):
    """float64 restatement against the reference's float32 run: 2e-5 of each array's scale (float32 has 6e-8; sums of up to 71 terms
    and two layers stay two orders below the bound), predictions bit for bit."""
    z = load_golden('g9_digae')
    out = run_ref(z, p)
    recorded = [k[len(p) + 1:] for k in z.files if k.startswith(p + '_') and not k.startswith(p + '_nl_')
                and not k.startswith(p + '_param_') and k != p + '_keys']
    assert {'s', 't', 'loss', 'pred_bin'} <= set(recorded) and len([k for k in recorded if k.startswith('grad_')]) == len(z[p + '_keys'])
    for k in recorded:
        if k == 'pred_bin':
            assert np.array_equal(out[k].numpy(), z[p + '_pred_bin'])
        else:
            assert k in out, k
            assert rel_err(out[k], z['%s_%s' % (p, k)]) <= 2e-5, (p, k, rel_err(out[k], z['%s_%s' % (p, k)]))


@pytest.mark.parametrize('alpha,beta,loops', [(1.0, 0.0, True), (0.5, 0.5, True), (0.0, 1.0, True), (1.0, 0.0, False), (0.5, 1.0, False)])
def test_factorised_layer_equals_the_per_edge_form(alpha, beta, loops):
    """out_i = W agg_i + rho_i b with agg = r_i sum c_j x_j, rho = r_i sum c_j: the Linear commutes with the sum (float64, 1e-12)."""
    z = load_golden('g9_digae')
    ei = torch.from_numpy(z['edge_index'])
    g = torch.Generator().manual_seed(3)
    x = torch.randn(204, 16, dtype=torch.float64, generator=g)
    W, b = torch.randn(32, 16, dtype=torch.float64, generator=g), torch.randn(32, dtype=torch.float64, generator=g)
    for e in (ei, R.flip(ei)):
        a, f = R.conv(x, W, b, e, alpha, beta, loops), R.conv_factored(x, W, b, e, alpha, beta, loops)
        assert float((a - f).abs().max()) <= 1e-12 * float(a.abs().max())
        if not loops:                            # an empty list gives a zero row, not the bias
            empty = torch.ones(204, dtype=torch.bool)
            empty[e[1]] = False
            assert empty.any() and float(a[empty].abs().max()) == 0.0


def test_scales_are_exact_at_exponent_zero_and_zero_at_degree_zero():
    z = load_golden('g9_digae')
    ei = torch.from_numpy(z['edge_index'])
    r, c = R.scales(ei, 204, 0.0, 1.0, True)
    assert bool((r == 1).all()) and float(c.max()) == 1.0 and float(c.min()) < 1 / 65
    r, c = R.scales(ei, 204, 1.0, 0.0, False)
    indeg = torch.bincount(ei[1], minlength=204)
    assert bool((r[indeg == 0] == 0).all()) and bool(torch.isfinite(r).all()) and int(indeg.max()) >= 2
    assert int(torch.bincount(ei[0], minlength=204).max()) > 64      # the fixture's hub


def build(p):
    from deepgate import digae_layer as L
    torch.manual_seed(0)
    a, b, loops = CASES[p]
    if p == 'single':
        return L.SingleLayerDirectedGCNConvEncoder(*SHAPES[p], a, b, loops, False)
    return L.DirectedGCNConvEncoder(*SHAPES.get(p, (6, 64, 64)), a, b, loops, False)


@pytest.mark.parametrize('p', list(CASES))
def test_modules_line_up_with_the_reference_state_dict(p):
    """Same keys in the same order, same shapes, the same seeded values; the recorded state_dict loads strictly."""
    z = load_golden('g9_digae')
    enc = build(p)
    sd = enc.state_dict()
    assert list(sd.keys()) == [str(k) for k in z[p + '_keys']]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z['%s_param_%s' % (p, k)]), k
    enc.load_state_dict({str(k): torch.from_numpy(z['%s_param_%s' % (p, k)]) + 1 for k in z[p + '_keys']}, strict=True)
    conv = enc.source_conv.conv if p == 'single' else enc.source_conv.conv1
    assert (conv.alpha, conv.beta, conv.self_loops, conv.adaptive) == (*CASES[p], False)


def test_package_exports_the_directed_gae():
    import deepgate
    from deepgate import digae_layer as L
    m = deepgate.digae_model.DirectedGAE(build('a1b0'))
    assert isinstance(m.decoder, L.DirectedInnerProductDecoder) and all(hasattr(m, a) for a in ('encode', 'decode', 'recon_loss', 'test'))
    assert list(m.state_dict().keys()) == ['encoder.' + k for k in build('a1b0').state_dict().keys()]


def test_cpu_tensors_are_refused():
    from deepgate._hip import HipLibraryError
    z = load_golden('g9_digae')
    x, ei, _, _ = fixture_case(z, 'float', torch.float32)
    with pytest.raises(HipLibraryError):
        build('float')(x, x, ei)


def test_train_builds_the_baseline_encoder_for_model_ae(monkeypatch, tmp_path):
    """train.py --model AE up to the first device call: the encoder handed to Model and Trainer."""
    import deepgate
    import train
    from deepgate import digae_layer as L
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(args, model, **kw):
        seen.update(args=args, model=model, kw=kw)
        raise Stop

    monkeypatch.setattr(deepgate, 'Trainer', fake_trainer)
    argv = ['--exp_id', 'ae', '--type', 'aig', '--synthetic', '2', '--synthetic_nodes', '64', '--synthetic_levels', '4', '--save_dir', str(tmp_path)]
    with pytest.raises(Stop):
        train.main(argv + ['--model', 'AE', '--dim_hidden', '32'])
    enc = seen['model'].struct_encoder
    assert isinstance(enc, L.DirectedGCNConvEncoder) and isinstance(seen['model'], deepgate.dg_ae_model_aig.Model)
    c1, c2 = enc.source_conv.conv1, enc.target_conv.conv2
    assert (c1.lin.in_features, c1.lin.out_features, c2.lin.in_features, c2.lin.out_features) == (6, 32, 32, 32)
    assert (c1.alpha, c1.beta, c1.self_loops, c1.adaptive) == (1.0, 0.0, True, False)
    with pytest.raises(Stop):
        train.main(argv + ['--model', 'DG_AE'])
    assert isinstance(seen['model'].struct_encoder, L.DirectMultiGCNEncoder)
    with pytest.raises(SystemExit, match='DG_VAE'):
        train.main(argv + ['--model', 'DG_VAE'])


def test_no_colour_tables_for_an_encoder_without_half_rounds():
    from deepgate import digae_layer as L
    from deepgate.trainer import Trainer
    half = lambda enc: Trainer._encoder_half_rounds(types.SimpleNamespace(model=types.SimpleNamespace(ENCODER_ATTR='struct_encoder', struct_encoder=enc)))
    assert half(build('a1b0')) == []
    assert half(L.DirectMultiGCNEncoder(6, 16, s_rounds=1, t_rounds=3)) == [2, 6]
    assert half(None) == [8]
    plan = deepgate_plan()
    plan.warm(torch.zeros(plan.N, dtype=torch.uint8), [])
    assert getattr(plan, '_stage1', None) is None and getattr(plan, '_quotient', None) is None


def deepgate_plan():
    from deepgate.graph_plan import GraphPlan
    z = load_golden('g9_digae')
    return GraphPlan(torch.from_numpy(z['edge_index']), 204)
