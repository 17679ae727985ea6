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
    assert 'first_stage' not in plan.cache and 'quotient' not in plan.cache and 'tagged' not in plan.cache
    plan.warm(torch.zeros(plan.N, dtype=torch.uint8), 0)     # (the same call with half rounds to expect does build the first-stage table)
    assert 'first_stage' in plan.cache


def deepgate_plan():
    from deepgate.graph_plan import GraphPlan
    z = load_golden('g9_digae')
    return GraphPlan(torch.from_numpy(z['edge_index']), 204)


# ------------------------------------------------------------------------------------------------
# the per-entry references of csrc/digcn_conv.hip (digae_ref.reference and its builders), pinned without a GPU: a float32 evaluation
# in another order stays inside every bound, every planted mistake is at least 8 times outside one, the builders plant what they say,
# and the five entries refuse what include/mgvae_hip.h says they refuse.  tests/test_hip_digae_entries.py holds the device to the same
# bounds.
# ------------------------------------------------------------------------------------------------
import ctypes  # noqa: E402
import functools  # noqa: E402

WIDTHS = (16, 32, 64, 128)
FACTOR = 8.0
SECOND_PASS_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 66, 300)       # on the first rows of a second grid pass (the pass has 11 rows)


def cpu_scales(ei, n, alpha, beta, loops, reverse):
    """The graph's own scales rounded to float32: what the device's mgv_digcn_scales output stands for on the CPU."""
    r, c = R.scales(R.flip(ei) if reverse else ei, n, alpha, beta, loops)
    return r.float(), c.float()


def gather_cases(H, ei, n, rc_of, special=None):
    """Both CSRs x (independent scales, self loops on / off; the graph's scales at the five settings) x (mask, none); ReLU alternating."""
    k = 0
    for reverse in (False, True):
        for form, (alpha, beta, loops) in [('random', (None, None, True)), ('random', (None, None, False))] + [('scales', s) for s in R.SETTINGS]:
            for masked in (True, False):
                rc = None if form == 'random' else rc_of(alpha, beta, loops, reverse)
                k += 1
                tag = 'H=%d n=%d rev=%d %s a=%s b=%s loops=%d mask=%d relu=%d' % (H, n, reverse, form, alpha, beta, loops, masked, k % 2)
                yield tag, R.gather_case(H, ei, n, reverse, loops, bool(k % 2), masked, form, k, rc, special)


def class_cases(H, ei, n, rc_of, special=None, dz_rows=None, Cs=(1, 6, 8)):
    """Both CSRs x C x (z, none), the scales rotating through independent ones and the five settings; ReLU alternating."""
    k = 0
    for reverse in (False, True):
        for C in Cs:
            for masked in (True, False):
                form = [None] + R.SETTINGS
                s = form[k % len(form)]
                k += 1
                loops = bool(k % 2) if s is None else s[2]
                rc = None if s is None else rc_of(s[0], s[1], loops, reverse)
                tag = 'H=%d n=%d rev=%d C=%d %s loops=%d z=%d relu=%d' % (H, n, reverse, C, s, loops, masked, k % 2)
                yield tag, R.class_case(H, ei, n, reverse, loops, bool(k % 2), masked, C, k, rc, special, dz_rows)


def second_pass(entry):
    """(H, n, edge_index, special rows, dz rows) of the smallest case in which `entry` makes a second grid pass: H = 128, 11 rows past the
    first pass, planted lengths on the first ten of them (in both CSRs) and on the last row; for class_bwd about 200 live dz rows."""
    H = 128
    first = R.pass_rows(H, entry)
    n = first + 11
    ei = R.designed_lists(H, n, first, first, SECOND_PASS_LENGTHS)
    special = R.special_rows(H, n, first, first, SECOND_PASS_LENGTHS)
    dz_rows = list(range(90)) + list(range(first - 100, n))
    return H, n, ei, special, dz_rows


@functools.lru_cache(maxsize=None)
def designed(H):
    return R.designed_lists(H)


def _inside(entry, cases, routes=(True,)):
    worst = 0.0
    for tag, a in cases:
        r = R.reference(entry, a)
        for heavy in routes:
            w = R.share(R.restate32(entry, a, heavy), r)
            worst = max(worst, w)
            assert w <= 1.0, (entry, tag, heavy, w)
    return worst


def _outside(entry, cases, seen):
    """Every defect that concerns `entry` and that the case can show: at least FACTOR times outside its bound on some entry."""
    for tag, a in cases:
        r = R.reference(entry, a)
        for name, f in R.defects().items():
            if entry in f.entries and f.applies(entry, a):
                w = R.share(f(entry, a)['ref'], r)
                seen[name] = min(seen.get(name, float('inf')), w)
                assert w >= FACTOR, (entry, tag, name, w)


@pytest.mark.parametrize('H', WIDTHS)
def test_float32_in_another_order_stays_inside_every_bound(H):
    ei, n = designed(H), 400
    rc_of = lambda *s: cpu_scales(ei, n, *s)
    wg = _inside('gather', gather_cases(H, ei, n, rc_of), (True, False))
    wf = _inside('class_fwd', class_cases(H, ei, n, rc_of))
    wb = _inside('class_bwd', class_cases(H, ei, n, rc_of))
    print('DG float32 H=%d | worst share of the bound: gather %.3g  class_fwd %.3g  class_bwd %.3g' % (H, wg, wf, wb))


@pytest.mark.parametrize('H', WIDTHS)
def test_every_defective_restatement_is_far_outside_its_bound(H):
    ei, n = designed(H), 400
    rc_of = lambda *s: cpu_scales(ei, n, *s)
    seen = {}
    _outside('gather', gather_cases(H, ei, n, rc_of), seen)
    _outside('class_fwd', class_cases(H, ei, n, rc_of), seen)
    _outside('class_bwd', class_cases(H, ei, n, rc_of), seen)
    assert set(seen) == set(R.defects()) - {'the rows of a second grid pass skipped'}
    print('DG defects H=%d | smallest distance from the bound: %s' % (H, '; '.join('%s %.3g' % kv for kv in seen.items())))


@pytest.mark.parametrize('entry', ['gather', 'class_fwd', 'class_bwd'])
def test_second_grid_pass_case(entry):
    H, n, ei, special, dz_rows = second_pass(entry)
    assert R.pass_rows(H, entry) == {'gather': 32768, 'class_fwd': 32768, 'class_bwd': 8192}[entry] and n % 64 != 0
    a, b = R.planted(H, n, n - 11, n - 11, SECOND_PASS_LENGTHS)
    for rev, want in ((False, a), (True, b)):
        ptr = R.csr_of(ei, n, rev)[0]
        assert all(int(ptr[v + 1] - ptr[v]) == l for v, l in want.items()) and min(want) == R.pass_rows(H, entry) and max(want) == n - 1
    rc_of = lambda *s: cpu_scales(ei, n, *s)
    if entry == 'gather':
        cases = [c for c in gather_cases(H, ei, n, rc_of, special)][:2]
    else:
        cases = [c for c in class_cases(H, ei, n, rc_of, special, dz_rows, Cs=(8,))]
    if entry == 'class_bwd':
        live = cases[0][1]['dz'].abs().sum(1) > 0
        assert int(live.sum()) == 201 and bool(live[n - 1]) and bool(live[8191]) and bool(live[8192])
    seen = {}
    w = _inside(entry, cases, (True, False) if entry == 'gather' else (True,))
    _outside(entry, cases, seen)
    assert seen['the rows of a second grid pass skipped'] >= FACTOR
    print('DG second pass %s n=%d | float32 worst share %.3g | %s' % (entry, n, w, '; '.join('%s %.3g' % kv for kv in seen.items())))


def test_many_heavy_nodes_case():
    n, H = 4100, 16
    ei = R.many_heavy_lists(n)
    ptr = R.csr_of(ei, n, False)[0]
    lens = ptr[1:] - ptr[:-1]
    assert int(lens.min()) == 65 and int(lens.max()) == 70 and int((lens > R.HEAVY).sum()) == n > 4096 and 270000 < ei.shape[1] < 280000
    a = R.gather_case(H, ei, n, False, True, False, True, 'random', 3, special=range(n))
    r = R.reference('gather', a)
    w = max(R.share(R.restate32('gather', a, heavy), r) for heavy in (True, False))
    assert w <= 1.0, w
    for name in ('heavy: the partial of lane group 0 dropped', 'heavy: the self term added once per group', 'a list of 65 left unwritten'):
        assert R.share(R.defects()[name]('gather', a)['ref'], r) >= FACTOR, name
    print('DG many heavy H=%d | float32 worst share %.3g' % (H, w))


@pytest.mark.parametrize('H', WIDTHS)
def test_designed_builders_plant_what_they_say(H):
    ei, n, G = designed(H), 400, 256 // (H // 4)
    L = R.planted_lengths(H)
    assert L == [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 66, 64 + G - 1, 64 + G, 64 + G + 1, 64 + 2 * G + 1, 129, 200, 300] and n % 64 != 0
    a, b = R.planted(H)
    assert sorted(a.values()) == sorted(L + [7]) and sorted(b.values()) == sorted(L + [65]) and n - 1 in a and n - 1 in b
    assert set(a) & set(b) == {n - 1}
    plan = deepgate_designed_plan(H)
    for rev, want in ((False, a), (True, b)):
        ptr, idx = R.csr_of(ei, n, rev)
        pp, pi = plan.csr(rev)
        assert torch.equal(ptr, pp.long()) and torch.equal(idx, pi.long())               # the lists the device plan will hold
        lens = ptr[1:] - ptr[:-1]
        assert all(int(lens[v]) == l for v, l in want.items())
        rest = torch.ones(n, dtype=torch.bool)
        rest[list(want)] = False
        assert int(lens[rest].max()) <= (3 if not rev else R.HEAVY) and int(lens[rest].min()) == 0
        heavy = set(torch.nonzero(lens > 64).reshape(-1).tolist())
        assert heavy == {v for v, l in want.items() if l > 64} == set(plan.heavy(rev)[1].tolist()) and len(heavy) >= 8
    assert bool((ei[0] == ei[1]).any()) and ei.shape[1] > len(set(map(tuple, ei.t().tolist())))      # self edges and duplicates occur
    rng = np.random.default_rng(H)
    for C in (1, 6, 8):
        ids = set(R.designed_classes(rng, n, C).tolist())
        assert ids == set(range(C)) - ({C - 2} if 2 <= C < 8 else set()) and C - 1 in ids
    m = R.designed_mask(rng, n, H, R.special_rows(H)).numpy()
    assert m.dtype == np.float32 and 0 < R.SUBNORMAL < np.finfo(np.float32).tiny and np.float32(R.SUBNORMAL) == R.SUBNORMAL
    for k in range(H):
        col = m[:, k]
        assert (col < 0).any() and (col >= np.finfo(np.float32).tiny).any() and int((col == np.float32(R.SUBNORMAL)).sum()) == 1
        assert ((col == 0) & ~np.signbit(col)).any() and ((col == 0) & np.signbit(col)).any()
    y, o = R.signed(rng, n, H), R.positive(rng, n)
    assert y.dtype == torch.float32 and 0.5 <= float(y.abs().min()) and float(y.abs().max()) <= 2 and bool((y < 0).any()) and bool((y > 0).any())
    assert o.dtype == torch.float32 and 0.25 <= float(o.min()) and float(o.max()) <= 4


def deepgate_designed_plan(H):
    from deepgate.graph_plan import GraphPlan
    return GraphPlan(designed(H), 400)


def test_reference_equals_propagate_and_autograd():
    """digae_ref.reference against the restatement the fixture pins (propagate, on the same float32 scales widened), forward, pull and dT."""
    H, n = 32, 400
    ei = designed(H)
    for alpha, beta, loops in R.SETTINGS:
        for reverse in (False, True):
            e = R.flip(ei) if reverse else ei
            rc = cpu_scales(ei, n, alpha, beta, loops, reverse)
            a = R.gather_case(H, ei, n, reverse, loops, False, False, 'scales', 1, rc)
            r = R.reference('gather', a)
            ref = R.propagate(a['y'].double(), e, alpha, beta, loops, rc=rc)
            assert float((r['ref'] - ref).abs().max()) <= 1e-13 * float(r['S'].max())
            b = R.class_case(H, ei, n, reverse, loops, False, True, 6, 2, rc)
            T = b['T'].double().requires_grad_(True)
            pre = R.propagate(T[b['cls'].long()], e, alpha, beta, loops, rc=rc)
            rf = R.reference('class_fwd', b)
            assert float((rf['ref'] - pre.detach()).abs().max()) <= 1e-13 * float(rf['S'].max())
            (pre * (b['z'].double() > 0) * b['dz'].double()).sum().backward()
            rb = R.reference('class_bwd', b)
            assert float((rb['ref'] - b['a0'].double() - T.grad).abs().max()) <= 1e-13 * float(rb['S'].max())
            assert bool((rb['S'][4] == 0).all()) and torch.equal(rb['ref'][4].float(), b['a0'][4])          # class C - 2 = 4 is absent


def test_heavy_row_is_the_64_of_the_header():
    from deepgate.graph_plan import GraphPlan
    from deepgate import _hip
    assert GraphPlan.HEAVY_ROW == 64 == R.HEAVY
    with open(_hip.HEADER_PATH) as f:
        assert 'heavy_nodes[heavy_n]: every node whose list is longer than 64 (GraphPlan.heavy)' in f.read()


EINVAL = -1


def _digcn(name, **over):
    """One call with dummy non-NULL pointers (never read on the host) and 1 for every scalar but those in `over`; a pointer named in
    `over` is None (NULL) or the name of the argument whose address it shares.  Every case returns before anything is launched."""
    import test_width_refusals_spec as WR
    from deepgate import _hip
    lib, sigs, names = _hip.load(), _hip.parse_header()[name], WR._arg_names()[name]
    addr = {nm: 64 * (k + 1) for k, nm in enumerate(names)}
    args = []
    for nm, t in zip(names, sigs):
        if t is ctypes.c_void_p:
            v = over.get(nm, nm)
            args.append(None if v is None else ctypes.c_void_p(addr[v]))
        else:
            args.append(over.get(nm, 64 if nm == 'H' else 1))
    args[-1] = None
    return getattr(lib, name)(*args)


def test_the_five_entries_refuse_what_the_header_says():
    from deepgate import _hip
    for name in ('mgv_digcn_scales', 'mgv_digcn_gather', 'mgv_digcn_class_fwd', 'mgv_digcn_class_bwd'):
        assert _digcn(name, N=0) == 0, name                          # an empty problem, every other argument as in the cases below
        assert _digcn(name, N=-1) == EINVAL, name
    for bad in (dict(alpha=-1.0), dict(beta=-0.5), dict(r=None), dict(list_ptr=None)):
        assert _digcn('mgv_digcn_scales', N=0, **bad) == EINVAL, bad
    for bad in (dict(out='y'), dict(heavy_n=1, heavy_nodes=None), dict(heavy_n=-1), dict(y=None), dict(outer=None)):
        assert _digcn('mgv_digcn_gather', N=0, **bad) == EINVAL, bad
    assert _digcn('mgv_digcn_gather', N=0, heavy_n=0, heavy_nodes=None, mask=None) == 0
    assert _digcn('mgv_digcn_gather', N=1, nbr_idx=None) == EINVAL
    for name in ('mgv_digcn_class_fwd', 'mgv_digcn_class_bwd'):
        for C in (0, 9, -1):
            assert _digcn(name, N=0, C=C) == EINVAL, (name, C)
        assert _digcn(name, N=0, C=8) == 0 and _digcn(name, N=1, nbr_idx=None) == EINVAL
    assert _digcn('mgv_digcn_class_bwd', N=0, z=None) == 0
    for H, N in ((16, 1), (64, 400), (128, 8203), (128, 5)):
        need = _hip.call_value('mgv_digcn_class_bwd_ws_floats', H, N)
        rows = 256 // (H // 4)
        assert need == min(-(-N // rows), 1024) * 8 * H
        assert _digcn('mgv_digcn_class_bwd', H=H, N=N, workspace_floats=need - 1) == EINVAL
        assert _digcn('mgv_digcn_class_bwd', H=H, N=N, workspace_floats=need, workspace=None) == EINVAL
    assert _hip.call_value('mgv_digcn_class_bwd_ws_floats', 64, 0) == 0 and _hip.call_value('mgv_digcn_class_bwd_ws_floats', 64, -3) == 0
