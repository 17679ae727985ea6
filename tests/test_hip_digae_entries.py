"""The entries of csrc/digcn_conv.hip (the --model AE baseline layer) one output entry at a time through the C ABI, against the float64
references of tests/digae_ref.py (`reference`: pinned on the CPU by tests/test_digae_spec.py, which also asserts the properties of
the builders used here and shows that the mistakes these tests are there to catch are at least 8 times outside the bounds):

  mgv_digcn_gather      |out - ref| <= (terms + 4) u S        S = |outer_i| sum |inner_j| [mask_jk > 0] |y_jk|
  mgv_digcn_class_fwd   |out - ref| <= (terms + 12) u S       S = |outer_i| sum |inner_j| |T[cls_j, k]|
  mgv_digcn_class_bwd   |dT - ref|  <= (nz + Lmax + 8) u S + 2 u |a0|     S[c,k] = sum_i w_i[c] |outer_i| [z_ik > 0] |dz_ik|

u = 2^-24, terms = list length (+ 1 with self loops), nz = nodes with a nonzero term, Lmax = the longest list, a0 = dT before the
call.  Every bound is a function of the reference's data (float32 rounding, digae_ref.reference's docstring); nothing is taken from
what the device returns.  An entry with S = 0 must be exactly 0 (a0 bit for bit for dT).  The mask decisions are float64 > 0 on the
float32 values, a positive subnormal included: a wrong decision loses or adds a whole term.

The lists are designed (digae_ref.designed_lists: 0 .. 8 entries, 63 .. 66, 64 + G - 1 .. 64 + 2G + 1 for the G lane groups of the
one-workgroup-per-list kernel, 129, 200, 300, in both CSRs and on the last node), plus 4,100 nodes of 65 to 70 entries (more heavy
nodes than heavy workgroups) and the smallest sizes at which the H = 128 kernels make a second grid pass.  Scales: independent random
ones, and the device's own mgv_digcn_scales output read back (the reference uses the float32 values widened, so the sum's error and the
scales' error are separate questions; test_hip_digae.py::test_scales_entry keeps the second).  Every output has 64 guard rows behind
it (NaN before the call, bit-identical after), workspaces are NaN-filled with a guard of their own, every call is made twice and must
give the same bits, and dT starts from random a0 of its entry's own magnitude.  Nothing here reads the reference checkout.

Every check prints one line `DG <entry> <case> | worst error / bound ...`; the table per entry and width is in NOTEBOOK.md."""
import numpy as np
import pytest
import torch

import digae_ref as R
from test_digae_spec import WIDTHS, class_cases, designed, gather_cases, second_pass

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


class Out:
    """[n][w] float32 with GUARD rows behind it: NaN everywhere before the call, or `fill` in the n rows."""

    def __init__(self, n, w, dev, fill=None):
        self.n = n
        self.parent = torch.full((n + GUARD, w), NAN, dtype=F32, device=dev)
        self.v = self.parent[:n]
        if fill is not None:
            self.v.copy_(fill)

    def intact(self):
        return bool((self.parent[self.n:].view(I32) == NANBITS).all())


def _bits(t):
    return t.detach().contiguous().view(I32).cpu()


def _plan(ei, n, dev):
    from deepgate.graph_plan import GraphPlan
    plan = GraphPlan(ei.to(dev), n)
    plan._check_status()
    return plan


def _own_lists(a, plan, reverse):
    """The case on the device plan's own arrays (read back): the same list lengths as the builder's, whatever the order inside a list."""
    p, i = plan.csr(reverse)
    assert torch.equal(p.long().cpu(), a['ptr'])
    return dict(a, ptr=p.long().cpu(), idx=i.long().cpu())


def _scales_of(plan):
    from deepgate import _hip

    def rc_of(alpha, beta, loops, reverse):
        r = torch.full((plan.N,), NAN, device=plan.in_ptr.device)
        c = torch.full((plan.N,), NAN, device=plan.in_ptr.device)
        _hip.call('mgv_digcn_scales', plan.N, _hip.ptr(plan.csr(reverse)[0]), _hip.ptr(plan.csr(not reverse)[0]), alpha, beta, int(loops),
                  _hip.ptr(r), _hip.ptr(c))
        return r, c
    return rc_of


def _twice(run):
    got, again = run(), run()
    assert torch.equal(_bits(got), _bits(again)), 'a repeated call gives other bits'
    return got.cpu()


def run_gather(a, plan, reverse, heavy, dev):
    from deepgate import _hip
    p, i = plan.csr(reverse)
    n, H = a['y'].shape
    hn, hnodes = plan.heavy(reverse) if heavy else (0, None)
    y, outer, inner = a['y'].to(dev), a['outer'].to(dev), a['inner'].to(dev)
    mask = None if a['mask'] is None else a['mask'].to(dev)

    def run():
        out = Out(n, H, dev)
        _hip.call('mgv_digcn_gather', H, n, _hip.ptr(y), _hip.ptr(p), _hip.ptr(i), _hip.ptr(outer), _hip.ptr(inner), _hip.ptr(mask), int(a['loops']),
                  int(a['relu']), hn, _hip.ptr(hnodes) if hn else None, _hip.ptr(out.parent))
        assert out.intact(), 'guard rows behind out'
        return out.v
    return _twice(run)


def run_class_fwd(a, plan, reverse, dev):
    from deepgate import _hip
    p, i = plan.csr(reverse)
    n, H = a['ptr'].shape[0] - 1, a['H']
    cls, T, outer, inner = a['cls'].to(dev), a['T'].to(dev), a['outer'].to(dev), a['inner'].to(dev)

    def run():
        out = Out(n, H, dev)
        _hip.call('mgv_digcn_class_fwd', H, n, _hip.ptr(cls), _hip.ptr(T), a['C'], _hip.ptr(p), _hip.ptr(i), _hip.ptr(outer), _hip.ptr(inner),
                  int(a['loops']), int(a['relu']), _hip.ptr(out.parent))
        assert out.intact(), 'guard rows behind out'
        return out.v
    return _twice(run)


def run_class_bwd(a, plan, reverse, dev):
    from deepgate import _hip
    p, i = plan.csr(reverse)
    n, H, C = a['ptr'].shape[0] - 1, a['H'], a['C']
    cls, outer, inner, dz = a['cls'].to(dev), a['outer'].to(dev), a['inner'].to(dev), a['dz'].to(dev)
    z = None if a['z'] is None else a['z'].to(dev)
    need = _hip.call_value('mgv_digcn_class_bwd_ws_floats', H, n)

    def run():
        dT = Out(C, H, dev, fill=a['a0'])
        ws = torch.full((need + GUARD,), NAN, dtype=F32, device=dev)
        _hip.call('mgv_digcn_class_bwd', H, n, _hip.ptr(cls), C, _hip.ptr(p), _hip.ptr(i), _hip.ptr(outer), _hip.ptr(inner), int(a['loops']),
                  _hip.ptr(z), _hip.ptr(dz), _hip.ptr(dT.parent), _hip.ptr(ws), need)
        assert dT.intact(), 'guard rows behind dT'
        assert bool((ws[need:].view(I32) == NANBITS).all()), 'guard behind the workspace'
        return dT.v
    return _twice(run)


def _held(entry, tag, got, r, a0=None):
    """The worst error / bound of one output; an entry nothing reaches keeps a0 bit for bit."""
    w = R.share(got, r)
    assert w <= 1.0, '%s %s: %.3g of its bound' % (entry, tag, w)
    if a0 is not None:
        dead = r['S'] == 0
        assert torch.equal(_bits(got)[dead], _bits(a0)[dead]), '%s %s: an entry no term reaches moved' % (entry, tag)
    return w


def _gather_checks(tag, a, plan, reverse, dev, relus=(False, True)):
    a = _own_lists(a, plan, reverse)
    worst = {}
    for relu in relus:
        ar = dict(a, relu=relu)
        r = R.reference('gather', ar)
        for heavy in (True, False):
            w = _held('gather', tag, run_gather(ar, plan, reverse, heavy, dev), r)
            worst[heavy] = max(worst.get(heavy, 0.0), w)
    print('DG gather %s | worst error / bound: heavy lists by workgroup %.3g, every list by its lane group %.3g' % (tag, worst[True], worst[False]))
    return max(worst.values())


def _class_checks(tag, a, plan, reverse, dev):
    a = _own_lists(a, plan, reverse)
    wf = 0.0
    for relu in (False, True):
        ar = dict(a, relu=relu)
        wf = max(wf, _held('class_fwd', tag, run_class_fwd(ar, plan, reverse, dev), R.reference('class_fwd', ar)))
    rb = R.reference('class_bwd', a)
    wb = _held('class_bwd', tag, run_class_bwd(a, plan, reverse, dev), rb, a['a0'])
    print('DG class %s | worst error / bound: class_fwd %.3g  class_bwd %.3g (%d entries no term reaches kept a0)' % (tag, wf, wb, int((rb['S'] == 0).sum())))
    return wf, wb


# ------------------------------------------------------------------------------------------------ the designed lists, every width
@pytest.mark.parametrize('H', WIDTHS)
def test_gather_on_the_designed_lists(H):
    """Both CSRs, self loops on and off, ReLU on and off, mask NULL and the designed mask (with its subnormal), heavy lists by workgroup
    and by lane group (both inside the bound; they need not agree bitwise), independent scales and the device's own at five settings."""
    dev = _dev()
    ei, n = designed(H), 400
    plan = _plan(ei, n, dev)
    assert plan.heavy(False)[0] >= 8 and plan.heavy(True)[0] >= 8
    worst = max(_gather_checks(tag, a, plan, 'rev=1' in tag, dev) for tag, a in gather_cases(H, ei, n, _scales_of(plan)))
    print('DG gather H=%d designed lists | worst error / bound %.3g' % (H, worst))


@pytest.mark.parametrize('H', WIDTHS)
def test_class_entries_on_the_designed_lists(H):
    """C in {1, 6, 8} (class C - 2 absent at C = 6: its dT row keeps a0), z NULL and the designed mask, dT from random a0 with guard
    rows behind its C rows, both CSRs, independent scales and the device's own."""
    dev = _dev()
    ei, n = designed(H), 400
    plan = _plan(ei, n, dev)
    ws = [_class_checks(tag, a, plan, 'rev=1' in tag, dev) for tag, a in class_cases(H, ei, n, _scales_of(plan))]
    print('DG class H=%d designed lists | worst error / bound: class_fwd %.3g  class_bwd %.3g' % (H, max(w[0] for w in ws), max(w[1] for w in ws)))


# ------------------------------------------------------------------------------------------------ more heavy nodes than heavy workgroups
@pytest.mark.parametrize('H', [16, 128])
def test_gather_with_more_heavy_nodes_than_workgroups(H):
    """4,100 lists of 65 to 70 entries: the workgroups of the one-workgroup-per-list kernel (4,096) take a second node."""
    dev = _dev()
    n = 4100
    ei = R.many_heavy_lists(n)
    plan = _plan(ei, n, dev)
    assert plan.heavy(False)[0] == n > 4096
    for masked in (True, False):
        a = R.gather_case(H, ei, n, False, True, False, masked, 'random', 3, special=range(n))
        _gather_checks('H=%d n=%d many heavy mask=%d' % (H, n, masked), a, plan, False, dev, relus=(False,))


# ------------------------------------------------------------------------------------------------ a second grid pass, at its smallest
def test_gather_second_grid_pass():
    """H = 128, 32,768 + 11 rows: planted lengths on the first rows of the second pass and on the last row, in both CSRs."""
    dev = _dev()
    H, n, ei, special, _ = second_pass('gather')
    plan = _plan(ei, n, dev)
    cases = list(gather_cases(H, ei, n, _scales_of(plan), special))
    picked = [c for c in cases if ('rev=0 random' in c[0] and 'loops=1' in c[0]) or 'rev=1 scales a=0.5' in c[0]]
    assert len(picked) == 4                                      # in-CSR with independent scales, out-CSR with the device's; mask and none
    for tag, a in picked:
        _gather_checks(tag, a, plan, 'rev=1' in tag, dev, relus=(a['relu'],))


@pytest.mark.parametrize('entry', ['class_fwd', 'class_bwd'])
def test_class_entries_second_grid_pass(entry):
    """H = 128: class_fwd at 32,768 + 11 rows, class_bwd at 8,192 + 11 with dz live on 201 rows around the boundary and at both ends
    (nz stays small: one lost node is far outside the bound)."""
    dev = _dev()
    H, n, ei, special, dz_rows = second_pass(entry)
    plan = _plan(ei, n, dev)
    for tag, a in class_cases(H, ei, n, _scales_of(plan), special, dz_rows, Cs=(8,)):
        reverse = 'rev=1' in tag
        a = _own_lists(a, plan, reverse)
        if entry == 'class_fwd':
            w = _held(entry, tag, run_class_fwd(a, plan, reverse, dev), R.reference(entry, a))
        else:
            w = _held(entry, tag, run_class_bwd(a, plan, reverse, dev), R.reference(entry, a), a['a0'])
        print('DG %s %s second pass | worst error / bound %.3g' % (entry, tag, w))


# ------------------------------------------------------------------------------------------------ through ops
@pytest.mark.parametrize('H', WIDTHS)
def test_through_ops_forward_and_backward(H):
    """ops.DiGCNGatherFn and ops.DiGCNClassFn on the designed lists, both `reverse` values, the five settings: forward against float64
    digae_ref.propagate (on the device's float32 scales widened) and backward against its float64 autograd on the device's own ReLU
    mask, with the per-entry bounds — the gather's backward is the pull over the OPPOSITE CSR with r and c exchanged and z as mask,
    so a wrong CSR or unswapped scales in ops.py are far outside."""
    dev = _dev()
    from deepgate import ops
    ei, n = designed(H), 400
    plan = _plan(ei, n, dev)
    k = 0
    for alpha, beta, loops in R.SETTINGS:
        for reverse in (False, True):
            k += 1
            relu, C = bool(k % 2) or k == 4, (1, 6, 8)[k % 3]
            rng = np.random.default_rng([H, k])
            e = R.flip(ei) if reverse else ei
            r, c = ops.digcn_scales(plan, reverse, alpha, beta, loops)
            rc = (r.cpu(), c.cpu())
            own, opp = R.csr_of(ei, n, reverse), R.csr_of(ei, n, not reverse)
            tag = 'H=%d rev=%d a=%s b=%s loops=%d relu=%d' % (H, reverse, alpha, beta, loops, relu)
            y, gz = R.signed(rng, n, H), R.signed(rng, n, H)
            # ---- DiGCNGatherFn
            yd = y.to(dev).requires_grad_(True)
            z = ops.DiGCNGatherFn.apply(yd, plan, reverse, alpha, beta, loops, relu)
            z.backward(gz.to(dev))
            zc = z.detach().cpu()
            y64 = y.double().requires_grad_(True)
            pre = R.propagate(y64, e, alpha, beta, loops, rc=rc)
            fw = dict(H=H, ptr=own[0], idx=own[1], y=y, outer=rc[0], inner=rc[1], mask=None, loops=loops, relu=relu)
            rf = R.reference('gather', fw)
            assert float((rf['ref'] - (pre.detach().clamp_min(0) if relu else pre.detach())).abs().max()) <= 1e-13 * float(rf['S'].max())
            w_z = _held('DiGCNGatherFn z', tag, zc, rf)
            m = (zc > 0).double() if relu else torch.ones_like(pre)
            (pre * m * gz.double()).sum().backward()
            rb = R.reference('gather', dict(H=H, ptr=opp[0], idx=opp[1], y=gz, outer=rc[1], inner=rc[0], mask=zc if relu else None, loops=loops, relu=False))
            assert float((rb['ref'] - y64.grad).abs().max()) <= 1e-13 * float(rb['S'].max())
            w_gy = _held('DiGCNGatherFn dy', tag, yd.grad.cpu(), dict(rb, ref=y64.grad))
            # ---- DiGCNClassFn
            cls, T = R.designed_classes(rng, n, C), R.signed(rng, C, H)
            Td = T.to(dev).requires_grad_(True)
            zk = ops.DiGCNClassFn.apply(Td, plan, cls.to(dev), reverse, alpha, beta, loops, relu)
            zk.backward(gz.to(dev))
            zkc = zk.detach().cpu()
            T64 = T.double().requires_grad_(True)
            prek = R.propagate(T64[cls.long()], e, alpha, beta, loops, rc=rc)
            ck = dict(H=H, ptr=own[0], idx=own[1], cls=cls, T=T, C=C, outer=rc[0], inner=rc[1], loops=loops, relu=relu,
                      z=zkc if relu else None, dz=gz, a0=torch.zeros(C, H))
            rkf = R.reference('class_fwd', ck)
            w_zk = _held('DiGCNClassFn z', tag, zkc, dict(rkf, ref=prek.detach().clamp_min(0) if relu else prek.detach()))
            mk = (zkc > 0).double() if relu else torch.ones_like(prek)
            (prek * mk * gz.double()).sum().backward()
            rkb = R.reference('class_bwd', ck)
            assert float((rkb['ref'] - T64.grad).abs().max()) <= 1e-13 * max(float(rkb['S'].max()), 1e-300)
            w_dT = _held('DiGCNClassFn dT', tag, Td.grad.cpu(), dict(rkb, ref=T64.grad), torch.zeros(C, H))
            print('DG ops %s C=%d | worst error / bound: gather z %.3g dy %.3g  class z %.3g dT %.3g' % (tag, C, w_z, w_gy, w_zk, w_dT))
