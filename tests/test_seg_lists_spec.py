"""Host side of the flat entry lists (no GPU): the argument checks of mgv_seg_sum_entries and mgv_seg_entries return the codes
include/mgvae_hip.h states, in the order it states them, and GraphPlan.seg_entries on CPU plans (the torch composition) is exactly
the encoding: per member position m of the order, the entry order[m], then ~idx[e] over order[m]'s list; segment pointers in entry
positions.

Every call returns before a launch and before any read through a pointer: the pointers are distinct non-NULL dummies that are never
dereferenced on the host (as in tests/test_width_refusals_spec.py)."""
import ctypes

import numpy as np
import pytest
import torch

import test_half_round_schedule as HRS
from deepgate import _hip

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
WIDTHS = (16, 32, 64, 128)
OUTSIDE = (0, 8, 24, 48, 256, -64)


def P(k):
    return ctypes.c_void_p(64 * k)


# ------------------------------------------------------------------------------------------------ mgv_seg_sum_entries
# (H, n_seg, seg_ptr, entries, direct, agg, out_row, out, stream)
def _sum(H=64, n_seg=5, seg_ptr=P(1), entries=P(2), direct=P(3), agg=P(4), out_row=P(5), out=P(6)):
    return _hip.load().mgv_seg_sum_entries(H, n_seg, seg_ptr, entries, direct, agg, out_row, out, None)


@pytest.mark.parametrize('H', OUTSIDE)
def test_sum_refuses_the_width_first(H):
    assert _sum(H=H) == EUNSUPPORTED
    assert _sum(H=H, n_seg=-1, seg_ptr=None, direct=None, out=None) == EUNSUPPORTED          # before any other check
    assert _sum(H=H, n_seg=0) == EUNSUPPORTED                                                # and before the empty problem's MGV_OK


@pytest.mark.parametrize('H', WIDTHS)
def test_sum_argument_checks(H):
    assert _sum(H=H, n_seg=-1) == EINVAL
    assert _sum(H=H, seg_ptr=None) == EINVAL
    assert _sum(H=H, direct=None) == EINVAL
    assert _sum(H=H, out=None) == EINVAL
    assert _sum(H=H, entries=None) == EINVAL                 # agg rows need a list that names them
    assert _sum(H=H, n_seg=0, seg_ptr=None) == EINVAL        # the checks come before the empty problem
    # n_seg = 0: MGV_OK with nothing launched, whichever optional pointers are there
    assert _sum(H=H, n_seg=0) == OK
    assert _sum(H=H, n_seg=0, entries=None, agg=None, out_row=None) == OK
    assert _sum(H=H, n_seg=0, agg=None) == OK


# ------------------------------------------------------------------------------------------------ mgv_seg_entries
# (n_items, items, nbr_ptr, nbr_idx, n_seg, seg_ptr, n_entries, entries, ent_seg_ptr, scratch, scratch_ints, stream)
def _build(n_items=10, items=P(1), nbr_ptr=P(2), nbr_idx=P(3), n_seg=4, seg_ptr=P(4), n_entries=30, entries=P(5), ent_seg_ptr=P(6),
           scratch=P(7), scratch_ints=None):
    if scratch_ints is None:
        scratch_ints = _hip.call_value('mgv_seg_entries_scratch_ints', max(n_items, 0))
    return _hip.load().mgv_seg_entries(n_items, items, nbr_ptr, nbr_idx, n_seg, seg_ptr, n_entries, entries, ent_seg_ptr, scratch, scratch_ints, None)


def test_builder_scratch_size():
    q = lambda n: _hip.call_value('mgv_seg_entries_scratch_ints', n)
    assert q(0) == 67 and q(10) == 2 * 10 + 1 + 66 and q(4096) == 2 * 4096 + 1 + 2 + 66       # counts [n], offsets [n + 1], scan blocks
    assert q(-1) == 0 and q(1 << 31) == 0 and q(1 << 30) == 0                                # sizes it does not serve


def test_builder_argument_checks():
    assert _build(n_items=-1) == EINVAL
    assert _build(n_seg=-1) == EINVAL
    assert _build(n_entries=9) == EINVAL                     # fewer entries than members
    assert _build(n_entries=1 << 31) == EINVAL
    assert _build(n_entries=(1 << 31) - 8) == EINVAL         # the sum kernel walks positions up to 2^31 - 9
    assert _build(seg_ptr=None) == EINVAL
    assert _build(ent_seg_ptr=None) == EINVAL
    # n_items = 0: MGV_OK, nothing written or launched — after the checks above, before the ones below
    assert _build(n_items=0, n_entries=0, seg_ptr=None) == EINVAL
    assert _build(n_items=0, n_entries=0) == OK
    assert _build(n_items=0, n_entries=0, items=None, nbr_ptr=None, nbr_idx=None, entries=None, scratch=None, scratch_ints=0) == OK
    for name in ('items', 'nbr_ptr', 'nbr_idx', 'entries', 'scratch'):
        assert _build(**{name: None}) == EINVAL, name
    need = _hip.call_value('mgv_seg_entries_scratch_ints', 10)
    assert _build(scratch_ints=need - 1) == EINVAL
    assert _build(n_items=1 << 30, n_entries=(1 << 31) - 9, scratch_ints=(1 << 40)) == EINVAL  # a size the scratch query does not serve


# ------------------------------------------------------------------------------------------------ the encoding, on CPU plans
def entries_ref(order, ptr, idx, seg_ptr):
    ent, off = [], [0]
    for m in order:
        ent.append(int(m))
        ent += [~int(j) for j in idx[ptr[m]:ptr[m + 1]]]
        off.append(len(ent))
    return np.array(ent, dtype=np.int32), np.array([off[s] for s in seg_ptr], dtype=np.int32)


@pytest.mark.parametrize('name', ['aig', 'hub', 'trees'])
def test_torch_composition_is_the_encoding(name):
    plan, xcls, _, quot = HRS._plan(name)
    st = quot[-1]
    order, tables = st['sum_levels']
    assert not plan.hip
    for rev in (st['rev'], not st['rev']):                    # (the stage's own direction, and the other CSR for good measure)
        p, i = plan.csr(rev)
        entries, esp = plan.seg_entries(rev, order, tables)
        want = entries_ref(order.numpy(), p.numpy(), i.numpy(), tables['levels'][0][1].numpy())
        assert entries.dtype == torch.int32 and esp.dtype == torch.int32
        assert np.array_equal(entries.numpy(), want[0]) and np.array_equal(esp.numpy(), want[1])
        assert entries.numel() == plan.N + plan.E and int(esp[-1]) == plan.N + plan.E
        assert plan.seg_entries(rev, order, tables)[0] is entries          # cached per direction and order tensor
    if name == 'hub':
        e = plan.seg_entries(True, order, tables)[0].numpy()
        assert int(np.diff(np.concatenate([np.nonzero(e >= 0)[0], [e.size]])).max()) - 1 >= 80      # node 5's list of 80 and more
