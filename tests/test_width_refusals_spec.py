"""Width refusals of the entries whose host code dispatches the hidden width and that no other CPU test calls with an unserved one:
the decoder / loss entries of csrc/losses.hip, csrc/link_metrics.hip, csrc/digcn_conv.hip, the heavy pull of the level sweep, and
(again, next to tests/test_sweep_spec.py) the attention pool.

Every expected code is include/mgvae_hip.h's: the width set stated with the entry, MGV_EUNSUPPORTED (-2) for any other width, and the
place of that refusal among the entry's checks (after the argument checks and the MGV_OK of an empty problem, before a workspace size is
looked at and before anything is launched).  The table was run against the library built from the commit BEFORE the launchers were
moved onto mgv::dispatch_width and passed there unchanged; no code was taken from the library under test.

The arguments pass every check that comes before the width — non-NULL dummy pointers that are never dereferenced on the host, a
non-empty problem, a row stride that covers the widest width asked for — so each call returns before any launch and before any host
read through a pointer: no GPU is needed."""
import ctypes
import re

import pytest

from deepgate import _hip

EUNSUPPORTED = -2
ALL, LANE, X3, POOL = (16, 32, 64, 128), (16, 32, 64), (32, 64), (32, 64, 128)
OUTSIDE = (0, 8, 24, 48, 256)                 # in no set
OTHER_FAMILY = {ALL: (), LANE: (128,), X3: (16, 128), POOL: (16,)}      # served by another family, not by this one

# entry -> (width set of the header, scalar arguments by name that the default of 1 would not get past the earlier checks)
ENTRIES = {
    'mgv_edge_dot_fwd': (ALL, {}),
    'mgv_edge_dot_bwd': (ALL, {}),
    'mgv_recon_loss_fwd': (ALL, {}),
    'mgv_recon_loss_bwd': (LANE, {}),
    'mgv_recon_loss_bwd_csr': (ALL, {}),
    'mgv_recon_step_csr': (ALL, {}),
    'mgv_recon_heavy_lists': (ALL, {}),
    'mgv_recon_step_heavy_lists': (ALL, {'which': 0}),
    'mgv_func_loss_fwd': (ALL, {'P': 2}),
    'mgv_func_loss_bwd': (LANE, {'P': 2}),
    'mgv_func_loss_bwd_csr': (LANE, {'P': 2}),
    'mgv_link_keys': (ALL, {}),
    'mgv_attn_pool_fwd': (POOL, {}),
    'mgv_attn_pool_bwd': (POOL, {}),
    'mgv_digcn_gather': (ALL, {}),
    'mgv_digcn_class_fwd': (ALL, {}),
    'mgv_digcn_class_bwd': (ALL, {}),
    'mgv_sweep_pull_heavy': (X3, {}),
}
STRIDES = ('ld',)                             # must be >= H and a multiple of 4: 256 covers every width of the table


def _arg_names():
    """{entry: [argument names]} from the header's declarations, in order."""
    with open(_hip.HEADER_PATH) as f:
        text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S))
    return {m.group(1): [re.findall(r'\w+', a)[-1] for a in m.group(2).split(',')]
            for m in re.finditer(r'\bint\s+(mgv_\w+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S) if m.group(2).strip() not in ('', 'void')}


def _call(name, width, overrides):
    lib, sigs, names = _hip.load(), _hip.parse_header(), _arg_names()[name]
    assert len(names) == len(sigs[name]) and names[0] in ('H', 'W') and names[-1] == 'stream'
    args = []
    for k, (n, t) in enumerate(zip(names, sigs[name])):
        if t is ctypes.c_void_p:
            args.append(ctypes.c_void_p(64 * (k + 1)))        # distinct (mgv_digcn_gather refuses out == y), 16-byte aligned, never read
        else:
            args.append(overrides.get(n, 256 if n in STRIDES else 1))
    args[0], args[-1] = width, None
    return getattr(lib, name)(*args)


CASES = [(name, w) for name, (ok, _) in ENTRIES.items() for w in OUTSIDE + OTHER_FAMILY[ok]]


@pytest.mark.parametrize('name,width', CASES, ids=['%s-%d' % c for c in CASES])
def test_unserved_width_is_refused_with_eunsupported(name, width):
    ok, overrides = ENTRIES[name]
    assert width not in ok
    assert _call(name, width, overrides) == EUNSUPPORTED


def test_the_table_covers_every_family_and_both_kinds_of_width():
    assert {ok for ok, _ in ENTRIES.values()} == {ALL, LANE, X3, POOL}
    assert all(set(OUTSIDE).isdisjoint(ok) for ok in OTHER_FAMILY)
    assert all(w not in ok and any(w in other for other in OTHER_FAMILY) for ok, ws in OTHER_FAMILY.items() for w in ws)


@pytest.mark.parametrize('width', OUTSIDE)
def test_digcn_workspace_size_of_an_unserved_width_is_zero(width):
    assert _hip.call_value('mgv_digcn_class_bwd_ws_floats', width, 1000) == 0
