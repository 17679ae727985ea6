"""CPU pins of tests/fanin_decode_ref.py, the restatement behind tests/test_hip_fanin_decode.py (mgv_fanin_decode of
csrc/pair_scores.hip, mgv_fanin_recovery of csrc/fanin_recovery.hip): the restatement against brute-force loops on every designed
case, the properties of the case builders the device tests rely on, planted defects of the restatement, the arity tables of the four
models, every refusal of both entries that needs no device, and the orthonormal design on which the device test demands full recovery."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fanin_decode_ref as FR  # noqa: E402

HS = (16, 32, 64, 128)
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2


@functools.lru_cache(maxsize=None)
def _cases(H):
    out = []
    for name, kw in FR.designed_cases(H):
        c = FR.decode_case(**kw)
        out.append((name, c, FR.dense_f32(c)))
    return out


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('H', (16, 64))
def test_restatement_equals_brute_force_loops_on_every_designed_case(H):
    for name, c, sc in _cases(H):
        a = FR.decode_ref(sc, c['key'], c['want'], c['K'], c['graph_ptr'])
        b = FR.decode_loops(sc, c['key'], c['want'], c['K'], c['graph_ptr'])
        assert FR.same_decode(a, b), name


def test_restatement_on_a_case_small_enough_to_read():
    nan = float('nan')
    #            u = 0    1    2    3
    sc = np.array([[9.0, 9.0, 9.0, 9.0],        # v = 0: key 0, nothing below it
                   [1.0, 9.0, 5.0, 9.0],        # v = 1: key 1, candidate 0 only (2 has the same key, 3 a larger one)
                   [2.0, 9.0, 9.0, 9.0],        # v = 2: key 1, wants nothing
                   [4.0, 4.0, nan, 7.0]], dtype=np.float32)   # v = 3: key 2, candidates 0, 1 (tie: 0 first); 2 is NaN; itself never
    idx, score, n_cand = FR.decode_ref(sc, [0, 1, 1, 2], [2, 2, 0, 5], 3)
    assert idx.tolist() == [[-1, -1, -1], [0, -1, -1], [-1, -1, -1], [0, 1, -1]]
    assert n_cand.tolist() == [0, 1, 0, 2]
    assert score[3].tolist() == [4.0, 4.0, -np.inf] and score[1, 0] == 1.0
    # with graphs (0, 1) (2, 3): node 3 keeps only node 2's graph, whose one candidate is NaN
    idx, _, n_cand = FR.decode_ref(sc, [0, 1, 1, 2], [2, 2, 0, 5], 3, [0, 2, 4])
    assert idx[3].tolist() == [-1, -1, -1] and n_cand.tolist() == [0, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize('H', HS)
def test_builder_properties(H):
    """Every boundary the device file names occurs in the built cases."""
    seen = dict(short=0, tie_kept=0, tie_cut=0, nan_col=0, nan_row=0, neg=0, big=0, zero_want=0, full=0)
    for name, c, sc in _cases(H):
        N, K, gp, info = c['N'], c['K'], c['graph_ptr'], c['info']
        idx, score, n_cand = FR.decode_ref(sc, c['key'], c['want'], K, gp)
        kk = FR.kept(c['want'], K)
        got = (idx >= 0).sum(1)
        assert np.array_equal(got, np.minimum(kk, n_cand))
        if gp is not None:
            assert [b - a for a, b in zip(gp, gp[1:])] == list(FR.SIZES) and any(b % 64 for b in gp[1:-1]) and 64 in gp and 128 in gp
        seen['short'] += int(((n_cand < c['want']) & (n_cand > 0)).sum())
        seen['zero_want'] += int((kk == 0).sum())
        seen['full'] += int((got == K).sum()) if K == 8 else 0
        if c['keys'] == 'equal':
            assert int(n_cand.sum()) == 0 and bool((idx == -1).all())
        if info and c['keys'] != 'equal':
            u, u2 = info['twin']
            both = (idx == u).any(1) & (idx == u2).any(1)
            for v in np.nonzero(both)[0]:
                row = idx[v].tolist()
                assert row.index(u) + 1 == row.index(u2)                   # equal scores: the lower id first, side by side
            seen['tie_kept'] += int(both.sum())
            seen['tie_cut'] += int(((idx == u).any(1) & ~(idx == u2).any(1) & (sc[:, u] == sc[:, u2])).sum())
            assert not (idx == info['nan_col']).any()
            below = FR.candidate_mask(np.zeros_like(sc), c['key'], c['want'], K, gp)[:, info['nan_col']]
            seen['nan_col'] += int(below.sum())                            # targets that would have had it as a candidate
            v = info['nan_row']
            assert n_cand[v] == 0 and (idx[v] == -1).all() and c['want'][v] == K
            seen['nan_row'] += int(FR.candidate_mask(np.zeros_like(sc), c['key'], c['want'], K, gp)[v].sum() > 0)
            assert c['want'][info['neg']] < 0 and (idx[info['neg']] == -1).all() and n_cand[info['neg']] == 0
            assert c['want'][info['big']] > K
            seen['neg'] += 1
            seen['big'] += int(got[info['big']] == min(K, n_cand[info['big']]) and n_cand[info['big']] > 0)
    print('FANIN builders H=%d | %s' % (H, seen))
    assert all(v > 0 for v in seen.values()), seen


def test_the_long_case_skips_tiles_and_has_an_idle_row_tile():
    """64 * 40 + 3 nodes in one graph, keys ascending with the id: the row tile b has no candidate behind column tile b, so with
    tile_min all but b + 1 of the 41 column tiles are skipped; the rows of tile 7 want nothing: it walks nothing."""
    c = FR.long_case(16)
    N, key, want = c['N'], c['key'], c['want']
    assert N == 64 * 40 + 3 and (want[7 * 64:8 * 64] == 0).all()
    tile_min = np.array([key[a:a + 64].min() for a in range(0, N, 64)])
    for b in (0, 1, 20, 40):
        rows = slice(64 * b, min(64 * b + 64, N))
        kmax = key[rows][FR.kept(want[rows], c['K']) > 0].max()
        walked = int((tile_min < kmax).sum())
        assert walked == b + 1 and walked < len(tile_min) or b == 40


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize('defect', FR.DEFECTS)
def test_planted_defects_change_the_result_on_the_designed_cases(defect):
    """`<=` for `<` in the key compare, the tie order reversed, `want` ignored, the graph range dropped, the row's own column allowed:
    each changes idx, score or n_cand of some designed case, so the comparison of the device file would catch it."""
    changed = []
    for name, c, sc in _cases(32):
        good = FR.decode_ref(sc, c['key'], c['want'], c['K'], c['graph_ptr'])
        bad = FR.decode_ref(sc, c['key'], c['want'], c['K'], c['graph_ptr'], defect=defect)
        if not FR.same_decode(good, bad):
            changed.append(name)
    print('FANIN defect %s | changes %d of %d cases' % (defect, len(changed), len(_cases(32))))
    assert changed
    if defect == 'tie':
        assert any('graphs' in n for n in changed)


# ------------------------------------------------------------------------------------------------ arity tables
def test_arity_tables_of_the_four_models():
    import deepgate
    from deepgate import synthetic as syn
    assert deepgate._model_base.FunctionalModel.ARITY == {'and': 2, 'or': 2, 'xor': 2, 'not': 1, 'maj': 3}
    for ctype, mod in (('aig', deepgate.dg_ae_model_aig), ('mig', deepgate.dg_ae_model_mig), ('xag', deepgate.dg_ae_model_xag),
                       ('xmg', deepgate.dg_ae_model_xmg)):
        M = mod.Model
        gate = torch.arange(-1, 8)
        got = M.gate_arity(M, gate)
        want = torch.zeros_like(gate, dtype=torch.int32)
        for name, gid in syn.GATE_IDS[ctype].items():
            if name != 'INPUT':
                want[gid + 1] = syn.FANIN[name]
        assert got.dtype == torch.int32 and torch.equal(got, want), ctype            # inputs and unknown ids: 0
        # the synthetic circuits obey their library: the arity of every gate is its true in-degree
        g = syn.make_graph(ctype, 64 + 6 * 10, 10, 3, n_inputs=64)
        deg = np.bincount(g['edge_index'][1], minlength=g['num_nodes'])
        assert np.array_equal(M.gate_arity(M, torch.from_numpy(g['gate'])).flatten().numpy(), deg)


# ------------------------------------------------------------------------------------------------ refusals on the host
def _lib():
    from deepgate import _hip
    return _hip.load()


def test_refusals_of_fanin_decode_need_no_device():
    """K, N, the strides, the alignment and the NULL pointers are looked at before any pointer is read or anything is launched (with a
    NULL graph_ptr nothing is read back), so this runs without a GPU on dummy pointers."""
    lib = _lib()
    d = ctypes.c_void_p(64)

    def rc(H=16, N=8, x=d, ldx=16, y=d, ldy=16, gp=None, G=0, key=d, want=d, K=3, tile_min=None, idx=d, score=d, n_cand=d):
        return lib.mgv_fanin_decode(H, N, x, ldx, y, ldy, gp, G, key, want, K, tile_min, idx, score, n_cand, None)

    for H in (0, 8, 24, 48, 96, 256):
        assert rc(H=H) == MGV_EUNSUPPORTED
    assert rc(H=48, K=0) == MGV_EUNSUPPORTED                          # the width is looked at first
    for K in (0, -1, 9, 32):
        assert rc(K=K) == MGV_EINVAL
    assert rc(N=-1) == MGV_EINVAL and rc(N=(2 ** 31 - 1) // 8 + 1) == MGV_EINVAL
    assert rc(gp=d, G=-1) == MGV_EINVAL
    assert rc(ldx=12) == MGV_EINVAL and rc(ldy=18) == MGV_EINVAL and rc(H=32, ldx=16) == MGV_EINVAL      # below H, no multiple of 4
    assert rc(x=ctypes.c_void_p(68)) == MGV_EINVAL and rc(y=ctypes.c_void_p(72)) == MGV_EINVAL          # not 16-byte aligned
    assert rc(x=None) == MGV_EINVAL and rc(y=None) == MGV_EINVAL
    for name in ('key', 'want', 'idx', 'score', 'n_cand'):
        assert rc(**{name: None}) == MGV_EINVAL, name
    # N = 0 launches nothing, whatever the pointers
    assert rc(N=0, x=None, y=None, key=None, want=None, idx=None, score=None, n_cand=None) == 0
    assert rc(N=0, K=9) == MGV_EINVAL and rc(N=0, H=48) == MGV_EUNSUPPORTED


def test_refusals_of_fanin_recovery_need_no_device():
    lib = _lib()
    d = ctypes.c_void_p(64)

    def rc(N=8, K=3, idx=d, tru_ptr=d, tru_src=d, gp=None, G=0, n_hit=d, rec=d):
        return lib.mgv_fanin_recovery(N, K, idx, tru_ptr, tru_src, gp, G, n_hit, rec, None)

    for K in (0, -1, 33):
        assert rc(K=K) == MGV_EINVAL
    assert rc(N=-1) == MGV_EINVAL and rc(N=(2 ** 31 - 1) // 32 + 1) == MGV_EINVAL
    assert rc(rec=None) == MGV_EINVAL and rc(N=0, rec=None) == MGV_EINVAL
    assert rc(gp=d, G=-1) == MGV_EINVAL
    assert rc(idx=None) == MGV_EINVAL and rc(tru_ptr=None) == MGV_EINVAL


def test_the_header_declares_both_entries_with_their_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_fanin_decode']) == 16 and len(sigs['mgv_fanin_recovery']) == 10
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in ('mgv_fanin_decode', 'mgv_fanin_recovery'):
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'digae_model.py:118-122' in comment


def test_host_side_refusals_and_edges():
    from deepgate import _hip, metrics, ops, pairs
    assert ops.fanin_decode is pairs.fanin_decode and ops.fanin_edges is pairs.fanin_edges and ops.fanin_recovery is metrics.fanin_recovery
    s = torch.zeros(4, 16)
    with pytest.raises(_hip.HipLibraryError, match='MGV_EUNSUPPORTED'):
        ops.fanin_decode(torch.zeros(4, 48), torch.zeros(4, 48), [0] * 4, [1] * 4)
    with pytest.raises(_hip.HipLibraryError, match='GPU'):
        ops.fanin_decode(s, s, [0] * 4, [1] * 4)                # no CPU implementation behind it
    idx = torch.tensor([[2, 0, -1], [-1, -1, -1], [1, -1, -1], [0, 1, 2]], dtype=torch.int32)
    assert ops.fanin_edges(idx).tolist() == [[2, 0, 1, 0, 1, 2], [0, 0, 2, 3, 3, 3]]     # by target, then by rank; sources on row 0
    # the true lists: ascending, repeats dropped, one scan
    tp, ts = metrics.true_fanin_lists(torch.tensor([[3, 1, 3, 0, 1], [2, 2, 2, 3, 0]]), 4)
    assert tp.tolist() == [0, 1, 1, 3, 4] and ts.tolist() == [1, 1, 3, 0] and ts.dtype == torch.int32
    with pytest.raises(ValueError, match='outside'):
        metrics.true_fanin_lists(torch.tensor([[4], [0]]), 4)


# ------------------------------------------------------------------------------------------------ recovery
def test_recovery_restatement_on_a_case_small_enough_to_read():
    ei = np.array([[0, 1, 0, 0, 2], [2, 2, 2, 3, 3]])                  # 2 <- {0, 1} (0 listed twice), 3 <- {0, 2}
    idx = np.array([[1, -1], [-1, -1], [1, 0], [0, 9]], dtype=np.int32)   # row 0 decodes where nothing is true; row 3 holds an id out of range
    n_hit, rec = FR.recovery_ref(idx, ei)
    assert n_hit.tolist() == [0, 0, 2, 1] and rec.tolist() == [[2, 1, 3, 4, 4]]
    n_hit, rec = FR.recovery_ref(idx, ei, [0, 2, 3, 4])
    assert rec.tolist() == [[0, 0, 0, 0, 0], [1, 1, 2, 2, 2], [1, 0, 1, 2, 2]]


def test_recovery_builder_properties():
    c = FR.recovery_case()
    gp, idx, ei = c['graph_ptr'], c['idx'], c['edge_index']
    assert all(c['kinds'].get(k, 0) > 0 for k in range(10)), c['kinds']      # every kind of damage, and rows with empty true lists
    assert len({(u, v) for u, v in ei.T.tolist()}) < ei.shape[1]              # repeated true edges
    assert ((idx >= c['N']) | (idx < -1)).any() and (idx == -1).any()
    n_hit, rec = FR.recovery_ref(idx, ei, gp)
    assert rec[0].tolist() == [0] * 5 and rec[2].tolist() == [0] * 5 and rec[4].tolist() == [0] * 5     # graphs without gates, an empty graph
    assert all(0 < rec[g][1] < rec[g][0] for g in (1, 3, 5))                 # some gates exact, some not, in every gate graph
    assert gp[3] < 256 < gp[4] and gp[5] < 512 < gp[6]                        # graphs across workgroup borders of 256 rows


# ------------------------------------------------------------------------------------------------ the orthonormal design
@pytest.mark.parametrize('H', HS)
def test_orthonormal_design_is_recovered_exactly_by_the_restatement(H):
    """The condition under which the device test may demand exact == gates: a true fan-in scores 1, every other candidate 0, to within
    float32 rounding, every true fan-in has a smaller key, and want is the true degree."""
    c = FR.ortho_case(H)
    sc = FR.dense_f32(c)
    ei, key = c['edge_index'], c['key']
    assert (key[ei[0]] < key[ei[1]]).all() and c['N'] > 128                    # levelised, and more than two row tiles
    true = np.zeros_like(sc, dtype=bool)
    true[ei[1], ei[0]] = True
    same = FR.graph_of(c['N'], c['graph_ptr'])
    same = same[:, None] == same[None, :]
    assert np.abs(sc[true] - 1).max() < 1e-4 and np.abs(sc[~true & same]).max() < 1e-4
    idx, score, n_cand = FR.decode_ref(sc, key, c['want'], c['K'], c['graph_ptr'])
    n_hit, rec = FR.recovery_ref(idx, ei, c['graph_ptr'])
    print('FANIN ortho H=%d | %d graphs, gates %d exact %d' % (H, rec.shape[0], rec[:, 0].sum(), rec[:, 1].sum()))
    assert (rec[:, 0] > 0).all() and np.array_equal(rec[:, 1], rec[:, 0]) and np.array_equal(rec[:, 2], rec[:, 3])
    assert np.array_equal(rec[:, 3], rec[:, 4]) and int(rec[:, 3].sum()) == ei.shape[1]
