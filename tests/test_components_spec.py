"""tests/components_ref.py pinned on the CPU: its three labellings agree on every builder, class_table_ref keeps its invariants, the
builders have the properties the device tests rely on, the device's hook restated with planted defects is caught by the very checker
tests/test_hip_components.py uses, and the new functions refuse on the host what they must refuse without a GPU."""
import functools
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as CR  # noqa: E402
import embed_sim_ref as ER  # noqa: E402

I32, I64 = torch.int32, torch.int64


@functools.lru_cache(maxsize=None)
def _cluster(H):
    c = CR.cluster_case(H, 1)
    pairs, r, mask = CR.truth_pairs(c['x'], c['graph_ptr'], CR.SIM_THR)
    return c, pairs, r, mask


def test_the_three_labellings_agree_on_every_builder():
    cases = dict(CR.list_cases())
    cases['forest'] = CR.forest(5001, 10002, 3)
    cases['forest + noise'] = CR.with_noise(cases['forest'])
    for name, c in cases.items():
        uf, bfs, prop = CR.uf_labels(c['pairs'], c['N']), CR.bfs_labels(c['pairs'], c['N']), CR.propagate_labels(c['pairs'], c['N'])
        assert torch.equal(uf, bfs) and torch.equal(uf, prop), name
        assert CR.check_components(uf, CR.sizes_ref(uf), bfs) == [], name
        assert torch.equal(CR.restated_union(c['pairs'], c['N']), uf), name
    # what the builders are for
    assert CR.uf_labels(CR.path(4097, 'shuffled')['pairs'], 4097).sum() == 0
    assert CR.uf_labels(CR.two_paths_joined_last(700)['pairs'], 1400).sum() == 0
    lab = CR.uf_labels(cases['forest']['pairs'], 5001)
    n_comp = int((lab == torch.arange(5001)).sum())
    assert 100 < n_comp < 1000 and bool((lab // 32 == torch.arange(5001) // 32).all())
    for k in ('clique 64', 'star centre N-1'):
        assert torch.equal(CR.uf_labels(cases[k + ' + noise']['pairs'], cases[k]['N']), CR.uf_labels(cases[k]['pairs'], cases[k]['N']))
        p = cases[k + ' + noise']['pairs']
        assert bool((p[0] == p[1]).any()) and bool((p[0] < p[1]).any()) and bool((p[0] > p[1]).any()) and p.shape[1] > cases[k]['pairs'].shape[1]


def test_class_table_ref_invariants():
    c = CR.forest(2000, 1500, 5)
    lab = CR.uf_labels(c['pairs'], c['N'])
    size = CR.sizes_ref(lab)
    for ms in (1, 2, 3, 40):
        ptr, mem = CR.class_table_ref(lab, ms)
        assert CR.check_table(ptr, mem, lab, ms) == []
        sp, sm = CR.class_table_sorted(lab, ms)
        assert torch.equal(sp, ptr) and torch.equal(sm, mem)
        assert int(ptr[0]) == 0 and int(ptr[-1]) == mem.numel() == int(size[size >= ms].sum())
        firsts = mem[ptr[:-1]]
        assert torch.equal(lab[firsts], firsts) and bool((firsts[1:] > firsts[:-1]).all())
        if ms == 2:
            single = torch.nonzero(size[lab] == 1).flatten()
            assert single.numel() > 0 and not bool(torch.isin(mem, single).any())
        if ms == 1:
            assert mem.numel() == c['N']
    ptr, mem = CR.class_table_ref(lab, 10 ** 6)
    assert ptr.tolist() == [0] and mem.numel() == 0
    # the checker sees a swapped pair of members and a class out of order
    ptr, mem = CR.class_table_ref(lab, 2)
    bad = mem.clone()
    bad[0], bad[1] = mem[1], mem[0]
    assert CR.check_table(ptr, bad, lab, 2) != []
    assert CR.check_table(ptr[:-1], mem, lab, 2) != []


@pytest.mark.parametrize('H', (64, 16))
def test_cluster_case_properties(H):
    c, pairs, r, mask = _cluster(H)
    assert c['N'] == 770 and c['graph_ptr'] == [0, 700, 770] and len(c['members']) == 300
    assert len({m // 64 for m in c['members']}) == 11                       # every row tile of the first graph
    assert pairs.shape[1] >= 44850 and pairs.shape[1] == 44850 + 3
    # a float64 truth is a fair yardstick only because no pair lies within its float32 bound of the threshold
    assert ER.band_count(r['cos'], r['bound'], CR.SIM_THR, mask) == 0
    assert float(r['bound'].max()) <= (2 * H + 6) * 2.0 ** -24 * 1.0000001
    lab = CR.uf_labels(pairs, c['N'])
    assert torch.equal(lab, CR.bfs_labels(pairs, c['N']))
    root = c['members'][0]
    assert torch.nonzero(lab == root).flatten().tolist() == c['members']
    assert int(lab[c['copy']]) == c['copy']                                 # the copy in the next graph is a class of its own
    ptr, mem = CR.class_table_ref(lab, 2)
    assert ptr.numel() - 1 == 4 and sorted((ptr[1:] - ptr[:-1]).tolist()) == [2, 2, 2, 300]
    for a, b in c['doubles']:
        assert int(lab[b]) == a and int(lab[a]) == a
    assert CR.class_table_ref(lab, 301)[0].tolist() == [0]


def test_planted_defects_are_caught_by_the_checker_of_the_device_tests():
    cases = CR.list_cases()
    caught = {}
    for defect in ('larger_root', 'drop_last', 'no_flatten'):
        hits = []
        for name, c in cases.items():
            want = CR.uf_labels(c['pairs'], c['N'])
            got = CR.restated_union(c['pairs'], c['N'], defect)
            if CR.check_components(got, CR.sizes_ref(got), want):
                hits.append(name)
        caught[defect] = hits
    assert len(caught['larger_root']) >= len(cases) - 3                     # everything with a pair
    assert 'two paths joined last' in caught['drop_last'] and 'path 4097 ascending' in caught['drop_last']
    assert 'path 4097 descending' in caught['no_flatten'] and 'two paths joined last' in caught['no_flatten']
    # the walk's defects, on the cluster: scores of the float64 unit rows stand in for the device's (the band is empty)
    c, pairs, r, _ = _cluster(16)
    want = CR.uf_labels(pairs, c['N'])
    ok = CR.restated_walk_pairs(r['cos'], c['graph_ptr'], CR.SIM_THR)
    assert torch.equal(ok, pairs)                                           # the walk's order is row-major
    assert CR.check_components(CR.restated_union(ok, c['N']), None, want) == []
    for defect in ('no_border', 'late_tile'):
        got = CR.restated_union(CR.restated_walk_pairs(r['cos'], c['graph_ptr'], CR.SIM_THR, defect), c['N'])
        assert CR.check_components(got, CR.sizes_ref(got), want) != [], defect
    got = CR.restated_union(CR.restated_walk_pairs(r['cos'], c['graph_ptr'], CR.SIM_THR, 'no_border'), c['N'])
    assert int(got[c['copy']]) == c['members'][0]
    # col >= row admits the diagonal: a node united with itself changes no component, so no labelling can show it — stated, not hidden
    diag = CR.restated_walk_pairs(r['cos'], c['graph_ptr'], CR.SIM_THR, 'col_ge_row')
    assert diag.shape[1] > pairs.shape[1] and bool((diag[0] == diag[1]).any())
    assert torch.equal(CR.restated_union(diag, c['N']), want)
    assert set(CR.DEFECTS) == {'larger_root', 'drop_last', 'no_flatten', 'no_border', 'late_tile'} and CR.HARMLESS == ('col_ge_row',)


def test_host_refusals_of_the_functions_need_no_gpu():
    from deepgate import _hip, ops, similarity
    from deepgate._model_base import FunctionalModel as M
    x, x48 = torch.zeros(4, 16), torch.zeros(4, 48)
    pairs = torch.zeros((2, 3), dtype=I64)
    E = _hip.HipLibraryError
    for route in ('walk', 'pairs'):
        with pytest.raises(E, match='GPU'):
            ops.sim_classes(x, route=route)                                 # no CPU implementation behind it
        with pytest.raises(E, match='MGV_EUNSUPPORTED'):
            ops.sim_classes(x48, route=route)
    with pytest.raises(E, match='route'):
        ops.sim_classes(x, route='host')
    for ms in (0, -1, 1.5):
        with pytest.raises(E, match='min_size'):
            ops.sim_classes(x, min_size=ms)
        with pytest.raises(E, match='min_size'):
            ops.class_table(torch.zeros(4, dtype=I32), min_size=ms)
    with pytest.raises(E, match='max_pairs'):
        ops.sim_classes(x, max_pairs=10)
    with pytest.raises(E, match='GPU'):
        ops.components(pairs, 4)
    with pytest.raises(E, match='GPU'):
        ops.class_table(torch.zeros(4, dtype=I32))
    with pytest.raises(E):
        ops.components(pairs, -1)
    with pytest.raises(E):
        ops.components(torch.zeros(3, dtype=I64), 4)
    with pytest.raises(E, match='union-find'):
        similarity._cc_status('components', [3, 7, 99, 0])
    similarity._cc_status('components', [0, 0, 0, 0])
    # the surface says what a user will meet
    for f in (ops.sim_classes, M.equivalence_classes):
        doc = ' '.join(f.__doc__.split()).lower()
        for words in ('single', 'linkage', 'below the threshold', 'hf = 0', 'nan', 'never cross graphs', '(2h + 6) 2^-24', 'threshold = 1.0'):
            assert words in doc, (f.__name__, words)
        assert inspect.signature(f).parameters['threshold'].default == 0.999 and inspect.signature(f).parameters['min_size'].default == 2
    assert inspect.signature(ops.sim_classes).parameters['route'].default == 'walk'


def test_the_header_declares_the_entries_with_their_reference_lines():
    from deepgate import _hip
    sigs = _hip.parse_header()
    want = {'mgv_cc_init': 4, 'mgv_cc_union_pairs': 7, 'mgv_cc_labels': 5, 'mgv_cc_class_count': 8, 'mgv_cc_class_fill': 11,
            'mgv_sim_union': 10}
    for name, n in want.items():
        assert len(sigs[name]) == n, name
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    for name in want:
        head = text[:text.index('int %s(' % name)]
        comment = head[head.rindex('/*'):]
        assert 'trainer.py:158-160' in comment and 'digae_layer.py:31-33' in comment, name
