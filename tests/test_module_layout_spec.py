"""The layout of the host side: ops.py is the train step's operators; the analysis surface lives in pairs.py (the decoder on all
pairs), similarity.py (cosine search on hf, classes) and metrics.py (ranking and accuracy), which depend on _hip and on each other
in that order and never on ops.  ops re-binds their public names — the documented ops.pair_select, ops.sim_classes, ops.link_ranks
... are the home modules' objects — and none of their underscored helpers: patching one through ops must fail, not patch an
alias.  Every textual reference to a name of the four modules, anywhere in the tree, resolves.  No GPU, no built library."""
import os
import re
import sys

import pytest

from conftest import PKG_PARENT, ROOT  # noqa: E402

if PKG_PARENT not in sys.path:
    sys.path.insert(0, PKG_PARENT)
from deepgate import metrics, ops, pairs, similarity  # noqa: E402

HOMES = {'ops': ops, 'pairs': pairs, 'similarity': similarity, 'metrics': metrics}

MOVED = {
    pairs: ('_pair_rows _pair_ld _pair_operands _PAIR_WIDTHS _pair_width _pair_graphs _free_bytes _dense_fits PairScoresFn pair_scores '
            'pair_scores_at pair_topk _list_room _select_room _count_scan_fill pair_select reconstruct_edges reconstruction_counts '
            'dense_scores PROFILE_MAX_EDGES _profile_edges pair_profile counts_above reconstruction_curve'),
    similarity: ('SIM_THRESHOLD row_unit sim_topk _sim_room sim_pairs sim_at _unit_profile sim_profile _f32 _f32_key _edges_between '
                 'threshold_search sim_threshold_for _CC_ERR _cc_status _cc_forest _cc_labels _cc_from_pairs _min_size components '
                 '_class_table class_table sim_classes'),
    metrics: ('LinkRanks RankLists RankMetrics pair_rank_counts _rank_by _rank_rows _f32_order_key _run_ends link_rank_lists '
              'link_rank_filter link_ranks rank_metrics LINK_RECORD_WORDS link_record link_auc_ap read_link_records CONCORD_TILE '
              'CONCORD_MAX_GAPS MIN_GAP segment_table pair_segments _concord_gaps concord_counts function_accuracy'),
}
MOVED_NAMES = [(home, name) for home, names in MOVED.items() for name in names.split()]


def test_the_name_lists_are_complete_and_disjoint():
    assert [len(v.split()) for v in MOVED.values()] == [24, 23, 24]
    assert len({n for _, n in MOVED_NAMES}) == len(MOVED_NAMES)


@pytest.mark.parametrize('home,name', MOVED_NAMES, ids=['%s.%s' % (h.__name__.rsplit('.', 1)[1], n) for h, n in MOVED_NAMES])
def test_ops_rebinds_public_names_and_no_private_one(home, name):
    assert hasattr(home, name), 'it lives in its home module'
    if name.startswith('_'):
        assert not hasattr(ops, name), 'a re-bound private helper would be an alias: patching it through ops would patch nothing'
    else:
        assert getattr(ops, name) is getattr(home, name)


def test_edge_rows_and_the_dtype_names_are_stated_once_in_hip():
    from deepgate import _hip
    assert ops.edge_rows is _hip.edge_rows is pairs.edge_rows and not hasattr(ops, '_edge_rows')
    for mod in (ops, pairs, similarity, metrics):
        assert mod.F32 is _hip.F32 and mod.I32 is _hip.I32


IMPORTS_OPS = re.compile(r'from\s+\.\s+import\s[^\n]*\bops\b|from\s+\.ops\b|import\s+deepgate\.ops\b|from\s+deepgate\s+import\s[^\n]*\bops\b'
                         r'|from\s+deepgate\.ops\b')


@pytest.mark.parametrize('mod', [pairs, similarity, metrics], ids=['pairs', 'similarity', 'metrics'])
def test_the_new_modules_do_not_import_ops(mod):
    with open(mod.__file__) as f:
        src = f.read()
    assert not IMPORTS_OPS.search(src)
    assert IMPORTS_OPS.search('    from . import ops\n') and IMPORTS_OPS.search('from .ops import linear') \
        and IMPORTS_OPS.search('import deepgate.ops') and IMPORTS_OPS.search('from deepgate import _hip, ops')
    # and the order among the three: pairs <- similarity <- metrics
    later = {pairs: ('similarity', 'metrics'), similarity: ('metrics',), metrics: ()}[mod]
    for name in later:
        assert not re.search(r'from\s+\.%s\b|from\s+\.\s+import\s[^\n]*\b%s\b' % (name, name), src)


# a `from deepgate import a, b as c` / `from . import (a, b)` statement and the module names it binds
FROM_PACKAGE = re.compile(r'^[ \t]*from[ \t]+(?:deepgate|\.+)[ \t]+import[ \t]+(\([^)]*\)|[^\n]*)', re.M)
REFERENCE = re.compile(r'(?<![\w.])(deepgate\.)?(ops|pairs|similarity|metrics)\.([A-Za-z_]\w*)')


def _bound(src):
    names = set()
    for m in FROM_PACKAGE.finditer(src):
        for part in re.sub(r'#[^\n]*', '', m.group(1)).strip('()').split(','):
            words = part.split()
            if words and len(words) == 1:             # `x as y` binds y, not the module's own name
                names.add(words[0])
    return names


def _sources():
    out = [os.path.join(ROOT, 'bench.py'), os.path.join(ROOT, '__graft_entry__.py')]
    for top in ('multi-gate-vae_amd', 'tests', 'tools'):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            out += [os.path.join(d, f) for f in files if f.endswith('.py')]
    return sorted(out)


def test_every_reference_to_a_name_of_the_four_modules_resolves():
    """A name reached through one of the four module names, wherever the file binds that name to the deepgate module (from deepgate
    import ... / from . import ...) or reaches it through the imported package; code, comments and docstrings alike.  `py` after the
    dot is a file name, and the prefix as another object's attribute (self. ...) is not the module."""
    dangling, seen = [], 0
    for path in _sources():
        with open(path) as f:
            src = f.read()
        bound = _bound(src)
        package = re.search(r'^[ \t]*import[ \t]+deepgate\b', src, re.M) is not None
        for m in REFERENCE.finditer(src):
            via_package, prefix, name = m.groups()
            if name == 'py' or not (package if via_package else prefix in bound):
                continue
            seen += 1
            if not hasattr(HOMES[prefix], name):
                dangling.append('%s:%d: %s' % (os.path.relpath(path, ROOT), src.count('\n', 0, m.start()) + 1, m.group(0)))
    assert seen >= len(MOVED_NAMES), 'the search found the tree: the package alone calls most of the moved public names'
    assert not dangling, '\n'.join(dangling)
