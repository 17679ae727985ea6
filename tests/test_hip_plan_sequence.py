"""GPU tests of GraphPlan as a whole on one small batch: the C-ABI entries a device plan calls, in order, and its host read-backs,
from construction to the warmed tables (the guard against a builder that quietly launches something twice or adds a round trip);
and a device-built plan moved to the CPU against one built there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GATE_IDS = [1, 2]


def _arrays():
    """Two AIGs of 384 nodes; primary input 3 of the first also drives 70 gates of its levels >= 2 (a heavy out-list)."""
    from deepgate import synthetic as syn
    graphs = [syn.make_graph('aig', 64 + 16 * 20, 16, 31 + i, n_inputs=64) for i in range(2)]
    a = syn.collate(graphs)
    later = np.nonzero(graphs[0]['forward_level'] >= 2)[0]
    rng = np.random.Generator(np.random.PCG64(9))
    hub = np.stack([np.full(70, 3), rng.choice(later, size=70, replace=False)])
    a['edge_index'] = np.unique(np.concatenate([a['edge_index'], hub], axis=1), axis=1)
    return a


def _inputs(a, dev):
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    return t(a['edge_index']), t(a['gate']), t(a['forward_level']), t(a['x'][:, 1].astype('uint8'))


def _record(dev):
    """(entry names in call order, host read-backs) of: build, set_levels, warm for 4 stages, quotient(4), the last stage's entry list.
    Read-backs are the calls of Tensor.item and Tensor.tolist; a synchronising int(tensor), bool(tensor) or .cpu() is not counted."""
    from deepgate import _hip
    from deepgate.graph_plan import GraphPlan
    ei, gate, level, xcls = _inputs(_arrays(), dev)
    torch.cuda.synchronize()
    names, reads = [], [0]
    real = _hip.call, _hip.call_value, torch.Tensor.item, torch.Tensor.tolist

    def named(f):
        return lambda name, *a: (names.append(name), f(name, *a))[1]

    def counted(f):
        def g(self, *a):
            reads[0] += 1
            return f(self, *a)
        return g
    old = GraphPlan.QUOTIENT_MIN_NODES
    GraphPlan.QUOTIENT_MIN_NODES = 1
    _hip.call, _hip.call_value, torch.Tensor.item, torch.Tensor.tolist = named(real[0]), named(real[1]), counted(real[2]), counted(real[3])
    try:
        plan = GraphPlan(ei, int(xcls.numel()))
        assert plan.hip
        plan.set_levels(gate, level, GATE_IDS)
        plan.warm(xcls, quotient_stages=4)
        stages = plan.quotient(xcls, 4)
        plan.seg_entries(stages[-1]['rev'], *stages[-1]['sum_levels'])
    finally:
        _hip.call, _hip.call_value, torch.Tensor.item, torch.Tensor.tolist = real
        GraphPlan.QUOTIENT_MIN_NODES = old
    return names, reads[0], plan, stages


SEQUENCE = [
    'mgv_plan_csr_scratch_ints', 'mgv_plan_csr', 'mgv_plan_keys', 'mgv_plan_check_levels', 'mgv_count_sort_scratch_ints',
    'mgv_count_sort_i32', 'mgv_plan_tile_counts', 'mgv_plan_tiles', 'mgv_count_sort_scratch_ints', 'mgv_count_sort_i32',
    'mgv_sort_pairs_temp_ints', 'mgv_plan_pairs', 'mgv_count_sort_scratch_ints', 'mgv_count_sort_i32',
    'mgv_count_sort_scratch_ints', 'mgv_count_sort_i32', 'mgv_seg_level_work_ints', 'mgv_seg_level_scan', 'mgv_seg_level_fill',
    'mgv_seg_level_work_ints', 'mgv_seg_level_scan', 'mgv_seg_level_fill', 'mgv_colour_keys', 'mgv_sort_pairs',
    'mgv_colour_groups', 'mgv_colour_check', 'mgv_colour_rep_rows', 'mgv_colour_rep_lists', 'mgv_count_sort_scratch_ints',
    'mgv_count_sort_i32', 'mgv_count_sort_scratch_ints', 'mgv_count_sort_i32', 'mgv_seg_level_work_ints', 'mgv_seg_level_scan',
    'mgv_seg_level_fill', 'mgv_seg_level_work_ints', 'mgv_seg_level_scan', 'mgv_seg_level_fill', 'mgv_seg_level_work_ints',
    'mgv_seg_level_scan', 'mgv_seg_level_fill', 'mgv_seg_level_work_ints', 'mgv_seg_level_scan', 'mgv_seg_level_fill',
    'mgv_seg_level_work_ints', 'mgv_seg_level_scan', 'mgv_seg_level_fill', 'mgv_seg_entries_scratch_ints', 'mgv_seg_entries',
]
READ_BACKS = 20


def test_entries_called_and_host_read_backs_are_the_recorded_ones():
    """The recorded list and count are those of the commit before the builders were split into plan_torch.py / plan_device.py."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    names, reads, plan, stages = _record(torch.device('cuda:0'))
    assert 2 <= len(stages) < 4 and plan.heavy(True)[0] == 1       # a keyed stage behind the pair table, a per-node half round, a heavy list
    assert names == SEQUENCE
    assert reads == READ_BACKS


def _same(a, b, name):
    """Field by field: tensors with torch.equal (and one dtype), containers entry by entry, the rest with ==."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.device == b.device and a.dtype == b.dtype and torch.equal(a, b), name
    elif isinstance(a, dict):
        assert set(a) == set(b), name
        for k in a:
            _same(a[k], b[k], (name, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), name
        for k, (u, v) in enumerate(zip(a, b)):
            _same(u, v, (name, k))
    else:
        assert a == b, name


def test_a_device_built_plan_moved_to_the_cpu_equals_one_built_there():
    """GraphPlan.to('cpu') on a device-built, levelled and warmed plan: the torch builder takes over (`hip` false), the cache is
    empty, and set_levels, first_stage_classes, quotient(force=True) and order_rows equal those of a plan built on the CPU from
    the same arrays."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepgate.graph_plan import GraphPlan
    a = _arrays()
    ei, gate, level, xcls = _inputs(a, torch.device('cuda:0'))
    moved = GraphPlan(ei, int(xcls.numel()))
    assert moved.hip
    moved.set_levels(gate, level, GATE_IDS).warm(xcls)
    assert len(moved.cache) > 0 and moved.to('cuda:0') is moved and len(moved.cache) > 0       # already there: nothing moves, nothing is dropped
    moved.to('cpu')
    assert not moved.hip and moved.device == torch.device('cpu') and len(moved.cache) == 0
    ei, gate, level, xcls = _inputs(a, torch.device('cpu'))
    home = GraphPlan(ei, int(xcls.numel()))
    assert not home.hip
    fields = ['in_ptr', 'in_src', 'in_dst', 'out_ptr', 'out_dst', 'out_slot', 'gslot', 'level', 'num_levels', 'order', 'order_span', 'tile_start',
              'tile_count', 'tile_slot', 'slot_tiles', 'slot_tile_ptr', 'level_tile_ptr', 'num_tiles', 'n_active', 'num_slots']
    for first in (True, False):                          # the levels the device set, then the levels set again after the move
        if not first:
            moved.set_levels(gate, level, GATE_IDS)
        home.set_levels(gate, level, GATE_IDS)
        for name in fields + ['order_rows']:
            _same(getattr(moved, name), getattr(home, name), name)
    _same(moved.first_stage_classes(xcls), home.first_stage_classes(xcls), 'first_stage_classes')
    got, want = moved.quotient(xcls, 4, force=True), home.quotient(xcls, 4, force=True)
    assert len(want) >= 2
    _same(got, want, 'quotient')
    _same(moved.seg_entries(got[-1]['rev'], *got[-1]['sum_levels']), home.seg_entries(want[-1]['rev'], *want[-1]['sum_levels']), 'seg_entries')
    _same(moved.heavy_segments(True), home.heavy_segments(True), 'heavy_segments')
