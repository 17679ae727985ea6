"""Per-batch graph structure ("plan") consumed by the HIP kernels.

Replaces, for the whole batch at once, what the reference recomputes inside every forward:
`torch.stack([edge_index[1], edge_index[0]])` (digae_layer.py:264), the boolean level/gate masks and
`forward_index[mask]` (dg_ae_model_aig.py:72-75) and the per-node edge scans of `subgraph`
(utils/dag_utils.py:91-105, O(nodes x E) Python) — with two CSRs and a list of 64-node tiles
bucketed by (level, gate type).  Two builders give identical arrays: on the GPU plan_device.py, the callers of the HIP kernels of
csrc/plan_build.hip; on CPU tensors (host-logic tests, and `MGV_PLAN=torch` as the GPU tests' cross-check)
plan_torch.py, torch sorts and scans.  This module keeps GraphPlan: the thresholds, the public methods, the choice of builder and
the cache of the derived tables.  It is batch construction, not part of the timed train step.
"""
import os

import numpy as np

import torch

from . import plan_device, plan_torch
from .plan_device import DECLINED
from .plan_torch import NO_GATE, TILE  # noqa: F401  (TILE: the width of a sweep tile, named here for the plan's readers)


class TableCache:
    """The derived tables of a plan, addressed by (kind, key).  An entry holds the tensors its key was derived from and hits only
    while each of them is the same OBJECT (an address can be reused, an object cannot).  A kind declared `level_derived` where it
    is built is dropped when the plan's levels are set again."""

    def __init__(self):
        self._entries, self._level_kinds = {}, set()

    def get(self, kind, key, build, held=(), level_derived=False):
        """The value of (kind, key), built by `build()` unless it is there for these very `held` tensors."""
        hit = self._entries.get((kind, key))
        if hit is not None and len(hit[0]) == len(held) and all(a is b for a, b in zip(hit[0], held)):
            return hit[1]
        return self.put(kind, key, build(), held, level_derived)

    def put(self, kind, key, value, held=(), level_derived=False):
        self._level_kinds.update([kind] if level_derived else [])
        self._entries[(kind, key)] = (tuple(held), value)
        return value

    def peek(self, kind, key=None):
        """The stored value, or None — also where None is what was built (a table above its cap, no heavy node): `kind in cache`
        says whether anything was."""
        hit = self._entries.get((kind, key))
        return None if hit is None else hit[1]

    def drop(self, *kinds):
        self._entries = {k: v for k, v in self._entries.items() if k[0] not in kinds}

    def drop_level_derived(self):
        self.drop(*self._level_kinds)

    def __contains__(self, kind):
        return any(k[0] == kind for k in self._entries)

    def __len__(self):
        return len(self._entries)


class GraphPlan:
    """in-CSR  : in_ptr[N+1], in_src[E]              sources of each node, original edge order kept
    out-CSR : out_ptr[N+1], out_dst[E], out_slot[E] destinations; out_slot = position of that edge
                                                     in the in-CSR (per-edge scratch is in-CSR ordered)
    sweep   : gslot[N] aggregator slot of a node (255 = never updated), order[] = updated nodes sorted
              by (level, slot), tiles of <= 64 consecutive `order` entries with one slot each,
              level_tile_ptr[L+1] = tile range of each level (levels >= 1)
    Built by plan_device.py (`hip`: device tensors, unless MGV_PLAN=torch) or plan_torch.py; every derived table lives in `cache`.
    """

    def __init__(self, edge_index, num_nodes, device=None):
        dev = edge_index.device if device is None else torch.device(device)
        ei = edge_index.to(dev)
        N = int(num_nodes)
        E = int(ei.shape[1])
        if N >= 2 ** 31 or E >= 2 ** 31:
            raise ValueError('node/edge counts must fit int32')
        self.N, self.E = N, E
        self._status = None
        self.cache = TableCache()
        self._pick_builder(dev)
        self.__dict__.update(self._build.csr(ei[0].long().contiguous(), ei[1].long().contiguous(), N))
        self.has_levels = False

    def _pick_builder(self, device):
        self.device = torch.device(device)
        self.hip = self.device.type == 'cuda' and os.environ.get('MGV_PLAN', 'hip') != 'torch'

    @property
    def _build(self):
        """The builder module of this plan (not kept as an attribute: whoever walks a plan's tensors would walk the module)."""
        return plan_device if self.hip else plan_torch

    @property
    def _graph(self):
        return plan_torch.Graph(self.N, self.E, self.in_ptr, self.in_src, self.in_dst, self.out_ptr, self.out_dst, self.out_slot)

    def asap_levels(self):
        """ASAP level of every node (the round of utils/dag_utils.top_sort in which it is evaluated = longest path from a source),
        by frontier relaxation over the out-CSR on the device.  Raises on a cycle.  -> int64 [N]"""
        self._check_status()
        return self._build.asap_levels(self._graph)

    def _check_status(self):
        """Read the device CSR builder's status, once (edge ids outside [0, N) raise here, before the lists are read)."""
        st, self._status = self._status, None
        if st is not None and int(st[0].item()) != 0:
            raise ValueError('edge_index holds node ids outside [0, num_nodes)')

    def csr(self, reverse):
        """(ptr, idx) of the neighbours a node sums over: in-neighbours, or out-neighbours when the
        edges are flipped (`r_edge_index`, digae_layer.py:264)."""
        return (self.out_ptr, self.out_dst) if reverse else (self.in_ptr, self.in_src)

    def tagged_idx(self, reverse, class_id):
        """The neighbour array of `csr(reverse)` with each neighbour's (degree, class) table row in the top byte (entry = node | row << 24):
        what the struct-stage kernels read in table mode.  Cached per direction and class-id tensor."""
        def build():
            idx = self.csr(reverse)[1]
            return (idx | (class_id[idx.long()] << 24)).to(torch.int32).contiguous()
        return self.cache.get('tagged', reverse, build, held=(class_id,), level_derived=True)

    def tagged_fits(self, n_classes):
        """Whether `tagged_idx` entries can hold every node id (24 bits) and every row of a table of `n_classes` rows (8 bits)."""
        return self.N < (1 << 24) and n_classes <= 256

    def count_self_loops(self):
        """Edges (v, v): the negative sampler draws E - self loops + N pairs (sampling.negative_sampling_device).  One host read-back,
        kept on the plan."""
        return self.cache.get('self_loops', None, lambda: int((self.in_src == self.in_dst).sum().item()) if self.E > 0 else 0)

    @property
    def num_self_loops(self):
        """The count of `count_self_loops`, or None before its first call."""
        return self.cache.peek('self_loops')

    def warm(self, xcls=None, quotient_stages=0):
        """Build, on the CURRENT stream, the per-batch caches a train step would otherwise build lazily inside the step (each with a
        host read-back): the quotient stages with the flat entry list of the boundary's gradient sums (seg_entries), or the first-stage
        (degree, class) table and the tagged lists of the half round after it; the heavy-row lists and their segments.  The batch
        prefetcher calls this on its worker's stream, beside the previous step."""
        self.count_self_loops()
        for rev in (False, True):
            self.heavy(rev)
            self.heavy_segments(rev)
        if self.has_levels:
            self.heavy_segments(True, inactive_only=True)
            self.heavy_segments(True, active_by_level=True)
        from . import ops
        if self.has_levels and ops.PACKED_ROWS == 2:
            self.order_rows                  # (default: a plan builds its packed sweep rows when it comes back for a second step, ops._sweep_rows)
        if isinstance(quotient_stages, (tuple, list, set)) and len(quotient_stages) == 0:
            return self                      # an encoder without half rounds (DirectedGCNConvEncoder): no colour classes, no first-stage table
        counts = sorted({int(c) for c in (quotient_stages if isinstance(quotient_stages, (tuple, list, set)) else [quotient_stages]) if int(c) > 0})
        if xcls is not None and self.N > 0 and counts and ops.QUOTIENT:
            staged = [self.quotient(xcls, c) for c in counts]
            if ops.SEG_LISTS:
                for c, stages in zip(counts, staged):
                    if 0 < len(stages) < c:  # a per-node half round follows: its gradient is summed per colour over the flat entry list
                        self.seg_entries(stages[-1]['rev'], *stages[-1]['sum_levels'])
            if all([len(stages) > 0 for stages in staged]):
                return self                  # the quotient stages replace the first-stage table and its tagged lists
        if xcls is not None and self.N > 0:
            first = self.first_stage_classes(xcls)
            if first is not None and self.tagged_fits(first[1]):
                self.tagged_idx(True, first[0])
        return self

    HEAVY_ROW = plan_torch.HEAVY_ROW      # csrc/struct_stage_x3_common.h: kHeavyRow

    def heavy(self, reverse):
        """(count, node ids int32 ascending) of the nodes with more than HEAVY_ROW neighbours in `csr(reverse)` — clock/reset-like
        nets.  The struct-stage launchers sum such lists in a pre-pass (one workgroup per node).  Built once per plan and direction
        (one host round trip); empty on most batches."""
        def build():
            p = self.csr(reverse)[0]
            nodes = torch.nonzero((p[1:] - p[:-1]) > self.HEAVY_ROW).reshape(-1).to(torch.int32)
            return (int(nodes.numel()), nodes.contiguous())
        return self.cache.get('heavy', reverse, build)

    HEAVY_SEG = 512     # list entries per workgroup of the heavy-list kernels

    def heavy_segments(self, reverse, inactive_only=False, active_by_level=False):
        """The heavy nodes' lists (see `heavy`) cut into segments of HEAVY_SEG entries for the per-node pull kernels whose
        lists they are (reconstruction-loss backward over the positive edges, the sweep backward's pulls):
        dict(K, nodes, node_seg_ptr[K+1], S, seg_node[S], seg_e0[S], seg_e1[S]) of int32 device arrays, or None when there
        are none.  `inactive_only`: only nodes without an aggregator slot; `active_by_level`: only nodes WITH one, ordered by
        (level, id), plus host lists lvl_k_ptr / lvl_seg_ptr [num_levels + 1] (the nodes / segments of each level); both need
        set_levels."""
        key = (reverse, inactive_only, active_by_level)
        return self.cache.get('heavy_segments', key, lambda: self._heavy_segments(*key), level_derived=True)

    def _heavy_segments(self, reverse, inactive_only, active_by_level):
        K, nodes = self.heavy(reverse)
        out = None
        lv = None
        if K > 0 and (inactive_only or active_by_level):
            act = self.gslot[nodes.long()] != NO_GATE
            nodes = nodes[act if active_by_level else ~act].contiguous()
            K = int(nodes.numel())
            if K > 0 and active_by_level:
                lv_dev = self.level[nodes.long()].long()
                order = torch.sort(lv_dev * (self.N + 1) + nodes.long()).indices          # by (level, id)
                nodes = nodes[order].contiguous()
                lv = lv_dev[order].cpu().numpy()
        if K > 0:
            p = self.csr(reverse)[0]
            e0 = p[nodes.long()].cpu().numpy().astype(np.int64)
            e1 = p[nodes.long() + 1].cpu().numpy().astype(np.int64)
            seg_node, s0, s1, nsp = [], [], [], [0]
            for k in range(K):
                for b in range(int(e0[k]), int(e1[k]), self.HEAVY_SEG):
                    seg_node.append(k); s0.append(b); s1.append(min(b + self.HEAVY_SEG, int(e1[k])))
                nsp.append(len(seg_node))
            i32 = dict(dtype=torch.int32, device=self.device)
            out = dict(K=K, nodes=nodes, node_seg_ptr=torch.tensor(nsp, **i32), S=len(seg_node), seg_node=torch.tensor(seg_node, **i32),
                       seg_e0=torch.tensor(s0, **i32), seg_e1=torch.tensor(s1, **i32))
            if lv is not None:
                L = max(self.num_levels, 1)
                cnt = np.bincount(lv, minlength=L)
                kp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
                out['lvl_k_ptr'] = [int(v) for v in kp]
                out['lvl_seg_ptr'] = [int(nsp[int(v)]) for v in kp]
        return out

    def first_stage_classes(self, xcls, max_classes=256):
        """(degree, feature class) pairs of the forward CSR: every node enters the first half round of an encoder with
        the same state (ones, digae_layer.py:260), so its output row there depends on that pair alone.  Returns
        (class_id[N] int32, C, ptr[C+1], idx[sum deg], xcls[C]) — one representative row per pair whose `deg`
        neighbours all point at row 0 (any row: the representatives' inputs are all ones) — or None when there are
        more than `max_classes` pairs.  Cached per xcls tensor and cap."""
        def build():
            out = self._build.first_stage_pairs(self._graph, xcls, max_classes)
            if out is DECLINED:              # the device builder's pair kernels, at a degree above 255: the torch builder numbers the pairs
                out = plan_torch.first_stage_pairs(self._graph, xcls, max_classes)
            return out
        return self.cache.get('first_stage', int(max_classes), build, held=(xcls,))

    QUOTIENT_FRACTION = 2.0    # a half round runs on distinct rows only while they are at most N / 2 (measured: DESIGN.md 4.3)
    QUOTIENT_GROWTH = 8        # colours multiply by at least this per half round (config 2: x50, x226, x48): the next one is not even tried if C * 8 would not qualify

    QUOTIENT_MIN_NODES = 131072  # below: a step is launch-bound, the extra small launches cost more than the rows save (65,536 nodes: 7.40 ms with, 7.18 without; 262,144: 10.8 / 11.3)

    QUOTIENT_DEVICE = True      # hip plans: a stage's tables by the plan builder's kernels (plan_device.quotient_stages); False: the torch stage loop around the device's keys and check

    def quotient(self, xcls, max_stages, force=False):
        """Quotient stages of the structural encoder.  Every node starts from the same state (ones, digae_layer.py:260), so after
        half round t a node's row depends only on its colour: (feature class, colour after t-1, multiset of its neighbours' colours
        after t-1) — colour refinement over the alternating in- / out-CSR.  While the colours are few (early half rounds of any
        netlist: three gate types, bounded fan-in), the half round is computed on ONE row per colour.  Returns a list of stages
        t = 1, 2, ... (possibly empty), each a dict:
            C        colours after the stage;  cid [N] int32 colour of every node;  rev  the stage gathers over the out-CSR
            ptr [C+1], idx int32: a representative's neighbour list, entries = C + (colour after t-1) — rows of the stacked input
                     [own rows (C) | table of stage t-1 (C_prev)] the fp32 stage kernels read;  own [C] int64: colour after t-1;
                     ent_idx / own32: the same lists and own colours as plain int32 rows of the table of stage t-1 (the bf16x3
                     kernels read that table in place: own rows through own32)
            xcls [C] uint8, heavy: (count, rows with more than HEAVY_ROW neighbours)
            own_rows/own_levels, ent_rows/ent_levels: per colour of stage t-1 the representatives that own it / whose lists name it,
                     as segment tables of mgv_seg_sum (backward)
        and the last stage also `sum_levels` (class_sum_levels) for the per-colour sums of the per-node gradient.
        Grouping is proposed by a 64-bit key (two sums of random per-colour values over the neighbour list, folded with the own
        colour, class and degree) and then CHECKED exactly: every member against its colour's representative, list entry by list
        entry (lists sorted by colour); refinement stops at the first disagreement, so a key collision costs speed, never
        correctness.  Cached per xcls tensor and stage count (the source and the target encoder may ask for different ones).
        `force`: the torch stage loop also below QUOTIENT_MIN_NODES, and stages go on while C * 1.1 <= N instead of stopping by
        QUOTIENT_FRACTION / QUOTIENT_GROWTH (small CPU plans of the host-logic tests)."""
        return self.cache.get('quotient', int(max_stages), lambda: self._quotient_stages(xcls, int(max_stages), force), held=(xcls,))

    def _quotient_stages(self, xcls, max_stages, force):
        N, g = self.N, self._graph
        self._check_status()
        if not ((force or N >= self.QUOTIENT_MIN_NODES) and self.E > 0):
            return []
        # which stages run on colours, stated once for both builders (force: until the graph is nearly fully refined)
        admits = lambda C: C * (1.1 if force else self.QUOTIENT_FRACTION) <= N
        goes_on = lambda C: force or C * self.QUOTIENT_GROWTH * self.QUOTIENT_FRACTION <= N
        if self.QUOTIENT_DEVICE and not force:
            return self._build.quotient_stages(g, xcls, max_stages, admits, goes_on)
        return plan_torch.quotient_stages(g, xcls, max_stages, admits, goes_on, *self._build.colour_key_and_check(g, xcls, not force))

    class_sum_levels = staticmethod(plan_torch.class_sum_levels)      # (the torch composition; plan_device.class_sum_levels fills the same tables from counts)
    # the builders' pieces that the tests hold one by one, under the names they have on the plan
    _colour_lists_equal = staticmethod(plan_torch.colour_lists_equal)
    _sort_by_key_dev = staticmethod(plan_device.sort_by_key)
    _class_sum_levels_dev = staticmethod(plan_device.class_sum_levels)

    def _key_bits(self, Cp):
        return plan_device.key_bits(self.N, Cp)

    def seg_entries(self, reverse, order, tables):
        """The flat entry list of mgv_seg_sum_entries for level 1 of `tables` (class_sum_levels) over the members `order` with the
        neighbour pull over `csr(reverse)`: (entries int32, ent_seg_ptr int32 [n_seg + 1]); `order` names every node at most once (the
        nodes sorted by colour), so the list holds at most N + E entries.  In member order, per member position m:
        the entry order[m] (>= 0: a row of `direct`, starts a new member), then ~idx[e] for e in [ptr[order[m]], ptr[order[m] + 1])
        (< 0: a row of `agg`, continues the member); ent_seg_ptr[s] = seg_ptr[s] + the list lengths of the members in front of it.
        Everything the kernel would otherwise resolve per call (order -> ptr -> idx) is static per plan: built once, by the builder
        of the plan, and cached per direction, `order` tensor and level-1 segment-pointer tensor.  The encoders of a model share the
        plan's quotient stages, so they share the list."""
        n_seg, seg_ptr = tables['levels'][0][0], tables['levels'][0][1]
        return self.cache.get('seg_entries', (bool(reverse), id(order), id(seg_ptr)),
                              lambda: self._build.seg_entries(self._graph, reverse, order, n_seg, seg_ptr), held=(order, seg_ptr))

    ROW_INTS = plan_torch.ROW_INTS      # func_level_x3_common.h kRowInts
    ROW_OUT = plan_torch.ROW_OUT

    @property
    def order_rows(self):
        """Packed sweep rows [n_active, 32] int32 (one 128-byte line per updated node, sweep order): {in0, in1, out0, out1}, the first 4
        in-edge sources (-1: none), the first 8 consumers as (node, in-CSR slot) pairs (node -1: none), their gate slots as bytes.
        The level kernels reach a tile's lists with this ONE load level instead of span -> CSR lists -> gslot."""
        return self.cache.get('order_rows', None, lambda: self._build.order_rows(self._graph, self.n_active, self.order, self.order_span,
                                                                                self.gslot), level_derived=True)

    def set_levels(self, gate, forward_level, gate_ids):
        """Bucket the nodes a Model updates: level >= 1 and gate id in `gate_ids` (list, position =
        aggregator slot).  Mirrors `layer_mask & <gate>_mask` of the reference level loop.  Drops the cached tables derived from
        gslot / level (and the tagged neighbour arrays): stale once the levels are set again, which `data.plan_of` does when a
        batch meets a model with another gate set."""
        self._check_status()                 # before anything consumes the CSR
        self.cache.drop_level_derived()
        fields = self._set_levels_hip(gate, forward_level, gate_ids) if self.hip else DECLINED
        if fields is DECLINED:               # a torch plan, or more than 8,192 (level, slot) keys for the device's counting sort: the torch builder on the same CSR
            fields = plan_torch.set_levels(self._graph, gate, forward_level, gate_ids)
        self.__dict__.update(fields)
        self.has_levels = True
        return self

    def _set_levels_hip(self, gate, forward_level, gate_ids):
        """The device builder's level fields, or DECLINED (False): the seam at which a test sees that it was asked once."""
        return plan_device.set_levels(self._graph, gate, forward_level, gate_ids)

    def to(self, device):
        """Move the plan: its arrays go to `device`, the builder is picked for it, and the derived tables are dropped (rebuilt on
        demand, identical).  A plan that is already there stays as it is."""
        if self.in_ptr.to(device) is self.in_ptr:
            return self
        self._check_status()
        for k, v in list(self.__dict__.items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        self._keep = None
        self.cache = TableCache()
        self._pick_builder(device)
        return self

    def slot_nodes(self):
        """Node ids (int64, ascending) of every aggregator slot's updated nodes: what a round >= 2 of the sweep gathers to form
        W_hh h_prev per gate type.  Cached per levelisation."""
        assert self.has_levels
        return self.cache.get('slot_nodes', None, lambda: [torch.nonzero(self.gslot == s_).reshape(-1) for s_ in range(self.num_slots)],
                              level_derived=True)
