"""Plain restatements of the Linear and row-sum entries of csrc/dense.hip and csrc/linear_x3.hip (with the fixed-order reduction of
csrc/mgv_slab.h they rely on), working from exactly what the C ABI takes (include/mgvae_hip.h), plus the builders of the cases
tests/test_hip_dense_reference.py runs on the device.  CPU only; pinned to independent formulations by tests/test_dense_spec.py,
which also asserts the properties of the builders and shows that the planted defects are far outside the device bounds.

  linear(X1, X2, W, b, R, dY)       Y = [X1 | X2] W^T + b + R;  dX = dY W (the forward with the transposed weight, as
                                    ops.LinearFn.backward calls it);  dW = dY^T [X1 | X2];  db = column sums of dY
  grouped(X, W, b, R, tables, dY)   the same over tile tables: row r of tile t is node order[tile_start[t] + r], r < tile_count[t], with
                                    the weights and bias of slot tile_slot[t]; tile_list (or None) names the tiles; 'named' = the node
                                    rows some listed tile names (the others must not be touched).  A tile of count 0 is ALLOWED by the
                                    header: it names no row and adds nothing.
  pair(S, T, Wl, bl, Wd, bd, ...)   the hs seam of mgv_linear_pair_fwd_x3 / _bwd_x3, composed of linear(): HS = [S | T] Wl^T + bl,
                                    ST = HS Wd^T + bd (of its own HS, and 'ST_given' of an HS handed in); with HS given, dhs = dST Wd + gHS
                                    (an fp32 value in the kernel before it is split into planes), dS | dT = dhs Wl, dWl = dhs^T [S | T],
                                    dbl = colsum(dhs), dWd = dST^T HS, dbd = colsum(dST)
  wpack(W, transpose)               the bf16 hi / lo bit patterns of mgv_wpack_bf16x3, fragment order
  gather_sum / seg_sum / class_expand / class_pull_sum

Arithmetic: dtype float64; dtype float32 with mm = 'exact' (the stand-in for the fp32 kernels); mm = 'x3' (float32 only: every matrix
product through struct_stage_ref.mm3, the stand-in for the bf16x3 kernels).  gather_sum and seg_sum add in the order the kernel comments
promise (list order; seg_sum: a member's own row, then its neighbours in list order, then the member into the segment's sum, members in
list order), so their float32 run is what the device must return bit for bit.  Every restatement takes mutate = (kind, ...): ONE planted
defect (tests/test_dense_spec.py).

Scales S (float64 without a defect): per ENTRY the sum of the magnitudes of the terms behind it: Y |X| |W|^T + |b| + |R|, dX |dY| |W|,
dW |dY|^T |X|, db the column sums of |dY|, the row sums the same sums over |rows|.  An error is judged against S of its own entry:
tests/struct_stage_ref.ratio.  The case builders scale every row by its own power of ten from [-3, 3], so a bound on the whole
matrix's largest entry would hide an error in a small row and the per-entry bound does not."""
import numpy as np
import torch

import struct_stage_ref as SR
from struct_stage_ref import F32, F64, GRID_CAP, TILE, grid_for, mm3, ratio  # noqa: F401

THREADS = 256                      # mgv_common.h kThreads
LDS_BYTES = 160 * 1024
ROW_U = 4                          # dense.hip k_class_pull_sum: rows per lane group in flight (U)
SLAB_PHASES = 16                   # mgv_slab.h k_slab_sum P
SLAB_UNROLL = 8                    # loads in flight per thread in its unrolled loop

X3_SHAPES = ((64, 128), (128, 64), (64, 64), (64, 32), (32, 64), (32, 32))          # linear_x3.hip mgv_linear_x3_supported
X3_WGRAD_WAVES = {(64, 128): 8, (128, 64): 8, (64, 64): 8, (64, 32): 8, (32, 64): 8, (32, 32): 4, (192, 64): 6}     # MGV_WGX(.., NW, ..)
F32_FWD_M, F32_FWD_K = (16, 32, 64, 128), (16, 48, 128, 256)
F32_WGRAD_SHAPES = ((16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 16), (64, 32), (64, 64), (64, 128), (128, 64))   # MGV_WG list
GROUPED_FWD, GROUPED_WGRAD = ((192, 64), (64, 192)), ((192, 64),)
WIDTHS = (16, 32, 64, 128)


# ------------------------------------------------------------------------------------------------ launch geometry, restated
def x3_fwd_smem(M, K):             # linear_x3.hip LinFwdGeom::smem_bytes: two bf16 planes of K + 8, the fp32 output stage of M + 4
    return 2 * TILE * (K + 8) * 2 + TILE * (M + 4) * 4


def x3_wgrad_smem(M, K):           # LinWgGeom::smem_bytes: hi / lo planes of dY (M + 8) and of X (K + 8), M floats for db
    return 2 * TILE * (M + 8) * 2 + 2 * TILE * (K + 8) * 2 + M * 4


# kernel: (workgroups per CU handed to grid_for, rows a workgroup takes per visit, the source line restated)
GEOMETRY = {
    'linear_fwd': (lambda s: 8, lambda s: TILE, 'dense.hip launch_linear_fwd: grid_for(ntiles, 8)'),
    'linear_wgrad': (lambda s: 2, lambda s: TILE, 'dense.hip launch_linear_wgrad: grid_for(ntiles, 2)'),
    'linear_fwd_x3': (lambda s: min(4, LDS_BYTES // x3_fwd_smem(*s)), lambda s: TILE,
                      'linear_x3.hip launch_linear_fwd_x3: per_cu = min(4, 160 KiB / smem_bytes)'),
    'linear_wgrad_x3': (lambda s: min(1024 // (64 * X3_WGRAD_WAVES[s]), LDS_BYTES // x3_wgrad_smem(*s)), lambda s: TILE,
                        'linear_x3.hip launch_linear_wgrad_x3: per_cu = min(1024 / NT, 160 KiB / smem_bytes)'),
    'linear_pair_fwd_x3': (lambda s: 2, lambda s: TILE, 'linear_x3.hip mgv_linear_pair_fwd_x3: grid = grid_for(ntiles, 2)'),
    'linear_pair_bwd_x3': (lambda s: 2, lambda s: TILE, 'linear_x3.hip pair_bwd_grid: grid_for(ntiles, 2), the grid of hs_linear\'s backward'),
    'gather_sum': (lambda H: 16, lambda H: THREADS // (H // 4), 'dense.hip mgv_gather_sum: row_grid<H>(N, 16) = grid_for(ceil(N / rows_per_block), 16)'),
    'seg_sum': (lambda H: 16, lambda H: THREADS // (H // 4), 'dense.hip mgv_seg_sum: row_grid<H>(n_seg, 16) = grid_for(ceil(n_seg / rows_per_block), 16)'),
    'class_expand': (lambda H: 16, lambda H: THREADS // (H // 4), 'dense.hip mgv_class_expand: row_grid<H>(N, 16) = grid_for(ceil(N / rows_per_block), 16)'),
    'class_pull_sum': (lambda H: 8, lambda H: THREADS // (H // 4), 'dense.hip mgv_class_pull_sum: row_grid<H>(N, 8) = grid_for(ceil(N / rows_per_block), 8); U = 4'),
}


def per_cu(kernel, shape):
    return GEOMETRY[kernel][0](shape)


def unit_rows(kernel, shape):
    return GEOMETRY[kernel][1](shape)


def grid(kernel, shape, N):
    u = unit_rows(kernel, shape)
    return grid_for((N + u - 1) // u, per_cu(kernel, shape))


def cap_rows(kernel, shape):
    """(Off by one against the wording "the row count FROM which a workgroup visits a second tile": that count is cap_rows + 1.)
    The LARGEST row count at which every workgroup visits one tile (one row per lane group): the grid cap times the rows of a
    visit.  From cap_rows + 1 on, workgroup 0 comes round a second time.  (k_class_pull_sum takes its U = 4 rows per lane group one
    grid stride apart: u = 1 is reached from cap_rows + 1, the outer loop's second pass from 4 cap_rows + 1.)"""
    return GRID_CAP * per_cu(kernel, shape) * unit_rows(kernel, shape)


def large_rows(kernel, shape):
    """2 cap_rows + 5 tiles + 19 rows: workgroups 0..5 visit three tiles, the others two, the last tile is partial; the prefetch
    condition tile + gridDim.x < ntiles is true and false inside one launch."""
    return 2 * cap_rows(kernel, shape) + 5 * TILE + 19


def visits(kernel, shape, N):
    """Tiles every workgroup visits (round-robin: tile = blockIdx.x + k gridDim.x)."""
    u = unit_rows(kernel, shape)
    nt, g = (N + u - 1) // u, grid(kernel, shape, N)
    return [len(range(b, nt, g)) for b in range(g)]


def slab_passes(nwg):
    """k_slab_sum over nwg slab rows: per row phase ty (rows ty, ty + 16, ...) the (passes of the eight-loads-in-flight loop, rows left
    to its tail loop)."""
    out = []
    for ty in range(SLAB_PHASES):
        g, unrolled = ty, 0
        while g + (SLAB_UNROLL - 1) * SLAB_PHASES < nwg:
            g += SLAB_UNROLL * SLAB_PHASES
            unrolled += 1
        out.append((unrolled, len(range(g, nwg, SLAB_PHASES))))
    return out


def slab_regime(nwg):
    """'short' (fewer rows than phases: some phases add nothing), 'phases' (every phase its tail loop only), 'mixed' (some phases
    reach the unrolled loop, others not: 113 .. 127 rows), 'unrolled' (every phase one or more unrolled passes, no tail) or
    'unrolled+tail'."""
    p = slab_passes(nwg)
    if nwg < SLAB_PHASES:
        return 'short'
    if all(u == 0 for u, _ in p):
        return 'phases'
    if any(u == 0 for u, _ in p):
        return 'mixed'
    return 'unrolled+tail' if any(t > 0 for _, t in p) else 'unrolled'


FLOOR = {'f32': 2.0 ** -23, 'x3': 2.0 ** -17}
U24 = 2.0 ** -24


def taus(r64, rk, mm):
    """The device bound per output: tau = 8 max(r, floor), r the worst ratio of the CPU restatement in the kernel's arithmetic (rk: the
    float32 or bf16x3-emulation run on the same inputs) against the float64 run r64, floor 2^-23 (fp32 kernels) or 2^-17 (bf16x3)."""
    return {k: 8 * max(ratio(rk[k], r64[k], S), FLOOR[mm]) for k, S in r64['S'].items() if k in rk}


def ratios(got, r64):
    return {k: ratio(got[k], r64[k], S) for k, S in r64['S'].items() if k in got}


def chain_length(kernel, output, shape, N):
    """L: the longest chain of sequential float32 additions the kernel's design makes for one entry of `output` (every addition is
    counted as sequential, also the four products one fp32 MFMA adds to its accumulator).  Stated only for the output whose device
    bound uses it (a correct kernel was measured outside tau there: NOTEBOOK.md, 2026-10-18):
      linear_wgrad dW   a wave keeps its 16 rows' share of a tile in registers: 4 MFMA accumulations of 4 products per visited tile (16
                        per visit); then the 4 waves of each of the g workgroups add their partial to the accumulator with a float atomic,
                        in arrival order: 4 g."""
    if (kernel, output) == ('linear_wgrad', 'dW'):
        return 16 * max(visits(kernel, shape, N)) + 4 * grid(kernel, shape, N)
    raise KeyError((kernel, output))


def device_bound(kernel, output, shape, N, tau):
    """The bound the device test uses: tau, or max(tau, L 2^-24) for the outputs with a stated chain length."""
    try:
        return max(tau, chain_length(kernel, output, shape, N) * U24)
    except KeyError:
        return tau


SMALL_ROWS = (1, 2, 63, 64, 65, 127, 129)
SLAB_TILES = (1, 2, 15, 16, 17, 127, 128, 129, 147)          # x3 weight gradient below the cap: grid = slab rows = tiles


def slab_rows(tiles):
    return TILE * (tiles - 1) + 5                             # a last tile of 5 rows


# ------------------------------------------------------------------------------------------------ arithmetic
def _mm(a, b, mm, kind=None):
    if mm == 'x3':
        if kind == 'drop_hilo':                               # hi.hi + lo.hi only
            ah, al = SR._split(a)
            bh, _ = SR._split(b)
            return ah @ bh + al @ bh
        return mm3(a, b)
    return a @ b


def linear(X1, X2, W, b=None, R=None, dY=None, dtype=F64, mm='exact', mutate=None):
    """{'Y', and with dY: 'dX', 'dW', 'db', and for float64 without a defect 'S'}.  Defects: ('drop_last_row',) the last row (of a
    partial tile) neither written nor summed; ('seam',) the four columns after the X1 | X2 seam read from X1's row (its next four
    floats: the next row's first columns); ('drop_hilo',); ('no_residual',); ('slab_from_128',) rows of tile 128 on not in dW / db;
    ('db_second_phase', rows) db from the first `rows` rows of every tile only; ('stale_prefetch', grid) the second tile a workgroup
    visits computed from the rows of its first."""
    assert mm == 'exact' or dtype == F32
    kind = mutate[0] if mutate else None
    cv = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    X = cv(X1) if X2 is None else torch.cat([cv(X1), cv(X2)], 1)
    N, K1 = X1.shape
    if kind == 'seam':
        assert X2 is not None
        X = X.clone()
        X[:, K1:K1 + 4] = torch.roll(cv(X1)[:, :4], -1, 0)
    if kind == 'stale_prefetch':
        rows = torch.arange(N)
        second = (rows >= mutate[1] * TILE) & (rows < 2 * mutate[1] * TILE)
        rows[second] -= mutate[1] * TILE
        X = X[rows]
    Wc = cv(W)
    Y = _mm(X, Wc.t(), mm, kind)
    if b is not None:
        Y = Y + cv(b)
    if R is not None and kind != 'no_residual':
        Y = Y + cv(R)
    keep = torch.ones(N, 1, dtype=dtype)
    if kind == 'drop_last_row':
        Y[N - 1] = 0
        keep[N - 1] = 0
    if kind == 'slab_from_128':
        keep[128 * TILE:] = 0
    out = {'Y': Y}
    if dY is not None:
        G = cv(dY)
        out['dX'] = _mm(G, Wc, mm, kind)
        out['dW'] = _mm((G * keep).t(), X, mm, kind)
        Gb = G * keep
        if kind == 'db_second_phase':
            Gb = Gb * ((torch.arange(N) % TILE) < mutate[1]).to(dtype)[:, None]
        out['db'] = Gb.sum(0)
    out = {k: v.to(F64) for k, v in out.items()}
    if dtype == F64 and mutate is None:
        aX, aW = X.abs(), Wc.abs()
        S = {'Y': aX @ aW.t() + (0 if b is None else cv(b).abs()) + (0 if R is None else cv(R).abs())}
        if dY is not None:
            S.update(dX=G.abs() @ aW, dW=G.abs().t() @ aX, db=G.abs().sum(0))
        out['S'] = S
    return out


PAIR = (64, 128)                   # the pair kernels serve one shape (Wl 64 x 128, Wd 128 x 64): the `shape` of their GEOMETRY entries
PAIR_OUT = ('dS', 'dT', 'dWl', 'dbl', 'dWd', 'dbd')
PAIR_SLAB = 64 * 128 + 64 + 128 * 64 + 128          # linear_x3.hip PairBwdGeom::slab_l + slab_d: workspace floats per workgroup


def stale_rows(N, g):
    """Row r of the second tile a workgroup of a grid of g visits -> the same row of its first tile (the row its stale registers
    hold); the other rows themselves."""
    rows = torch.arange(N)
    second = (rows >= g * TILE) & (rows < 2 * g * TILE)
    rows[second] -= g * TILE
    return rows


def last_visit_rows(N, g):
    """[N][1] bool: the rows of the tile its workgroup (of a grid of g, round-robin) visits last."""
    nt = (N + TILE - 1) // TILE
    return (torch.arange(N) // TILE + g >= nt)[:, None]


def pair(S_, T_, Wl, bl=None, Wd=None, bd=None, dST=None, gHS=None, HS=None, dtype=F64, mm='exact', mutate=None):
    """{'HS', 'ST' (of that HS), 'ST_given' (HS handed in: of it); with dST: 'dhs', 'dS', 'dT', 'dWl', 'dbl', 'dWd', 'dbd' of the
    backward whose given input is HS (None: this run's own HS); float64 without a defect: 'S'}.  Every product is linear()'s; what
    the kernels keep unstored between two products (hs in LDS, dhs in LDS) is the float32 value linear() returns, handed on as it is.
    S: |X| |Wl|^T + |bl| for HS, that scale times |Wd|^T + |bd| for ST, |HS| |Wd|^T + |bd| for ST_given; Sdhs = |dST| |Wd| + |gHS|,
    and dS | dT, dWl, dbl take Sdhs as their operand's magnitude: Sdhs |Wl|, Sdhs^T |S | T|, colsum(Sdhs); dWd |dST|^T |HS|, dbd
    colsum |dST|.
    Defects (g = the grid): ('stale_fwd', g) S | T of the second tile a workgroup visits from its first tile's rows;
    ('stale_bwd_gh', g) dST and HS so; ('stale_bwd_x', g) S | T of the backward so; ('stale_bwd_ghs', g) gHS alone so;
    ('last_visit', out, g) a workgroup's sum `out` (dWd, dWl, dbl, dbd) kept from the tile it visits last only; ('no_ghs',) gHS
    not added to dhs; ('dbl_no_ghs',); ('st_unbiased',) ST from hs before bl was added; ('drop_last_row',) the last row neither
    written nor summed; ('drop_hilo_dhs',) the hi.lo term missing from dST Wd; ('dbd_half',) rows 32 .. 63 of each tile not in dbd."""
    assert mm == 'exact' or dtype == F32
    kind = mutate[0] if mutate else None
    N = S_.shape[0]
    drop = ('drop_last_row',) if kind == 'drop_last_row' else None
    lin = lambda *a, **k: linear(*a, dtype=dtype, mm=mm, **k)      # noqa: E731
    stale = stale_rows(N, mutate[1]) if kind and kind.startswith('stale') else None
    Sf, Tf = (S_[stale], T_[stale]) if kind == 'stale_fwd' else (S_, T_)
    f1 = lin(Sf, Tf, Wl, bl, mutate=drop)
    out = {'HS': f1['Y']}

    def st_of(h):
        if kind == 'st_unbiased' and bl is not None:
            h = (h.to(dtype) - bl.to(dtype)).to(F64)
        return lin(h, None, Wd, bd, mutate=drop)

    f2 = st_of(f1['Y'])
    out['ST'] = f2['Y']
    fg = None
    if HS is not None:
        fg = st_of(HS)
        out['ST_given'] = fg['Y']
    if dST is not None:
        Hg = f1['Y'] if HS is None else HS
        G, Hb, Xs, Xt, R = dST, Hg, S_, T_, None if kind == 'no_ghs' else gHS
        if kind == 'stale_bwd_gh':
            G, Hb = dST[stale], Hg[stale]
        if kind == 'stale_bwd_x':
            Xs, Xt = S_[stale], T_[stale]
        if kind == 'stale_bwd_ghs' and R is not None:
            R = gHS[stale]
        d = lin(G, None, Wd.t(), None, R, mutate=('drop_hilo',) if kind == 'drop_hilo_dhs' else None)
        dhs = d['Y']                                           # fp32 in the kernel: split into planes and summed into dbl as it is
        bd_ = lin(Hb, None, Wd, None, None, G, mutate=drop)    # dWd, dbd
        bl_ = lin(Xs, Xt, Wl, None, None, dhs, mutate=drop)    # dS | dT, dWl, dbl
        out.update(dhs=dhs, dS=bl_['dX'][:, :64], dT=bl_['dX'][:, 64:], dWl=bl_['dW'], dbl=bl_['db'], dWd=bd_['dW'], dbd=bd_['db'])
        if kind == 'last_visit' or kind == 'dbd_half':
            which = mutate[1] if kind == 'last_visit' else 'dbd'
            keep = last_visit_rows(N, mutate[2]) if kind == 'last_visit' else ((torch.arange(N) % TILE) < 32)[:, None]
            if which in ('dWd', 'dbd'):
                out[which] = lin(Hb, None, Wd, None, None, (G.to(dtype) * keep).to(F64))['dW' if which == 'dWd' else 'db']
            else:
                out[which] = lin(Xs, Xt, Wl, None, None, (dhs.to(dtype) * keep).to(F64))['dW' if which == 'dWl' else 'db']
        if kind == 'dbl_no_ghs':
            out['dbl'] = lin(Xs, Xt, Wl, None, None, lin(G, None, Wd.t())['Y'])['db']
    if dtype == F64 and mutate is None:
        aWd = Wd.to(F64).abs()
        S = {'HS': f1['S']['Y'], 'ST': f1['S']['Y'] @ aWd.t() + (0 if bd is None else bd.to(F64).abs())}
        if fg is not None:
            S['ST_given'] = fg['S']['Y']
        if dST is not None:
            sc = linear(S_, T_, Wl, None, None, d['S']['Y'])['S']
            S.update(dhs=d['S']['Y'], dS=sc['dX'][:, :64], dT=sc['dX'][:, 64:], dWl=sc['dW'], dbl=sc['db'], dWd=bd_['S']['dW'], dbd=bd_['S']['db'])
        out['S'] = S
    return out


def tile_nodes(tables, listed=True):
    """(node of every row of the listed tiles, its tile's slot), in list order (int64).  listed=False: of all tiles."""
    order, ts, tc, slot = (tables[k].long() for k in ('order', 'tile_start', 'tile_count', 'tile_slot'))
    tl = tables.get('tile_list')
    tiles = torch.arange(ts.numel()) if tl is None or not listed else tl.long()
    nodes = [order[int(ts[t]):int(ts[t]) + int(tc[t])] for t in tiles]
    slots = [torch.full((int(tc[t]),), int(slot[t])) for t in tiles]
    z = torch.zeros(0, dtype=torch.int64)
    return torch.cat(nodes + [z]), torch.cat(slots + [z])


def grouped(X, W, b, R, tables, dY=None, dtype=F64, mm='exact', mutate=None):
    """{'Y' [rows of X][M] (zero in the rows no listed tile names), 'named' (bool per row); with dY: 'dW', 'db' over the rows of the
    listed tiles (one slot's list: the slots are not looked at), 'S'}.  W [T][M][K] or None (weight gradient only), b [T][M] or None.
    Defects: ('bias_slot0',) slot 0's bias for every tile; ('write_outside_list',) every tile computed although tile_list names a
    subset; ('drop_last_row',) the last row of the last listed non-empty tile; ('drop_hilo',)."""
    assert mm == 'exact' or dtype == F32
    kind = mutate[0] if mutate else None
    cv = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    Xc = cv(X)
    nodes, slots = tile_nodes(tables)
    named = torch.zeros(X.shape[0], dtype=torch.bool)
    named[nodes] = True
    out = {'named': named}
    S = {}
    if W is not None:
        wn, ws = tile_nodes(tables, listed=kind != 'write_outside_list')
        if kind == 'drop_last_row':
            wn, ws = wn[:-1], ws[:-1]
        M = W.shape[1]
        Y = torch.zeros(X.shape[0], M, dtype=dtype)
        Sy = torch.zeros(X.shape[0], M, dtype=F64)
        for s in sorted(set(ws.tolist())):
            sel = wn[ws == s]
            y = _mm(Xc[sel], cv(W[s]).t(), mm, kind)
            sy = Xc[sel].abs().to(F64) @ W[s].to(F64).abs().t()
            if b is not None:
                bs = b[0 if kind == 'bias_slot0' else s]
                y, sy = y + cv(bs), sy + bs.to(F64).abs()
            if R is not None:
                y, sy = y + cv(R)[sel], sy + R.to(F64)[sel].abs()
            Y[sel], Sy[sel] = y, sy
        out['Y'], S['Y'] = Y.to(F64), Sy
    if dY is not None:
        gn = nodes[:-1] if kind == 'drop_last_row' else nodes
        G = cv(dY)[gn]
        out['dW'], out['db'] = _mm(G.t(), Xc[gn], mm, kind).to(F64), G.sum(0).to(F64)
        S['dW'], S['db'] = G.abs().to(F64).t() @ Xc[gn].abs().to(F64), G.abs().to(F64).sum(0)
    if dtype == F64 and mutate is None:
        out['S'] = S
    return out


def wpack(W, transpose):
    """(hi, lo) int16 bit patterns, R K each, of A = W (R x K) or its transposed view: hi = bf16(A) (round to nearest even),
    lo = bf16(A - hi) (the difference is exact in float32), in MFMA fragment order: blocks (row tile of 16, k-step of 32) of 512
    elements, lane 16 q + r of a block holds A[16 rt + r][32 ks + 8 q .. + 7] at offset 8 lane."""
    A = (W.t() if transpose else W).to(F32)
    Rn, K = A.shape
    hi = A.to(torch.bfloat16)
    lo = (A - hi.to(F32)).to(torch.bfloat16)
    frag = lambda w: w.reshape(Rn // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1).contiguous().view(torch.int16)      # noqa: E731
    return frag(hi), frag(lo)


def _list_sum(start, src, ptr, idx, rows, drop_pos=None):
    """start[m] + src[idx[ptr[rows[m]] + 0]] + src[idx[... + 1]] + ..., added one list position at a time (list order) in start's
    dtype.  idx None: the entry's position is its row.  drop_pos: that list position is skipped (a defect)."""
    p0 = ptr.long()[rows]
    d = ptr.long()[rows + 1] - p0
    acc = start.clone()
    on = torch.arange(d.numel())
    for k in range(int(d.max()) if d.numel() else 0):
        on = on[d[on] > k]
        if k == drop_pos:
            continue
        e = p0[on] + k
        acc[on] = acc[on] + src[e if idx is None else idx.long()[e]]
    return acc


def _with_scale(fn, dtype, mutate):
    out = fn(dtype, False)
    if dtype == F64 and mutate is None:
        out['S'] = {k: v for k, v in fn(F64, True).items() if torch.is_floating_point(v) and k != 'deg'}
    return out


def gather_sum(h, ptr, idx, dtype=F64, mutate=None):
    """agg[i] = h[idx[ptr[i]]] + h[idx[ptr[i] + 1]] + ... in list order, deg[i] = the list's length.  Defect: ('drop_pos', k)."""
    N = ptr.numel() - 1

    def run(dt, mag):
        src = h.to(dt).abs() if mag else h.to(dt)
        agg = _list_sum(torch.zeros(N, h.shape[1], dtype=dt), src, ptr, idx, torch.arange(N), mutate[1] if mutate else None)
        return {'agg': agg.to(F64), 'deg': (ptr[1:] - ptr[:-1]).to(F64)}
    return _with_scale(run, dtype, mutate)


def seg_sum(seg_ptr, items, direct, agg, nbr_ptr, nbr_idx, out_row, dtype=F64, mutate=None):
    """{'out' [n_seg][H] per SEGMENT, 'rows' the row of the caller's matrix each segment writes}.  Defects: ('drop_pos', k) a member's
    k-th neighbour, ('drop_member', k) a segment's k-th member."""
    n_seg = seg_ptr.numel() - 1
    total = int(seg_ptr[-1])
    kind = mutate[0] if mutate else None

    def run(dt, mag):
        f = (lambda t: t.to(dt).abs()) if mag else (lambda t: t.to(dt))
        rows = items.long()[:total] if items is not None else torch.arange(total)
        v = f(direct)[rows]
        if agg is not None:
            v = _list_sum(v, f(agg), nbr_ptr, nbr_idx, rows, mutate[1] if kind == 'drop_pos' else None)
        out = _list_sum(torch.zeros(n_seg, direct.shape[1], dtype=dt), v, seg_ptr, None, torch.arange(n_seg), mutate[1] if kind == 'drop_member' else None)
        return {'out': out.to(F64)}
    res = _with_scale(run, dtype, mutate)
    res['rows'] = out_row.long() if out_row is not None else torch.arange(n_seg)
    return res


def class_expand(table, class_id):
    return table[class_id.long()]


def class_pull_sum(gy_direct, gy_agg, ptr, idx, class_id, C, dtype=F64, mutate=None):
    """out[c] = sum over the nodes of class c of (gy_direct[i] + its neighbours' gy_agg rows in list order); the sum over the nodes as
    a product with the class indicator matrix.  Defects: ('drop_pos', k); ('fold_class', a, b) class a counted as b; ('lost_u', u,
    stride) the rows a lane group reaches as its u-th (node0 + u stride) lost."""
    N = class_id.numel()
    kind = mutate[0] if mutate else None

    def run(dt, mag):
        f = (lambda t: t.to(dt).abs()) if mag else (lambda t: t.to(dt))
        v = f(gy_direct).clone()
        if gy_agg is not None:
            v = _list_sum(v, f(gy_agg), ptr, idx, torch.arange(N), mutate[1] if kind == 'drop_pos' else None)
        cls = class_id.long().clone()
        if kind == 'fold_class':
            cls[cls == mutate[1]] = mutate[2]
        if kind == 'lost_u':
            v[(torch.arange(N) // mutate[2]) % ROW_U == mutate[1]] = 0
        ind = torch.zeros(C, N, dtype=dt)
        ind[cls, torch.arange(N)] = 1
        return {'out': (ind @ v).to(F64)}
    return _with_scale(run, dtype, mutate)


# ------------------------------------------------------------------------------------------------ cases
NAN = float('nan')


def _gen(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def scaled_rows(g, n, w, last_on_top=False, first_on_top=0):
    """[n][w] float32 standard normal, every row times its own power of ten from [-3, 3]; last_on_top: the last row gets 10^3 (a
    partial tile's last row is then the largest term of every sum over the rows: with a random scale it can be too small for its loss
    to show in dW); first_on_top: so do that many first rows (one row past the grid cap ONE workgroup visits a second tile: what it
    carries over from its first, 64 rows of 32,769, must weigh enough in a sum over all rows for its loss to show)."""
    e = g.uniform(-3, 3, (n, 1))
    e[:first_on_top] = 3
    if last_on_top:
        e[n - 1] = 3
    return torch.from_numpy((g.standard_normal((n, w)) * 10.0 ** e).astype(np.float32))


class Operand:
    """An [n][w] float32 matrix as the ABI takes it: contiguous, or (strided) columns 4 .. 4 + w of a matrix 8 columns wider whose
    other columns hold NaN.  .v the CPU view, .ld its row stride, .on(dev) the same view of a device copy, .parent the whole matrix."""

    def __init__(self, t, strided=False):
        n, w = t.shape
        self.off, self.w = (4, w) if strided else (0, w)
        if strided:
            self.parent = torch.full((n, w + 8), NAN, dtype=F32)
            self.parent[:, 4:4 + w] = t
        else:
            self.parent = t.contiguous()
        self.v = self.parent[:, self.off:self.off + w]
        self.ld = self.parent.shape[1]

    def on(self, dev):
        return self.parent.to(dev)[:, self.off:self.off + self.w]


def linear_case(M, K, N, K1=None, strided=False, bias=True, res=False, seed=0, coherent=False):
    """X = [X1 | X2] (K1 None or K: one input), W 0.2 g, b g, R and dY row-scaled like X; strided: every row matrix a column slice of
    a wider NaN-holding one (the outputs' layout is the device test's business: it follows c['strided']).  coherent: X, dY >= 0 and
    every weight (1 + 2^-9) 2^j, j by output row: bf16 hi = 2^j, lo = 2^(j - 9) exactly, so the hi.lo products all have one sign and add
    up to 2^-9 of the entry's scale (with random signs they largely cancel: at K = 128 a kernel that lost them would sit at 2^-13.5 of
    scale, beside a bound of 2^-14)."""
    g = _gen(seed, M, K, N, K1 or K)
    K1 = K if K1 is None else K1
    X = scaled_rows(g, N, K, True)
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    if coherent:
        c = {'M': M, 'K': K, 'K1': K1, 'K2': K - K1, 'N': N, 'strided': strided,
             'X1': Operand(X[:, :K1].abs(), strided), 'X2': Operand(X[:, K1:].abs(), strided) if K1 < K else None,
             'W': ((1 + 2.0 ** -9) * 2.0 ** (torch.arange(M) % 5 - 2).to(F32))[:, None].repeat(1, K), 'b': f(M) if bias else None, 'R': None,
             'dY': Operand(scaled_rows(g, N, M, True).abs(), strided)}
        return c
    c = {'M': M, 'K': K, 'K1': K1, 'K2': K - K1, 'N': N, 'strided': strided,
         'X1': Operand(X[:, :K1], strided), 'X2': Operand(X[:, K1:], strided) if K1 < K else None,
         'W': 0.2 * f(M, K), 'b': f(M) if bias else None, 'R': Operand(scaled_rows(g, N, M), strided) if res else None,
         'dY': Operand(scaled_rows(g, N, M, True), strided)}
    return c


def linear_ref(c, dtype=F64, mm='exact', mutate=None, want_grad=True):
    v = lambda o: None if o is None else o.v       # noqa: E731
    return linear(v(c['X1']), v(c['X2']), c['W'], c['b'], v(c['R']), v(c['dY']) if want_grad else None, dtype, mm, mutate)


def pair_case(N, strided=False, bias=True, ghs=True, coherent=False, seed=0):
    """S, T [N][64], dST [N][128], gHS [N][64] (or None), every row of each its own power of ten, the last row 10^3 in all four (each
    is an operand of a sum over the rows; past the grid cap the 64 rows of tile 0 as well); Wl 64 x 128 and Wd 128 x 64 0.2 g, bl and bd g (or None).  strided: every row matrix a
    column slice of a wider NaN-holding one; the device test lays out its outputs, and the HS it hands to the backward, the same
    way.  coherent: as linear_case: rows >= 0 and every weight (1 + 2^-9) 2^j, j by output row."""
    g = _gen(seed, N, 6412864)
    # past the grid cap the rows of tile 0 are on top too: at cap_rows + 1 it is the one tile whose sums a workgroup carries into a
    # second visit, and with random scales its share of a sum over 32,769 rows is 1.6x the bound of dbl (measured: not 10x)
    top = TILE if N > cap_rows('linear_pair_bwd_x3', PAIR) else 0
    rows = lambda w: (lambda t: t.abs() if coherent else t)(scaled_rows(g, N, w, True, top))      # noqa: E731
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    coh = lambda M, K: ((1 + 2.0 ** -9) * 2.0 ** (torch.arange(M) % 5 - 2).to(F32))[:, None].repeat(1, K)      # noqa: E731
    S_, T_, dST, gHS = rows(64), rows(64), rows(128), rows(64)
    Wl, Wd, bl, bd = 0.2 * f(64, 128), 0.2 * f(128, 64), f(64), f(128)
    if coherent:
        Wl, Wd = coh(64, 128), coh(128, 64)
    return {'N': N, 'strided': strided, 'S': Operand(S_, strided), 'T': Operand(T_, strided), 'dST': Operand(dST, strided),
            'gHS': Operand(gHS, strided) if ghs else None, 'Wl': Wl, 'Wd': Wd, 'bl': bl if bias else None, 'bd': bd if bias else None}


def pair_ref(c, HS=None, dtype=F64, mm='exact', mutate=None, want_grad=True):
    return pair(c['S'].v, c['T'].v, c['Wl'], c['bl'], c['Wd'], c['bd'], c['dST'].v if want_grad else None,
                None if c['gHS'] is None else c['gHS'].v, HS, dtype, mm, mutate)


def pair_runs(c):
    """(float64 run, bf16x3-emulation run, tau per output) of a pair case, the backward's given HS the emulation's own forward
    result (float32 values, as the device's are) in both runs."""
    hs = pair_ref(c, None, F32, 'x3', want_grad=False)['HS']
    r64, rx3 = pair_ref(c, hs), pair_ref(c, hs, F32, 'x3')
    return r64, rx3, taus(r64, rx3, 'x3')


# The clauses of the two entries' MGV_CHECK_ARG lines (linear_x3.hip), one override of a valid call each: (entry, argument, value).
# Pointers: None.  ldghs is looked at only where gHS is given: the last two rows are ACCEPTED forms and are listed apart.
PAIR_REFUSALS = (
    [('mgv_linear_pair_fwd_x3', k, None) for k in ('S', 'T', 'wlpack_bf16', 'wdpack_bf16', 'HS', 'ST')]
    + [('mgv_linear_pair_fwd_x3', k, w) for k, lo in (('lds', 64), ('ldt', 64), ('ldhs', 64), ('ldst', 128)) for w in (lo - 4, lo + 2)]
    + [('mgv_linear_pair_fwd_x3', 'N', -1), ('mgv_linear_pair_bwd_x3', 'N', -1)]
    + [('mgv_linear_pair_bwd_x3', k, None) for k in ('dST', 'HS', 'S', 'T', 'wltpack_bf16', 'wdtpack_bf16', 'dS', 'dT', 'dWl', 'dWd')]
    + [('mgv_linear_pair_bwd_x3', k, w) for k, lo in (('lddst', 128), ('ldghs', 64), ('ldhs', 64), ('lds', 64), ('ldt', 64), ('ldds', 64), ('lddt', 64))
       for w in (lo - 4, lo + 2)])
PAIR_GHS_NULL_ACCEPTS = (60, 66, 0)      # ldghs with gHS NULL: not a fault


GROUPED_COUNTS = (64, 1, 63, 0, 64, 63, 1, 64, 0, 63, 64, 5)      # rows of the hand-built tiles (tile t: GROUPED_COUNTS[t % 12])


def grouped_case(M, K, ntiles=12, T=3, subset=False, bias=True, res=False, strided=False, seed=0):
    """Hand-built tables.  Tiles of 64, 1, 63 and 0 rows; `order` lists the tiles' nodes as a non-monotone permutation of a node range
    that leaves every fifth node (and 37 nodes at the end) out, with 3 unused entries between tiles (tile_start is not the running
    sum of the counts); slots 2, 0, 1, 2, ... (not sorted); per-slot weights 0.2 g (1 + s) and biases g + 10 s.  subset: tile_list names
    the tiles t % 3 != 1 in shuffled order (with the zero-count tiles among them)."""
    g = _gen(seed, M, K, ntiles, T, int(subset))
    counts = np.array([GROUPED_COUNTS[t % len(GROUPED_COUNTS)] for t in range(ntiles)])
    used = int(counts.sum())
    Nn = used + used // 4 + 38
    pool = np.array([n for n in range(Nn - 37) if n % 5 != 4])[:used]
    assert pool.size == used
    pool = g.permutation(pool)
    starts, order, pos = [], [], 0
    for t in range(ntiles):
        order += [0, 0, 0]                                    # entries no tile owns
        starts.append(len(order))
        order += pool[pos:pos + counts[t]].tolist()
        pos += counts[t]
    slot = np.array([(2 + t) % T for t in range(ntiles)])
    tl = None
    if subset:
        tl = g.permutation(np.array([t for t in range(ntiles) if t % 3 != 1]))
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))      # noqa: E731
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32))      # noqa: E731
    scale = torch.arange(1, T + 1, dtype=F32)
    return {'M': M, 'K': K, 'Nn': Nn, 'T': T, 'strided': strided,
            'tables': {'order': i32(order), 'tile_start': i32(starts), 'tile_count': i32(counts), 'tile_slot': i32(slot), 'tile_list': None if tl is None else i32(tl)},
            'X': Operand(scaled_rows(g, Nn, K), strided), 'W': 0.2 * f(T, M, K) * scale[:, None, None],
            'b': f(T, M) + 10 * (scale[:, None] - 1) if bias else None,
            'R': Operand(scaled_rows(g, Nn, M), strided) if res else None, 'dY': Operand(scaled_rows(g, Nn, M), strided)}


def grouped_ref(c, dtype=F64, mm='exact', mutate=None, fwd=True, wgrad=False):
    v = lambda o: None if o is None else o.v       # noqa: E731
    return grouped(c['X'].v, c['W'] if fwd else None, c['b'] if fwd else None, v(c['R']) if fwd else None, c['tables'], c['dY'].v if wgrad else None, dtype, mm, mutate)


DEGREES = (0, 1, 2, 3, 5, 64, 65)          # two neighbours are fetched ahead: 3 is the first degree with a tail loop
SEG_LENS = (0, 1, 2, 3, 64, 65)            # two members are in flight together
HUB = 600
FEW = 2048                                 # beyond this many lists the long ones (64, 65) are left out: the sizes past the grid cap stay small


def _lengths(n, ladder, hub_at):
    k = np.arange(n)
    short = len(ladder) - 2
    d = np.where(k < FEW, np.array(ladder)[k % len(ladder)], np.array(ladder)[k % short])
    if hub_at is not None and n > 0:
        d[min(hub_at, n - 1)] = HUB
    return d


def _csr(g, lengths, n_src):
    ptr = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=ptr[1:])
    idx = g.integers(0, n_src, max(int(ptr[-1]), 1))
    return torch.from_numpy(ptr.astype(np.int32)), torch.from_numpy(idx.astype(np.int32))


def list_case(H, N, seed=0):
    """mgv_gather_sum: list lengths DEGREES in turn (node 7 a HUB of 600), entries anywhere in an h of N + 11 rows."""
    g = _gen(seed, H, N, 1)
    ptr, idx = _csr(g, _lengths(N, DEGREES, 7), N + 11)
    return {'H': H, 'N': N, 'h': scaled_rows(g, N + 11, H), 'ptr': ptr, 'idx': idx}


def seg_case(H, n_seg, items=True, agg=True, out_row=True, seed=0):
    """mgv_seg_sum: segment lengths SEG_LENS in turn (segment 4 a HUB of 600 members), members any rows of `direct` (items) or the
    rows 0, 1, ... themselves (no items), neighbour lists of DEGREES in turn per direct row (row 3 a HUB), out_row a permutation of the
    segments into a matrix 7 rows longer (rows n_seg - 3 .. n_seg + 3 are skipped: they must stay untouched)."""
    g = _gen(seed, H, n_seg, 2)
    seg_ptr, _ = _csr(g, _lengths(n_seg, SEG_LENS, 4), 1)
    total = int(seg_ptr[-1])
    Rd = total + 5 if not items else max(total // 2, 1) + 5
    nptr, nidx = _csr(g, _lengths(Rd, DEGREES, 3), Rd + 3)
    rows = np.concatenate([np.arange(max(n_seg - 3, 0)), np.arange(n_seg + 4, n_seg + 7 + min(n_seg, 3))])[:n_seg]
    return {'H': H, 'n_seg': n_seg, 'n_out': n_seg + 7, 'seg_ptr': seg_ptr,
            'items': torch.from_numpy(g.integers(0, Rd, max(total, 1)).astype(np.int32)) if items else None,
            'direct': scaled_rows(g, Rd, H), 'agg': scaled_rows(g, Rd + 3, H) if agg else None, 'nbr_ptr': nptr if agg else None, 'nbr_idx': nidx if agg else None,
            'out_row': torch.from_numpy(g.permutation(rows).astype(np.int32)) if out_row else None}


def seg_ref(c, dtype=F64, mutate=None):
    return seg_sum(c['seg_ptr'], c['items'], c['direct'], c['agg'], c['nbr_ptr'], c['nbr_idx'], c['out_row'], dtype, mutate)


def class_case(H, N, C, agg=True, seed=0):
    """mgv_class_expand / mgv_class_pull_sum: classes at random with class C - 2 absent (C > 2: its sum must stay a0), table rows and
    gradient rows row-scaled, neighbour lists of DEGREES in turn (node 7 a HUB) into a gy_agg of N + 11 rows."""
    g = _gen(seed, H, N, C, 3)
    cls = g.integers(0, C, N)
    absent = C - 2 if C > 2 else -1
    cls[cls == absent] = C - 1
    ptr, idx = _csr(g, _lengths(N, DEGREES, 7), N + 11)
    return {'H': H, 'N': N, 'C': C, 'absent': absent, 'class_id': torch.from_numpy(cls.astype(np.int32)), 'table': scaled_rows(g, C, H),
            'gy_direct': scaled_rows(g, N, H), 'gy_agg': scaled_rows(g, N + 11, H) if agg else None, 'ptr': ptr if agg else None, 'idx': idx if agg else None}


def class_ref(c, dtype=F64, mutate=None):
    return class_pull_sum(c['gy_direct'], c['gy_agg'], c['ptr'], c['idx'], c['class_id'], c['C'], dtype, mutate)


def pull_sizes(H):
    """Row counts of mgv_class_pull_sum at which node0 + u stride crosses N for u = 1, 2, 3 (stride = cap_rows at a capped grid: N in
    (u stride, (u + 1) stride) leaves lane groups whose u-th row exists beside groups whose u-th row does not) and one past 4 strides
    (the outer loop's second pass)."""
    s = cap_rows('class_pull_sum', H)
    return [u * s + 5 * (THREADS // (H // 4)) + 3 for u in (1, 2, 3, 4)]
