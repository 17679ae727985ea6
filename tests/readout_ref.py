"""Plain restatements of the readout entries of csrc/readout.hip and csrc/readout_fused_x3.hip (with the fixed-order reduction of
csrc/mgv_slab.h behind them), working from exactly what the C ABI takes (include/mgvae_hip.h), plus the builders of the cases
tests/test_hip_readout_entries.py runs on the device.  CPU only; pinned to torch autograd, oracle/ref_cpu.py and fixture g1 by
tests/test_readout_spec.py, which also asserts the properties of the builders and shows that the planted defects are far outside the
device bounds.

  colstats(Y, ld, C, sums0)                                 sums0[c] + sum_i Y[i][c],  sums0[C + c] + sum_i Y[i][c]^2
  bn_act_fwd / bn_act_bwd / bn_bwd_apply                    A = f relu(bn), bn = (Y - mean) invstd gamma + beta, f the dropout factor of element
                                                            row C + col (oracle.ref_cpu.drop_factors); dZ = [bn > 0] dA f, sums0 + (sum dZ, sum dZ xhat);
                                                            dY = gamma invstd (dZ - [batch_stats] (s1 / N + (Y - mean) invstd s2 / N))
  head_fwd / head_bwd                                       h = A w + b, prob = clamp01 ? clamp(h, 0, 1) : h; dy = dprob [clamp01 ? 0 <= h <= 1 : 1],
                                                            dA = dy w, dw0 + sum dy A, db0 + sum dy
  l1_fwd / l1_bwd                                           sum0 + sum |x - t|;  dx = sign(x - t) gscale / n, sign(0) = 0
  fused_fwd_stages(case, given)                             every stage of mgv_readout_fused_fwd from what it reads: y1 from hf; stats1, rm1, rv1
                                                            from a GIVEN y1 (given['y1'], else its own); y2 from given y1 and stats1; and so on
  fused_bwd(case, y1, y2, stats, dprob)                     dhf and the ten gradient blocks in the order of mgv_readout_fused_grad_floats()

Arithmetic: dtype float64; dtype float32 is the stand-in for the kernels: float32 element by element, the float32 partial sums the
kernels form before their double totals (k_bn_act_bwd's four rows in flight, k_head's workgroup), and with mm = 'x3' every fused
Linear product through struct_stage_ref.mm3 (hi.hi + hi.lo + lo.hi of bf16 planes).  Every restatement takes mutate = (kind, ...):
ONE planted defect (tests/test_readout_spec.py), and dec = {...}: imposed ReLU / clamp decisions (see BAND).

Scales S (float64 without a defect): per ENTRY the sum of the magnitudes of the entry's own terms, carried forward through the chain
(the scale of bn is |Y - mean| invstd |gamma| + |beta|, of a product the product of the operands' scales, of a sum the sum).  An error
is judged against S of its own entry: struct_stage_ref.ratio.  The builders give every row its own power of ten from [-2, 2].

Bound of the device tests: tau = 8 max(r, floor) per output, r the worst ratio of the float32 / 'x3' run here against the float64 run
on the same case with the same decisions, floor the unit roundoff class of the output (FLOOR: 2^-23 for float32 element-wise work and
float32 partial sums, 2^-17 where a bf16x3 product is behind the entry; for mgv_colstats, whose sums are double from the first term on, 2^-53 chain_len).

Decisions.  ReLU (bn > 0) and clamp (0 <= h <= 1) are piecewise: an entry whose float64 pre-activation is closer than BAND to the
break may take either branch on the device and is compared on the branch the device took; everywhere else the decision is the float64
run's own.  The per-layer cases and the designed backward cases are nudged so that NO entry is inside the band; the stages behind a
device-made y1 / y2 cannot be, and the share of their banded entries is asserted (on the reference alone) to stay under
max(4, 1e-4 entries).  Entries designed to be exactly zero (the dead column, the zero dprob row, the L1 ties) are never banded."""
import numpy as np
import torch

from oracle.ref_cpu import drop_factors
from struct_stage_ref import F32, F64, mm3, ratio  # noqa: F401
from dense_ref import wpack  # noqa: F401

THREADS, TILE, U, CAP = 256, 64, 4, 2048
NAN = float('nan')
D, CF = 64, 32                       # readout_fused_x3.hip ro::D, ro::C
WIDTHS = (4, 8, 16, 32, 64)          # readout.hip c_ok
U24 = 2.0 ** -24
FLOOR = {'f32': 2.0 ** -23, 'x3': 2.0 ** -17}
# MEASURED (tests/test_readout_spec.py::test_band_is_eight_times_the_restatements_own_error, every builder case, float32 / 'x3' run
# against float64): worst absolute pre-activation error 8.0e-6 (ReLU inputs 3.0e-6, head outputs 8.0e-6) -> 8 x = 6.4e-5 -> 1e-4
BAND = 1e-4
BN_EPS, MOMENTUM = 1e-5, 0.1
GRAD_BLOCKS = (('dW1', CF * D), ('db1', CF), ('dgamma1', CF), ('dbeta1', CF), ('dW2', CF * CF), ('db2', CF), ('dgamma2', CF), ('dbeta2', CF),
               ('dw3', CF), ('db3', 1))          # readout_fused_x3.hip g_w1 .. g_b3


# ------------------------------------------------------------------------------------------------ launch geometry, restated
def rows_per_wg(C):
    return THREADS // (C // 4)


# kernel: (rows, or elements for l1, one workgroup takes per visit; grid cap; rows in flight per thread; the source line restated)
GEOMETRY = {
    'colstats': (rows_per_wg, 2048, 1, 'readout.hip mgv_colstats: rows = kThreads / (C / 4); grid_for(ceil(N / rows), 8)'),
    'bn_act_fwd': (rows_per_wg, 2048, 1, 'readout.hip ew_grid(N C / 4): 256 float4 = 256 / (C / 4) rows per workgroup; grid_for(.., 8)'),
    'bn_act_bwd': (rows_per_wg, 2048, 4, 'readout.hip mgv_bn_act_bwd: grid_for(ceil(N / rows), 8); k_bn_act_bwd U = 4'),
    'bn_bwd_apply': (rows_per_wg, 2048, 4, 'readout.hip ew_grid(N C / 4); k_bn_bwd_apply U = 4'),
    'head_fwd': (rows_per_wg, 2048, 1, 'readout.hip mgv_readout_head_fwd: grid_for(ceil(N / rows), 8)'),
    'head_bwd': (rows_per_wg, 2048, 1, 'readout.hip mgv_readout_head_bwd: grid_for(ceil(N / rows), 8)'),
    'l1_fwd': (lambda C: THREADS, 2048, 1, 'readout.hip ew_grid(n): 256 elements per workgroup; grid_for(.., 8)'),
    'l1_bwd': (lambda C: THREADS, 2048, 1, 'readout.hip ew_grid(n)'),
    'ro_fwd_lin': (lambda C: TILE, 1024, 1, 'readout_fused_x3.hip kGridF = 256 * 4; grid_tiles(N, kGridF)'),
    'ro_b3': (lambda C: TILE, 512, 1, 'readout_fused_x3.hip kGridB3 = 256 * 2'),
    'ro_db2': (lambda C: TILE, 1024, 1, 'readout_fused_x3.hip kGridDb2 = 256 * 4 (g2n of k_ro_b3)'),
    'ro_head': (lambda C: THREADS // (CF // 4), 2048, 1, 'readout_fused_x3.hip grid_rows(N): kGridS = 256 * 8, 32 rows'),
    'ro_b1': (lambda C: THREADS // (CF // 4), 2048, 4, 'readout_fused_x3.hip grid_rows(N); kU = 4'),
    'ro_b2': (lambda C: THREADS // (CF // 4), 2048, 4, 'readout_fused_x3.hip grid_rows(N); kU = 4'),
}


def unit(kernel, C=CF):
    return GEOMETRY[kernel][0](C)


def grid(kernel, N, C=CF):
    u = unit(kernel, C)
    return min(max((N + u - 1) // u, 1), GEOMETRY[kernel][1])


def cap_rows(kernel, C=CF):
    """The largest row count at which every workgroup makes one visit; from cap_rows + 1 on workgroup 0 comes round again."""
    return GEOMETRY[kernel][1] * unit(kernel, C)


def stride(kernel, N, C=CF):
    return grid(kernel, N, C) * unit(kernel, C)


def u_counts(kernel, N, C=CF):
    """(fewest, most) rows in range among the U = 4 a thread holds in flight, over the threads of the LAST outer pass that have any."""
    s = stride(kernel, N, C)
    rem = N - ((N - 1) // (U * s)) * U * s
    return min(U, -(-(rem - (min(s, rem) - 1)) // s)), min(U, -(-rem // s))


def partial_u(kernel, N, C=CF):
    """Some thread has a second row in flight and some thread has fewer than four: the guard `i0 + u stride < N` is true and false
    for u >= 1 inside one launch."""
    lo, hi = u_counts(kernel, N, C)
    return hi >= 2 and lo < U


def ws_doubles(N):
    """mgv_readout_fused_ws_doubles restated."""
    b3 = (grid('ro_b3', N) * (CF * D + CF) + grid('ro_db2', N) * (CF * CF + CF) + 1) // 2
    return max(grid('ro_fwd_lin', N) * 2 * CF, grid('ro_b1', N) * (3 * CF + 1), grid('ro_b2', N) * 2 * CF, b3)


def layer_sizes(C):
    r = rows_per_wg(C)
    s = [1, 2, r - 1, r, r + 1, 4099]
    if C in (4, 32, 64):
        s += [CAP * r, CAP * r + 1]
    if C in (4, 64):
        s.insert(-2, CAP * r - 1)              # the element kernels' last workgroup one float4 short of full
    if C == 32:
        s += [2 * CAP * r + 7, 4 * CAP * r + 5]
    return s


L1_SIZES = (1, 255, 256, 257, CAP * THREADS, CAP * THREADS + 1, 2 * CAP * THREADS + 3)
B3_SIZES = (512 * TILE, 512 * TILE + 1)
FUSED_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4099) + B3_SIZES + (1024 * TILE, 1024 * TILE + 1, 1024 * TILE + 128 * 3 + 5, 98305 + 64)


# ------------------------------------------------------------------------------------------------ arithmetic
def _mm(a, b, mm):
    return mm3(a, b) if mm == 'x3' else a @ b


def _factors(seed, N, C, p, dt, row4=False):
    """Dropout factors [N][C] of element row C + col; float32: the kernels' ks = 1.0f / (1.0f - p).  row4: the defect row 4 + col."""
    if not np.float32(p) > 0:
        return torch.ones(N, C, dtype=dt)
    if row4:
        flat = drop_factors(seed, 1, N * C, p)[0]
        f = flat[torch.arange(N)[:, None] * 4 + torch.arange(C)[None, :]]
    else:
        f = drop_factors(seed, N, C, p)
    if dt == F32:
        return (f != 0).to(F32) * float(np.float32(1) / (np.float32(1) - np.float32(p)))
    return f


def _keep_rows(N, kernel, C, mutate):
    """Row weights of the defects that lose rows from a sum: ('last_row',), ('lost_wg', b): the rows of workgroup b; ('lost_u', u): the
    rows the last outer pass reaches as its u-th in flight (-1: the last u any thread of that pass has); ('lost_visit', v): the rows of
    every workgroup's v-th grid-stride visit."""
    keep = torch.ones(N, dtype=torch.bool)
    kind = mutate[0] if mutate else None
    i = torch.arange(N)
    un, g = unit(kernel, C), grid(kernel, N, C)
    if kind == 'last_row':
        keep[N - 1] = False
    if kind == 'lost_wg':
        keep &= ((i // un) % g) != mutate[1]
    if kind == 'lost_visit':                   # the workgroups' mutate[1]-th grid-stride visit
        keep &= (i // (un * g)) != mutate[1]
    if kind == 'lost_u':
        s = un * g
        last = (N - 1) // (U * s)
        u = mutate[1] if mutate[1] >= 0 else (N - 1 - last * U * s) // s
        keep &= ~((i // (U * s) == last) & ((i // s) % U == u))
    return keep


def _colsum(T, kernel, C, dt, how):
    """Column sums of T [N][*] in double.  float64: one sum.  The float32 stand-in, how = 'u32': the U rows a thread holds in flight
    (one grid stride apart) meet in float32 first; 'wg32': a workgroup's rows meet in float32; 'f64': double, workgroup by workgroup."""
    N = T.shape[0]
    if dt == F64:
        return T.to(F64).sum(0)
    un, g = unit(kernel, C), grid(kernel, N, C)
    if how == 'u32':
        s = un * g
        P = -(-N // (U * s))
        pad = torch.zeros(P * U * s, T.shape[1], dtype=F32)
        pad[:N] = T
        pad = pad.view(P, U, s, -1)
        return (((pad[:, 0] + pad[:, 1]) + pad[:, 2]) + pad[:, 3]).to(F64).sum((0, 1))
    wg = (torch.arange(N) // un) % g
    part = torch.zeros(g, T.shape[1], dtype=F32 if how == 'wg32' else F64).index_add_(0, wg, T.to(F32 if how == 'wg32' else F64))
    return part.to(F64).sum(0)


def _tile_colsum32(T, kernel, dt):
    """Column sums of T [N][*] as B3 leaves db1 / db2: float64: one sum.  The float32 stand-in: a workgroup's rows (the tiles
    b, b + grid, ...) one after another in float32, then the workgroups' rows as k_slab_sum<float, float> adds them: 16 phases (rows
    ty, ty + 16, ...) one after another, then the phases.  (The kernel's chains inside a workgroup are shorter: a thread's few rows,
    then 32 threads in order.)"""
    if dt == F64:
        return T.to(F64).sum(0)
    N, g = T.shape[0], grid(kernel, T.shape[0])
    z = lambda n: torch.zeros(n, T.shape[1], dtype=F32)       # noqa: E731
    part = z(g).index_add_(0, (torch.arange(N) // TILE) % g, T.to(F32))
    ph = z(16).index_add_(0, torch.arange(g) % 16, part)
    return z(1).index_add_(0, torch.zeros(16, dtype=torch.long), ph)[0].to(F64)


def _out(res, S, dtype, mutate):
    res = {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in res.items()}
    if dtype == F64 and mutate is None:
        res['S'] = S
    return res


def colstats(Y, ld, C, sums0=None, dtype=F64, mutate=None):
    """Y: the [N][ld] matrix the entry is handed (its columns C .. ld are foreign).  Defects: last_row, lost_wg, ('ld_ignored',)."""
    N = Y.shape[0]
    kind = mutate[0] if mutate else None
    y = (Y.reshape(-1)[:N * C].reshape(N, C) if kind == 'ld_ignored' else Y[:, :C]).to(F64)
    y = y * _keep_rows(N, 'colstats', C, mutate)[:, None].to(F64)
    both = torch.cat([y, y * y], 1)
    s = _colsum(both, 'colstats', C, dtype, 'f64')
    a0 = torch.zeros(2 * C, dtype=F64) if sums0 is None else sums0.to(F64)
    return _out({'sums': a0 + s}, {'sums': both.abs().sum(0)}, dtype, mutate)


def _bn(Y, mean, invstd, gamma, beta, dt):
    cv = lambda t: t.to(dt)       # noqa: E731
    d = cv(Y) - cv(mean)
    xhat = d * cv(invstd)
    return d, xhat, xhat * cv(gamma) + cv(beta), d.abs().to(F64) * (invstd.to(F64) * gamma.to(F64)).abs() + beta.to(F64).abs()


def bn_act_fwd(Y, mean, invstd, gamma, beta, p, seed, dtype=F64, dec=None, mutate=None):
    """{'A', 'bn' (the pre-activation), 'relu' (this run's own decision)}.  Defects: ('mask_row4',), ('last_row',) (left unwritten: the NaN it was filled with)."""
    N, C = Y.shape
    kind = mutate[0] if mutate else None
    _, _, bn, Sbn = _bn(Y, mean, invstd, gamma, beta, dtype)
    f = _factors(seed, N, C, p, dtype, kind == 'mask_row4')
    gate = (bn > 0) if dec is None else dec['relu']
    A = bn * gate.to(dtype) * f
    if kind == 'last_row':
        A[N - 1] = NAN
    return _out({'A': A, 'bn': bn, 'relu': bn > 0}, {'A': Sbn * f.to(F64)}, dtype, mutate)


def bn_act_bwd(Y, mean, invstd, gamma, beta, p, seed, dA, sums0=None, dtype=F64, dec=None, mutate=None, kernel='bn_act_bwd'):
    """{'dZ', 'sums' = sums0 + [sum dZ | sum dZ xhat]}.  Defects: last_row, lost_wg, lost_u (rows lost from dZ and the sums),
    ('swap',) the two halves of sums exchanged, ('mask_row4',), ('gate_on_y',) the ReLU gate taken from Y > 0."""
    N, C = Y.shape
    kind = mutate[0] if mutate else None
    _, xhat, bn, _ = _bn(Y, mean, invstd, gamma, beta, dtype)
    f = _factors(seed, N, C, p, dtype, kind == 'mask_row4')
    gate = (bn > 0) if dec is None else dec['relu']
    if kind == 'gate_on_y':
        gate = Y > 0
    keep = _keep_rows(N, kernel, C, mutate)
    dz = dA.to(dtype) * f * gate.to(dtype) * keep[:, None].to(dtype)
    both = torch.cat([dz, dz * xhat], 1)
    s = _colsum(both, kernel, C, dtype, 'u32')
    dz = torch.where(keep[:, None], dz, torch.full_like(dz, NAN))          # a lost row stays the NaN it was filled with
    if kind == 'swap':
        s = torch.cat([s[C:], s[:C]])
    a0 = torch.zeros(2 * C, dtype=F64) if sums0 is None else sums0.to(F64)
    Sdz = (dA.to(F64) * f.to(F64)).abs()
    return _out({'dZ': dz, 'sums': a0 + s, 'relu': bn > 0}, {'dZ': Sdz, 'sums': torch.cat([Sdz, Sdz * xhat.to(F64).abs()], 1).sum(0)}, dtype, mutate)


def _bwd_factors(N, invstd, gamma, sums, batch_stats, dt, kind=None):
    """sc, a1, a2 of k_bn_bwd_apply / BnBwdQuad: a1 = float(sums / N), a2 = float(sums2 / N) invstd (the kernels' roundings in float32)."""
    C = invstd.numel()
    invn = 1.0 / N
    cv = lambda t: t.to(dt)       # noqa: E731
    sc = cv(gamma) * cv(invstd)
    on = batch_stats or kind == 'eval_keeps_correction'
    a1 = cv(sums[:C].to(F64) * invn) if on else torch.zeros(C, dtype=dt)
    a2 = cv(sums[C:].to(F64) * invn) * (1 if kind == 'no_invstd_a2' else cv(invstd)) if on else torch.zeros(C, dtype=dt)
    return sc, a1, a2


def bn_bwd_apply(Y, mean, invstd, gamma, dZ, sums, batch_stats, dtype=F64, mutate=None):
    """{'dY'}.  Defects: ('eval_keeps_correction',), ('no_invstd_a2',), last_row, lost_u (rows left unwritten: 0)."""
    N, C = Y.shape
    kind = mutate[0] if mutate else None
    sc, a1, a2 = _bwd_factors(N, invstd, gamma, sums, batch_stats, dtype, kind)
    d = Y.to(dtype) - mean.to(dtype)
    dY = sc * (dZ.to(dtype) - a1 - d * a2)
    dY = torch.where(_keep_rows(N, 'bn_bwd_apply', C, mutate)[:, None], dY, torch.full_like(dY, NAN))
    S = sc.to(F64).abs() * (dZ.to(F64).abs() + a1.to(F64).abs() + d.to(F64).abs() * a2.to(F64).abs())
    return _out({'dY': dY}, {'dY': S}, dtype, mutate)


def _head(A, w, b, dt, short=False):
    C = A.shape[1]
    n = C // 2 if short else C                      # the defect: the row sum over C / 8 lanes (the DPP ladder one step short)
    h = (A.to(dt)[:, :n] * w.to(dt)[:n]).sum(1) + b.to(dt)
    return h, A.to(F64).abs() @ w.to(F64).abs() + b.to(F64).abs()


def head_fwd(A, w, b, clamp01, dtype=F64, dec=None, mutate=None):
    """{'prob', 'h' (in front of the clamp), 'inside'}.  Defects: ('dpp_short',), ('last_row',)."""
    kind = mutate[0] if mutate else None
    h, S = _head(A, w, b, dtype, kind == 'dpp_short')
    prob = h
    if clamp01:
        prob = h.clamp(0, 1) if dec is None else torch.where(dec['inside'], h, (h > 0.5).to(dtype))
    if kind == 'last_row':
        prob = prob.clone()
        prob[-1] = NAN
    return _out({'prob': prob, 'h': h, 'inside': (h >= 0) & (h <= 1)}, {'prob': S}, dtype, mutate)


def head_bwd(A, w, b, clamp01, dprob, dw0=None, db0=None, dtype=F64, dec=None, mutate=None, kernel='head_bwd'):
    """{'dA', 'dw' = dw0 + sum dy A, 'db' = db0 + sum dy}.  Defects: ('clamp_open_above',) the gate open at h > 1, last_row, lost_wg,
    ('db_col',) db from the slab column in front of its own (the last column of dw), ('dpp_short',)."""
    N, C = A.shape
    kind = mutate[0] if mutate else None
    h, _ = _head(A, w, b, dtype, kind == 'dpp_short')
    inside = torch.ones(N, dtype=torch.bool)
    if clamp01:
        inside = ((h >= 0) & (h <= 1)) if dec is None else dec['inside']
        if kind == 'clamp_open_above':
            inside = h >= 0
    dy = dprob.to(dtype) * inside.to(dtype)
    dA = dy[:, None] * w.to(dtype)
    dys = dy * _keep_rows(N, kernel, C, mutate if kind != 'last_row' else None).to(dtype)
    if kind == 'last_row':
        dA[N - 1] = NAN
        dys = dys.clone()
        dys[N - 1] = 0
    both = torch.cat([dys[:, None] * A.to(dtype), dys[:, None]], 1)
    s = _colsum(both, kernel, C, dtype, 'wg32')
    dw, db = s[:C], s[C:]
    if kind == 'db_col':
        db = s[C - 1:C]
    dw = dw + (0 if dw0 is None else dw0.to(F64))
    db = db + (0 if db0 is None else db0.to(F64))
    ap = dprob.to(F64).abs()
    S = {'dA': ap[:, None] * w.to(F64).abs(), 'dw': (ap[:, None] * A.to(F64).abs()).sum(0), 'db': ap.sum()[None]}
    return _out({'dA': dA, 'dw': dw, 'db': db, 'inside': (h >= 0) & (h <= 1), 'h': h}, S, dtype, mutate)


def l1_fwd(x, t, sum0=0.0, dtype=F64, mutate=None):
    """sum0 + sum |x - t| (the kernel rounds each difference to float32 and adds in double).  Defects: last_row, lost_wg, lost_visit."""
    n = x.numel()
    d = (x.to(dtype) - t.to(dtype)).abs().to(F64) * _keep_rows(n, 'l1_fwd', 0, mutate).to(F64)
    wg = _colsum(d[:, None], 'l1_fwd', 0, dtype, 'f64')
    return _out({'sum': wg + sum0}, {'sum': (x.to(F64) - t.to(F64)).abs().sum()[None]}, dtype, mutate)


def l1_bwd(x, t, gscale, dtype=F64, mutate=None):
    """dx = sign(x - t) gscale / n with sign(0) = 0.  Defects: ('tie_positive',) sign(0) = 1, ('last_row',)."""
    n = x.numel()
    g = (torch.tensor(float(np.float32(gscale)), dtype=dtype) / torch.tensor(float(n), dtype=dtype))
    sg = torch.sign(x.to(F64) - t.to(F64))
    if mutate and mutate[0] == 'tie_positive':
        sg = torch.where(sg == 0, torch.ones_like(sg), sg)
    dx = sg.to(dtype) * g
    if mutate and mutate[0] == 'last_row':
        dx[n - 1] = NAN
    return _out({'dx': dx}, {'dx': torch.full((n,), abs(float(gscale)) / n, dtype=F64) * (sg != 0)}, dtype, mutate)


# ------------------------------------------------------------------------------------------------ the fused entries
def bn_finalize(N, sums, momentum, keep, eps, rm, rv, dtype=F64, mutate=None):
    """k_ro_bn_finalize from the double column sums [sum y | sum y^2]: mean, var = max(E[y^2] - mean^2, 0) in double; the running
    buffers take the UNBIASED variance var N / max(N - 1, 1) (N = 1: the factor is 1 and var is 0, so running_var only decays:
    running_var keep + momentum 0); running = running keep + momentum value; invstd = 1 / sqrt(var + eps).  float32: the kernel's roundings.
    Defects: ('biased_var',), ('swap_momentum_keep',)."""
    kind = mutate[0] if mutate else None
    C = sums.numel() // 2
    r = (lambda t: t.to(F32).to(F64)) if dtype == F32 else (lambda t: t)
    inv = 1.0 / N
    mean64 = sums[:C] * inv
    var64 = (sums[C:] * inv - mean64 * mean64).clamp(min=0)
    mean, var = r(mean64), r(var64)
    unb = r(var64 * (1.0 if kind == 'biased_var' else N / max(N - 1, 1)))
    q = (lambda v: float(np.float32(v))) if dtype == F32 else float       # the ABI takes momentum, keep, eps as float
    mo, ke = (q(keep), q(momentum)) if kind == 'swap_momentum_keep' else (q(momentum), q(keep))
    rm1 = r(r(rm.to(F64) * ke) + r(mo * mean))
    rv1 = r(r(rv.to(F64) * ke) + r(mo * unb))
    invstd = r(1.0 / torch.sqrt(r(var + q(eps))))
    return {'stats': torch.cat([mean, invstd]), 'rm': rm1, 'rv': rv1}


def _finalize_scales(N, ysum_abs, y2sum, momentum, keep, rm, rv, invstd):
    m = ysum_abs / N
    v = (y2sum / N + m * m) * (N / max(N - 1, 1))
    return {'stats': torch.cat([m, invstd.abs()]), 'rm': rm.to(F64).abs() * abs(keep) + abs(momentum) * m, 'rv': rv.to(F64).abs() * abs(keep) + abs(momentum) * v}


def fused_fwd_stages(c, given=None, dtype=F64, mm='exact', dec=None, mutate=None):
    """Every stage of mgv_readout_fused_fwd from what the stage reads.  given: {'y1', 'stats1', 'y2', 'stats2'} (float32, e.g. the
    device's own) stand in for this run's outputs of the earlier stages.  dec: {'relu1', 'relu2', 'inside'} imposed decisions.
    Defects: last_row (of y1, y2, prob), ('lost_wg', b) a workgroup's rows lost from the statistics, biased_var, swap_momentum_keep,
    ('mask1_for_2',) layer 1's mask (seed, p) used in layer 2, ('dpp_short',)."""
    assert mm == 'exact' or dtype == F32
    given, dec = given or {}, dec or {}
    kind = mutate[0] if mutate else None
    cv = lambda t: t.to(dtype)       # noqa: E731
    N = c['N']
    out, S = {}, {}

    def stat(y, k):
        yy = y.to(F64)
        yk = yy * _keep_rows(N, 'ro_fwd_lin', CF, mutate if kind == 'lost_wg' else None)[:, None].to(F64)
        sums = _colsum(torch.cat([yk, yk * yk], 1), 'ro_fwd_lin', CF, dtype, 'f64')
        f = bn_finalize(N, sums, c['momentum'], c['keep'], c['eps'], c['rm%d' % k], c['rv%d' % k], dtype, mutate)
        sc = _finalize_scales(N, yy.abs().sum(0), (yy * yy).sum(0), c['momentum'], c['keep'], c['rm%d' % k], c['rv%d' % k], f['stats'][CF:])
        for name in ('stats', 'rm', 'rv'):
            out['%s%d' % (name, k)], S['%s%d' % (name, k)] = f[name], sc[name]

    def act(y, stats, k):
        st = stats.to(F64)
        _, _, bn, Sbn = _bn(y, st[:CF], st[CF:], c['g%d' % k], c['be%d' % k], dtype)
        src = 1 if kind == 'mask1_for_2' else k
        f = _factors(c['seed%d' % src], N, CF, c['p%d' % src], dtype)
        gate = dec.get('relu%d' % k, bn > 0)
        out['bn%d' % k], out['relu%d' % k] = bn, bn > 0
        return bn * gate.to(dtype) * f, Sbn * f.to(F64)

    y1 = _mm(cv(c['hf']), cv(c['W1']).t(), mm) + cv(c['b1'])
    S['y1'] = c['hf'].to(F64).abs() @ c['W1'].to(F64).abs().t() + c['b1'].to(F64).abs()
    if kind == 'last_row':
        y1[N - 1] = NAN
    out['y1'] = y1
    y1 = given.get('y1', y1)
    stat(y1, 1)
    st1 = given.get('stats1', out['stats1'])
    a1, Sa1 = act(y1, st1, 1)
    y2 = _mm(a1, cv(c['W2']).t(), mm) + cv(c['b2'])
    S['y2'] = Sa1 @ c['W2'].to(F64).abs().t() + c['b2'].to(F64).abs()
    if kind == 'last_row':
        y2[N - 1] = NAN
    out['y2'] = y2
    y2 = given.get('y2', y2)
    stat(y2, 2)
    st2 = given.get('stats2', out['stats2'])
    a2, Sa2 = act(y2, st2, 2)
    hd = head_fwd(a2, c['w3'], c['b3'], c['clamp01'], dtype, dec if 'inside' in dec else None, mutate if kind in ('dpp_short', 'last_row') else None)
    out['prob'], out['h'], out['inside'] = hd['prob'], hd['h'], hd['inside']
    S['prob'] = Sa2 @ c['w3'].to(F64).abs() + c['b3'].to(F64).abs()
    return _out(out, S, dtype, mutate)


FWD_OUT = ('y1', 'stats1', 'rm1', 'rv1', 'y2', 'stats2', 'rm2', 'rv2', 'prob')
FWD_FLOOR = {'y1': 'x3', 'y2': 'x3', 'prob': 'f32', 'stats1': 'f32', 'rm1': 'f32', 'rv1': 'f32', 'stats2': 'f32', 'rm2': 'f32', 'rv2': 'f32'}
# dw3, db3, dgamma2, dbeta2 and dy2 (so db2) are formed without any bf16x3 product; dW2 and everything further back has one behind it
BWD_FLOOR = {'dhf': 'x3', 'dW1': 'x3', 'db1': 'x3', 'dgamma1': 'x3', 'dbeta1': 'x3', 'dW2': 'x3', 'db2': 'f32', 'dgamma2': 'f32', 'dbeta2': 'f32',
             'dw3': 'f32', 'db3': 'f32'}


def fused_bwd(c, y1, y2, stats, dprob, dtype=F64, mm='exact', dec=None, mutate=None):
    """mgv_readout_fused_bwd from exactly its arguments: {'dhf', the ten blocks of GRAD_BLOCKS, 'grads' (the blocks in order, flat)}.
    Defects: last_row; ('lost_wg', b) / ('lost_u', u) rows lost from B1's slab (dw3, db3, dgamma2, dbeta2 and the BN2 sums behind dy2);
    ('db_col',) db3 from the slab column in front of its own; ('swap',) dgamma2 / dbeta2 exchanged; ('mask1_for_2',);
    ('gate_on_y',); ('no_invstd_a2',); ('clamp_open_above',); ('dpp_short',); ('db2_g3n',) db2 from the tiles of B3's first set only."""
    assert mm == 'exact' or dtype == F32
    dec = dec or {}
    kind = mutate[0] if mutate else None
    cv = lambda t: t.to(dtype)       # noqa: E731
    N = c['N']
    st = stats.to(F64)
    f1 = _factors(c['seed1'], N, CF, c['p1'], dtype)
    f2 = f1 if kind == 'mask1_for_2' else _factors(c['seed2'], N, CF, c['p2'], dtype)
    d1, xh1, bn1, Sbn1 = _bn(y1, st[:CF], st[CF:2 * CF], c['g1'], c['be1'], dtype)
    d2, xh2, bn2, Sbn2 = _bn(y2, st[2 * CF:3 * CF], st[3 * CF:], c['g2'], c['be2'], dtype)
    gate1, gate2 = dec.get('relu1', bn1 > 0), dec.get('relu2', bn2 > 0)
    a1, a2 = bn1 * gate1.to(dtype) * f1, bn2 * gate2.to(dtype) * f2          # (the forward's activations: the gate_on_y defect is the backward's)
    if kind == 'gate_on_y':
        gate1, gate2 = y1 > 0, y2 > 0
    # B1: the head and the BN2 sums
    hb_mut = mutate if kind in ('last_row', 'lost_wg', 'lost_u', 'db_col', 'clamp_open_above', 'dpp_short') else None
    hb = head_bwd(a2, c['w3'], c['b3'], c['clamp01'], dprob, None, None, dtype, {'inside': dec['inside']} if 'inside' in dec else None, hb_mut, 'ro_b1')
    keep = _keep_rows(N, 'ro_b1', CF, mutate if kind in ('last_row', 'lost_wg', 'lost_u') else None)[:, None].to(dtype)
    dz2 = hb['dA'].to(dtype) * f2 * gate2.to(dtype)
    s2 = _colsum(torch.cat([dz2 * keep, dz2 * keep * xh2], 1), 'ro_b1', CF, dtype, 'u32')
    dw3, db3 = hb['dw'], hb['db']
    sc2, p21, p22 = _bwd_factors(N, st[3 * CF:], c['g2'], s2, True, dtype, kind)
    dy2 = sc2 * (dz2 - p21 - d2 * p22)
    # B2: the BN1 sums
    dA1 = _mm(dy2, cv(c['W2']), mm)
    dz1 = dA1 * f1 * gate1.to(dtype)
    s1 = _colsum(torch.cat([dz1, dz1 * xh1], 1), 'ro_b2', CF, dtype, 'u32')
    sc1, p11, p12 = _bwd_factors(N, st[CF:2 * CF], c['g1'], s1, True, dtype, kind)
    dy1 = sc1 * (dz1 - p11 - d1 * p12)
    # B3
    dy2b = dy2
    if kind == 'db2_g3n':
        g3n = grid('ro_b3', N)
        dy2b = dy2 * (((torch.arange(N) // TILE) // g3n) % 2 == 0)[:, None].to(dtype)
    out = {'dhf': _mm(dy1, cv(c['W1']), mm), 'dW1': _mm(dy1.t(), cv(c['hf']), mm), 'db1': _tile_colsum32(dy1, 'ro_b3', dtype), 'dgamma1': s1[CF:], 'dbeta1': s1[:CF],
           'dW2': _mm(dy2.t(), a1, mm), 'db2': _tile_colsum32(dy2b, 'ro_db2', dtype), 'dgamma2': s2[CF:], 'dbeta2': s2[:CF], 'dw3': dw3, 'db3': db3}
    if kind == 'swap':
        out['dgamma2'], out['dbeta2'] = out['dbeta2'], out['dgamma2']
    if kind == 'last_row':
        out['dhf'][N - 1] = NAN
    out['grads'] = torch.cat([out[k].to(F64).reshape(-1) for k, _ in GRAD_BLOCKS])
    out.update(bn1=bn1, bn2=bn2, h=hb['h'], relu1=bn1 > 0, relu2=bn2 > 0, inside=hb['inside'])
    S = None
    if dtype == F64 and mutate is None:
        A = lambda t: t.to(F64).abs()       # noqa: E731
        Sa1, Sa2 = Sbn1 * A(f1), Sbn2 * A(f2)
        Sdz2 = A(dprob)[:, None] * A(c['w3']) * A(f2)
        Ss2 = torch.cat([Sdz2, Sdz2 * A(xh2)], 1).sum(0)
        Sdy2 = A(sc2) * (Sdz2 + Ss2[:CF] / N + A(d2) * (Ss2[CF:] / N * A(st[3 * CF:])))
        SdA1 = Sdy2 @ A(c['W2'])
        Sdz1 = SdA1 * A(f1)
        Ss1 = torch.cat([Sdz1, Sdz1 * A(xh1)], 1).sum(0)
        Sdy1 = A(sc1) * (Sdz1 + Ss1[:CF] / N + A(d1) * (Ss1[CF:] / N * A(st[CF:2 * CF])))
        S = {'dhf': Sdy1 @ A(c['W1']), 'dW1': Sdy1.t() @ A(c['hf']), 'db1': Sdy1.sum(0), 'dgamma1': Ss1[CF:], 'dbeta1': Ss1[:CF],
             'dW2': Sdy2.t() @ Sa1, 'db2': Sdy2.sum(0), 'dgamma2': Ss2[CF:], 'dbeta2': Ss2[:CF], 'dw3': (A(dprob)[:, None] * Sa2).sum(0),
             'db3': A(dprob).sum()[None]}
    return _out(out, S, dtype, mutate)


def chain_len(kernel, N, C=CF):
    """L: the longest chain of sequential additions behind one entry of a double column sum: a thread's visits, the workgroup's lane
    groups (added in thread order), then k_slab_sum's phase (every 16th workgroup row) and its 16 phases.  The floor of such a sum is
    2^-53 L: the unit roundoff of the format it is accumulated in times the terms of its longest chain."""
    u, g = unit(kernel, C), grid(kernel, N, C)
    lanes = THREADS // (C // 4) if C else THREADS
    return -(-(-(-N // u)) // g) + lanes + -(-g // 16) + 16


def _floor(f):
    return FLOOR[f] if isinstance(f, str) else f


def taus(r64, rk, floors):
    """tau = 8 max(r, floor) per output (module docstring)."""
    return {k: 8 * max(ratio(rk[k], r64[k], S), _floor(floors[k] if isinstance(floors, dict) else floors)) for k, S in r64['S'].items() if k in rk}


def ratios(got, r64):
    return {k: ratio(got[k], r64[k], S) for k, S in r64['S'].items() if k in got}


def banded(pre, at=(0.0,)):
    """Entries of a float64 pre-activation closer than BAND to a break."""
    m = torch.zeros_like(pre, dtype=torch.bool)
    for a in at:
        m |= (pre - a).abs() < BAND
    return m


def band_cap(entries):
    return max(4, int(1e-4 * entries))


# ------------------------------------------------------------------------------------------------ cases
CONST_COL, ZERO_GAMMA_COL, DEAD_COL = 1, 2, 3          # present at every served width (C >= 4)


def _gen(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def scaled_rows(g, n, w, lo=-2, hi=2):
    """[n][w] float32 standard normal, every row times its own power of ten from [lo, hi]; the last row gets the top decade (the
    last row of a partial group is then among the largest terms of every sum over the rows)."""
    e = g.uniform(lo, hi, (n, 1))
    e[n - 1] = hi
    return torch.from_numpy((g.standard_normal((n, w)) * 10.0 ** e).astype(np.float32))


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _column_stats(Y, eps=BN_EPS):
    y = Y.to(F64)
    mean = y.mean(0)
    var = (y * y).mean(0) - mean * mean
    return mean.to(F32), (1.0 / torch.sqrt(var.clamp(min=0).to(F32).to(F64) + eps)).to(F32)


def _affine(g, C):
    gamma = _t(g.uniform(0.5, 1.5, C) * g.choice([-1.0, 1.0], C))
    beta = _t(g.uniform(1.0, 2.0, C) * g.choice([-1.0, 1.0], C))      # away from 0: the small-decade rows sit at bn = beta, outside the band
    gamma[ZERO_GAMMA_COL] = 0.0
    return gamma, beta


def _kill(Y, mean, invstd, gamma, beta):
    """beta[DEAD_COL] so far below zero that the column is negative behind the BatchNorm in every row, with half as much again to spare."""
    xhat = (Y[:, DEAD_COL].to(F64) - mean[DEAD_COL].to(F64)) * invstd[DEAD_COL].to(F64)
    gamma[DEAD_COL] = 0.5
    beta[DEAD_COL] = -float(np.ceil(0.75 * float(xhat.abs().max()) + 1.0))


def _nudge_relu(Y, mean, invstd, gamma, beta):
    """Move the entries of Y whose pre-activation is inside the band to 4 BAND away from 0 (same sign), where gamma != 0."""
    for _ in range(3):
        _, _, bn, _ = _bn(Y, mean, invstd, gamma, beta, F64)
        bad = banded(bn) & (gamma != 0)[None, :]
        if not bool(bad.any()):
            break
        want = torch.where(bn >= 0, 4 * BAND, -4 * BAND)
        y = ((want - beta.to(F64)) / (gamma.to(F64) * invstd.to(F64)) + mean.to(F64)).to(F32)
        Y = torch.where(bad, y, Y)
    return Y


def layer_case(C, N, seed=0, p=0.2, drop_seed=1234):
    """One BatchNorm + ReLU + Dropout block as the per-layer entries take it.  Y row-scaled; column CONST_COL constant (with the batch
    statistics handed in: xhat = 0, invstd = rsqrt(eps)); gamma[ZERO_GAMMA_COL] = 0; column DEAD_COL all negative behind the BatchNorm;
    mean / invstd the float32 batch statistics of Y (eps 1e-5); dA row-scaled with one row exactly 0; sums: designed double sums for
    mgv_bn_bwd_apply (of the columns' own magnitude, not the sums of this dA)."""
    g = _gen(seed, C, N, 11)
    Y = scaled_rows(g, N, C)
    Y[:, CONST_COL] = 3.0
    mean, invstd = _column_stats(Y)
    gamma, beta = _affine(g, C)
    _kill(Y, mean, invstd, gamma, beta)
    Y = _nudge_relu(Y, mean, invstd, gamma, beta)
    dA = scaled_rows(g, N, C)
    if N > 1:
        dA[N // 2] = 0.0
    sums = torch.from_numpy(g.standard_normal(2 * C)) * float(dA.abs().sum() / C) * 0.3
    return {'C': C, 'N': N, 'Y': Y, 'mean': mean, 'invstd': invstd, 'gamma': gamma, 'beta': beta, 'p': p, 'seed': drop_seed, 'dA': dA,
            'dZ': scaled_rows(g, N, C), 'sums': sums.to(F64)}


def head_case(C, N, seed=0):
    """A >= 0 row-scaled with a third of its entries 0 (what ReLU + Dropout leave), w 0.02 g, b = 0.3: the rows of the small decades
    sit inside (0, 1), the large ones on both sides; rows nudged out of the band round 0 and 1, the last row inside the clamp (its dprob is of the top decade: its loss shows in dw and db);
    dprob row-scaled, one row exactly 0."""
    g = _gen(seed, C, N, 12)
    A = scaled_rows(g, N, C).abs() * _t(g.uniform(0, 1, (N, C)) > 1 / 3)
    w, b = _t(0.02 * g.standard_normal(C)), _t([0.3])
    A[N - 1] = A[N - 1] * float(0.2 / max(float(A[N - 1].to(F64) @ w.to(F64).abs()), 1e-30))      # the last row inside the clamp: |A w| = 0.2 at most
    k = int(w.abs().argmax())
    for _ in range(3):
        h, _ = _head(A, w, b, F64)
        bad = banded(h, (0.0, 1.0))
        if not bool(bad.any()):
            break
        A[bad, k] = A[bad, k] + float(8 * BAND / abs(float(w[k])))        # A stays >= 0; h moves by 8 BAND
    dprob = scaled_rows(g, N, 1)[:, 0].contiguous()
    if N > 1:
        dprob[N // 2] = 0.0
    return {'C': C, 'N': N, 'A': A, 'w': w, 'b': b, 'dprob': dprob}


L1_MARKS = (THREADS, CAP * THREADS, 2 * CAP * THREADS)      # the first element of workgroup 1, of the second and of the third grid-stride visit


def l1_case(n, seed=0, ties=0.25):
    """x, t in [0, 1) at random; a quarter of the entries (every fourth) exact ties x == t.  The last element and the elements L1_MARKS
    are never ties and carry |x - t| of about 100, so the one element that makes a size an edge (the element behind a full workgroup,
    the first of a second visit) is 3e-4 of the sum or more even at a million elements: its loss shows far above the float32 floor."""
    g = _gen(seed, n, 13)
    x, t = _t(g.uniform(0, 1, n)), _t(g.uniform(0, 1, n))
    tie = torch.arange(n) % int(round(1 / ties)) == 1
    for i in sorted(set(L1_MARKS + (n - 1,))):
        if i < n:
            tie[i] = False
            x[i] = float(np.float32(100.0 + 50.0 * float(x[i])))
    t = torch.where(tie, x, t)
    return {'n': n, 'x': x, 't': t, 'tie': tie}


def fused_case(N, seed=0, p=(0.2, 0.5), seeds=(1234, 1234 + 7919), clamp01=1, momentum=MOMENTUM, keep=None, eps=BN_EPS):
    """The whole readout as mgv_readout_fused_fwd takes it.  hf row-scaled; W1 / W2 0.2 g with row CONST_COL zero (y1, y2 constant in
    that column: variance 0, invstd = rsqrt(eps)); gamma[ZERO_GAMMA_COL] = 0 and column DEAD_COL dead in both blocks; w3 0.6 g, b3 0.25;
    running buffers away from (0, 1); dprob row-scaled with one row exactly 0 (N > 1)."""
    g = _gen(seed, N, 14)
    n = lambda *s: _t(g.standard_normal(s))       # noqa: E731
    c = {'N': N, 'hf': scaled_rows(g, N, D), 'W1': 0.2 * n(CF, D), 'b1': 0.3 * n(CF), 'W2': 0.2 * n(CF, CF), 'b2': 0.3 * n(CF),
         'w3': 0.6 * n(CF), 'b3': _t([0.25]), 'p1': p[0], 'p2': p[1], 'seed1': seeds[0], 'seed2': seeds[1], 'clamp01': clamp01,
         'momentum': momentum, 'keep': 1.0 - momentum if keep is None else keep, 'eps': eps}
    for k in (1, 2):
        c['g%d' % k], c['be%d' % k] = _affine(g, CF)
        c['W%d' % k][CONST_COL] = 0.0
        c['rm%d' % k], c['rv%d' % k] = _t(g.uniform(-0.1, 0.1, CF)), _t(g.uniform(0.5, 1.5, CF))
    c['b1'][CONST_COL], c['b2'][CONST_COL] = 0.5, -0.25
    y = c['hf'].to(F64) @ c['W1'].to(F64).t() + c['b1'].to(F64)          # the dead columns need the float64 forward's own statistics
    for k in (1, 2):
        mean, invstd = _column_stats(y, eps)
        _kill(y, mean, invstd, c['g%d' % k], c['be%d' % k])
        if k == 1:
            _, _, bn, _ = _bn(y, mean, invstd, c['g1'], c['be1'], F64)
            y = (bn.clamp(min=0) * _factors(seeds[0], N, CF, p[0], F64)) @ c['W2'].to(F64).t() + c['b2'].to(F64)
    dprob = scaled_rows(g, N, 1)[:, 0].contiguous()
    if N > 1:
        dprob[N // 2] = 0.0
    c['dprob'] = dprob
    return c


def designed_bwd_inputs(c, seed=0):
    """y1, y2, stats for mgv_readout_fused_bwd that no forward produced: row-scaled y with the constant column, stats = the columns'
    float32 batch statistics with the mean moved by 0.1 / invstd and invstd times 1.1 (constant column: left alone); both y nudged out
    of the ReLU band and y2 moved where the head would sit inside the band round 0 or 1."""
    N = c['N']
    g = _gen(seed, N, 15)
    ys, st = [], []
    for k in (1, 2):
        y = scaled_rows(g, N, CF)
        y[:, CONST_COL] = 0.5
        mean, invstd = _column_stats(y)
        off = torch.ones(CF)
        off[CONST_COL] = 0.0
        mean, invstd = (mean + 0.1 * off / invstd).to(F32), (invstd * (1 + 0.1 * off)).to(F32)
        lim = float(c['be%d' % k][DEAD_COL].abs())              # the dead column stays dead: |xhat| <= |beta| there (gamma 0.5)
        y[:, DEAD_COL] = (mean[DEAD_COL] + ((y[:, DEAD_COL] - mean[DEAD_COL]) * invstd[DEAD_COL]).clamp(-lim, lim) / invstd[DEAD_COL]).to(F32)
        ys.append(_nudge_relu(y, mean, invstd, c['g%d' % k], c['be%d' % k]))
        st += [mean, invstd]
    stats = torch.cat(st)
    y2 = ys[1]
    special = (CONST_COL, ZERO_GAMMA_COL, DEAD_COL)
    f2 = _factors(c['seed2'], N, CF, c['p2'], F64)
    if N > 1:
        # the last row: every ordinary unit just open (bn2 = 0.01), so the head sits near b3 inside the clamp and the row's dprob (top
        # decade) reaches dz2, dy2 and db2: at 513 tiles the last row is all that B3's second set of workgroups holds
        for k in range(CF):
            if k not in special:
                y2[N - 1, k] = ((0.01 - c['be2'][k].to(F64)) / (c['g2'][k].to(F64) * stats[3 * CF + k].to(F64)) + stats[2 * CF + k].to(F64)).to(F32)
    for k in [int(k) for k in torch.argsort(-c['w3'].abs()) if int(k) not in special][:8]:
        _, _, bn2, _ = _bn(y2, stats[2 * CF:3 * CF], stats[3 * CF:], c['g2'], c['be2'], F64)
        h, _ = _head(bn2.clamp(min=0) * f2, c['w3'], c['b3'], F64)
        bad = banded(h, (0.0, 1.0)) if c['clamp01'] else torch.zeros(N, dtype=torch.bool)
        if not bool(bad.any()):
            break
        # unit k of the banded rows gets a pre-activation from [1, 2] (a dropped unit stays dropped: the next column is tried then)
        want = torch.from_numpy(g.uniform(1, 2, int(bad.sum())))
        y2[bad, k] = ((want - c['be2'][k].to(F64)) / (c['g2'][k].to(F64) * stats[3 * CF + k].to(F64)) + stats[2 * CF + k].to(F64)).to(F32)
    return ys[0], y2, stats
