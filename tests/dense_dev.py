"""Device-side buffers and the per-entry comparison shared by tests/test_hip_dense_reference.py and
tests/test_hip_linear_pair_reference.py: outputs with NaN guard rows (and NaN foreign columns where strided), NaN-filled workspaces
with a guard of their own, accumulator contents of each entry's own magnitude, and `compare`: err <= bound S entry by entry against a
float64 run of tests/dense_ref.py, an accumulator entry additionally 2^-24 |a0|, an entry nothing contributes to returned exactly."""
import torch

import dense_ref as DR

F64, F32, I32 = torch.float64, torch.float32, torch.int32
GUARD = 64
NAN = float('nan')
NANBITS = torch.tensor(NAN, dtype=F32).view(I32).item()


class Out:
    """An [n][w] output with GUARD rows behind it, contiguous or columns 4 .. 4 + w of a matrix 8 wider, NaN everywhere before the call."""

    def __init__(self, n, w, dev, strided=False, fill=None):
        self.n, self.w, self.off = n, w, 4 if strided else 0
        self.parent = torch.full((n + GUARD, w + (8 if strided else 0)), NAN, dtype=F32, device=dev)
        self.v = self.parent[:n, self.off:self.off + w]
        self.ld = self.parent.shape[1]
        if fill is not None:
            self.v.copy_(fill)

    def intact(self):
        """Guard rows and foreign columns bit-identical to the NaN they were filled with."""
        bits = self.parent.view(I32)
        mine = torch.zeros_like(bits, dtype=torch.bool)
        mine[:self.n, self.off:self.off + self.w] = True
        return bool((bits[~mine] == NANBITS).all())


def ws(nfloats, dev):
    return torch.full((nfloats + GUARD,), NAN, dtype=F32, device=dev)


def ws_intact(ws, nfloats):
    return bool((ws[nfloats:].view(I32) == NANBITS).all())


def a0(S, seed):
    """Random accumulator contents of each entry's own magnitude; standard normal where nothing contributes."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(S.shape, generator=g, dtype=F64) * 2 - 1
    return torch.where(S > 0, S * u, torch.randn(S.shape, generator=g, dtype=F64)).to(F32)


def bits(t):
    return t.detach().contiguous().view(I32).cpu()


def compare(prefix, derived, entry, tag, got, r64, tau, a0=None, chain=None):
    """Ratio err / S per output against its bound: tau, or max(tau, L 2^-24) for the (entry, output) pairs of `derived` with
    L = chain(output); prints one line `<prefix> <entry> <tag> | <output> ratio/bound | ...`, returns the violations."""
    a0 = a0 or {}
    line, bad = [], []
    for k, val in got.items():
        val = val.detach().cpu().to(F64)
        ref, S = r64[k], r64['S'][k]
        bound = max(tau[k], chain(k) * DR.U24) if (entry, k) in derived else tau[k]
        if k in a0:
            b = a0[k].to(F64)
            zero = S == 0
            if bool(zero.any()) and not torch.equal(val[zero].to(F32), a0[k][zero]):
                bad.append('%s: an entry nothing contributes to changed' % k)
            err = (((val - b) - ref).abs() - DR.U24 * b.abs()).clamp(min=0)
            r = float((err / S.clamp(min=1e-300))[~zero].max()) if bool((~zero).any()) else 0.0
            if not bool(torch.isfinite(val).all()):
                r = float('inf')
        else:
            r = DR.ratio(val, ref, S)
        line.append('%s %.2g/%.2g' % (k, r, bound))
        if not r <= bound:
            bad.append('%s: %.3g of its scale, bound %.3g' % (k, r, bound))
    print('%s %s %s | %s' % (prefix, entry, tag, ' | '.join(line)))
    return ['%s %s: %s' % (entry, tag, b) for b in bad]
