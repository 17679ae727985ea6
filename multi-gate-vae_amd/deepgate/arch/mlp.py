"""Readout MLP (reference: DG_VAE/deepgate/arch/mlp.py:14-56): [Linear, BatchNorm1d, ReLU, Dropout] x
(num_layer-1) + Linear.  Same `fc` Sequential layout, so state_dict keys match (fc.0, fc.1, fc.4, ...);
forward runs the MFMA Linear kernel and the fused BN/ReLU/Dropout and head kernels; in training mode the 64-32-32-1 readout of the
DG_AE models runs as one fused autograd node instead (ops.ReadoutMLPFn, csrc/readout_fused_x3.hip)."""
import os

import torch
import torch.nn as nn

from .. import ops

# MGV_FUSED_READOUT=0 keeps the per-layer path (linear / BnReluDropFn / HeadFn) for a same-process A/B: tests flip this flag
FUSED_READOUT = os.environ.get('MGV_FUSED_READOUT', '1') != '0'


class MLP(nn.Module):
    def __init__(self, dim_in=256, dim_hidden=32, dim_pred=1, num_layer=3, norm_layer=None, act_layer=None,
                 p_drop=0.5, sigmoid=False, tanh=False):
        super().__init__()
        assert num_layer >= 2, 'The number of layers shoud be larger or equal to 2.'
        if norm_layer != 'batchnorm' or act_layer != 'relu' or sigmoid or tanh or dim_pred != 1 or p_drop <= 0:
            raise NotImplementedError('the HIP readout implements Linear-BatchNorm1d-ReLU-Dropout blocks with a '
                                      'scalar output (the configuration the DG_AE models use)')
        fc = [nn.Linear(dim_in, dim_hidden), nn.BatchNorm1d(dim_hidden), nn.ReLU(inplace=True), nn.Dropout(p_drop)]
        for _ in range(num_layer - 2):
            fc += [nn.Linear(dim_hidden, dim_hidden), nn.BatchNorm1d(dim_hidden), nn.ReLU(inplace=True), nn.Dropout(p_drop)]
        fc.append(nn.Linear(dim_hidden, dim_pred))
        self.fc = nn.Sequential(*fc)
        self.num_blocks = num_layer - 1
        self._step = 0

    def _fused_ok(self, x):
        if not (FUSED_READOUT and self.training and x.is_cuda and ops.PRECISION == 'x3' and self.num_blocks == 2):
            return False
        if x.dim() != 2 or x.shape[0] == 0 or self.fc[0].weight.shape != (32, 64) or self.fc[4].weight.shape != (32, 32):
            return False
        bn1, bn2 = self.fc[1], self.fc[5]
        return (bn1.track_running_stats and bn2.track_running_stats and bn1.affine and bn2.affine and bn1.momentum is not None
                and bn1.momentum == bn2.momentum and bn1.eps == bn2.eps)

    def forward(self, x, clamp01=False, seed=None):
        """`seed` fixes the dropout masks (tests); by default one is drawn from torch's CPU generator."""
        if self._fused_ok(x):
            # the torch RNG and the BatchNorm counters are consumed / advanced exactly as in the per-layer loop below
            seeds = []
            for k in range(2):
                drop, bn = self.fc[4 * k + 3], self.fc[4 * k + 1]
                if drop.p > 0:
                    seeds.append(int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed) + 7919 * k)
                else:
                    seeds.append(0)
                bn.num_batches_tracked += 1
            l1, bn1, d1, l2, bn2, d2, last = (self.fc[i] for i in (0, 1, 3, 4, 5, 7, 8))
            return ops.ReadoutMLPFn.apply(x, l1.weight, l1.bias, bn1.weight, bn1.bias, l2.weight, l2.bias, bn2.weight, bn2.bias,
                                          last.weight, last.bias, bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var,
                                          d1.p, d2.p, seeds[0], seeds[1], bn1.momentum, bn1.eps, clamp01)
        y = x
        for k in range(self.num_blocks):
            lin, bn, drop = self.fc[4 * k], self.fc[4 * k + 1], self.fc[4 * k + 3]
            y = ops.linear(y, lin.weight, lin.bias)
            training = self.training
            if training and drop.p > 0:
                s = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed) + 7919 * k
            else:
                s = 0
            if training and bn.track_running_stats:
                bn.num_batches_tracked += 1
            y = ops.BnReluDropFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, training,
                                       drop.p, s, bn.momentum, bn.eps)
        last = self.fc[4 * self.num_blocks]
        return ops.HeadFn.apply(y, last.weight, last.bias, clamp01)
