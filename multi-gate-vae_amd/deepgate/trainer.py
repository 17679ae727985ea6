"""Trainer with the reference's surface (DG_VAE/deepgate/trainer.py:20-277): same constructor
arguments, `set_training_args`, `run_batch` -> {'recon_loss','pred_bin','gt_bin','prob_loss','func_loss'},
`train`, `save`, `load`, `resume`, same checkpoint dict.  Differences, all deliberate (SURVEY.md
Appendix B): gradients ARE averaged across ranks (one RCCL all-reduce of the flat gradient buffer per
step), only rank 0 writes checkpoints, step metrics come from four device-side counters instead of a
host copy of every edge prediction, and the dead N x N negative mask of the edge split is never built.
"""
import os
import sys
import time

import numpy as np
import torch
from torch import nn

from . import metrics, ops
from .data import CircuitBatch
from .digvae_model import DirectedGVAE
from .optim import FlatAdam
from .prefetch import BatchPrefetcher
from .step_branch import StepBranch
from .synthetic import collate as collate_arrays
from .utils.logger import Logger
from .utils.model_utils import load_model
from .utils.utils import AverageMeter


class GraphLoader:
    """Minimal stand-in for torch_geometric's DataLoader over a list of per-graph array dicts:
    drop_last batching, optional shuffling, DistributedSampler-style rank striding
    (trainer.py:178-195)."""

    def __init__(self, graphs, batch_size, shuffle, rank=0, world_size=1, seed=0):
        self.graphs, self.batch_size, self.shuffle = graphs, batch_size, shuffle
        self.rank, self.world_size, self.seed, self.epoch = rank, world_size, seed, 0

    def _indices(self):
        n = len(self.graphs)
        if self.shuffle or self.world_size > 1:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g).tolist() if self.shuffle else list(range(n))
        else:
            idx = list(range(n))
        if self.world_size > 1:
            total = (n + self.world_size - 1) // self.world_size * self.world_size
            idx = (idx + idx[:total - n])[self.rank:total:self.world_size]
        return idx

    def __len__(self):
        return len(self._indices()) // self.batch_size

    def chunks(self):
        """The epoch's batches as lists of per-graph array dicts (what a BatchPrefetcher collates on its worker threads)."""
        idx = self._indices()
        self.epoch += 1
        for b in range(len(idx) // self.batch_size):
            yield [self.graphs[i] for i in idx[b * self.batch_size:(b + 1) * self.batch_size]]

    def __iter__(self):
        for chunk in self.chunks():
            yield CircuitBatch.from_arrays(collate_arrays(chunk))


class Trainer():
    # the phase line of the reference's log (trainer.py:259-262); --val_auc appends ' |AUC: x.xxxx |AP: x.xxxx' to the val line,
    # --val_func_acc ' |FuncAcc: x.xxxx' behind it, --val_recovery ' |Recov: x.xxxx' behind that
    LOG_LINE = '{}| Epoch: {:}/{:} |Recon: {:.4f} |ACC: {:.2f} |Prob: {:.4f} |Func: {:.4f}|Net: {:.2f}s'

    def __init__(self, args, model, training_id='default', save_dir='./exp', lr=1e-4,
                 rc_prob_func_weight=[1.0, 4.0, 2.0], emb_dim=128, device='cpu', batch_size=32, num_workers=0,
                 distributed=True):
        super(Trainer, self).__init__()
        self.args = args
        self.emb_dim = emb_dim
        self.device = device
        self.lr = lr
        self.lr_step = -1
        self.rc_prob_func_weight = list(rc_prob_func_weight)
        # weight of the KL term of a variational model in the step's loss.  0.0 is the reference: KL is computed, reported under
        # 'kl_loss' and never added (trainer.py:145-148)
        self.kl_weight = float(getattr(args, 'kl_weight', 0.0) or 0.0)
        os.makedirs(save_dir, exist_ok=True)
        self.log_dir = os.path.join(save_dir, training_id)
        os.makedirs(self.log_dir, exist_ok=True)
        time_str = time.strftime('%Y-%m-%d-%H-%M')
        self.log_path = os.path.join(self.log_dir, 'log-{}.txt'.format(time_str))
        self.batch_size = batch_size
        self.num_workers = num_workers
        self.distributed = distributed
        self.local_rank, self.rank, self.world_size = 0, 0, 1
        if self.distributed:
            if 'LOCAL_RANK' in os.environ:
                self.local_rank = int(os.environ['LOCAL_RANK'])
            backend = os.environ.get('MGV_DIST_BACKEND', 'nccl')      # 'nccl' is RCCL on ROCm; 'gloo' = single-GPU rehearsal
            ndev = torch.cuda.device_count()
            if self.local_rank >= ndev and backend == 'nccl':
                raise RuntimeError('rank with LOCAL_RANK=%d but only %d GPU(s) visible: one rank per GPU '
                                   '(MGV_DIST_BACKEND=gloo stacks ranks on the visible GPUs for rehearsals)' % (self.local_rank, ndev))
            dev_index = self.local_rank % max(ndev, 1)
            self.device = 'cuda:%d' % dev_index
            torch.cuda.set_device(dev_index)
            if not torch.distributed.is_initialized():
                # rendezvous from the torchrun environment
                if backend == 'nccl':
                    torch.distributed.init_process_group(backend='nccl', init_method='env://', device_id=torch.device(self.device))
                else:
                    torch.distributed.init_process_group(backend=backend, init_method='env://')
            self.world_size = torch.distributed.get_world_size()
            self.rank = torch.distributed.get_rank()
            print('Training in distributed mode. Device {}, Process {:}, total {:}.'.format(self.device, self.rank, self.world_size), file=sys.stderr)
        else:
            print('Training in single device: ', self.device, file=sys.stderr)
        self.reg_loss = ops.l1_loss                     # nn.L1Loss() of the reference, on the HIP kernel
        self.model = model.to(self.device)
        # --neg_scope / --neg_reverse: which negatives the reconstruction loss draws (FunctionalModel.set_negative_sampling)
        self.neg_scope, self.neg_reverse = getattr(args, 'neg_scope', 'batch'), float(getattr(args, 'neg_reverse', 0.0))
        if (self.neg_scope, self.neg_reverse) != ('batch', 0.0):
            if not hasattr(self.model, 'set_negative_sampling'):
                raise ValueError('--neg_scope / --neg_reverse: %s draws its negatives over the whole batch only' % type(self.model).__name__)
            self.model.set_negative_sampling(self.neg_scope, self.neg_reverse)
        self.optimizer = FlatAdam(self.model.parameters(), lr=self.lr)
        if self.world_size > 1:
            for p in self.model.parameters():           # every rank starts from rank 0's weights
                torch.distributed.broadcast(p.data, 0)
            for b in self.model.buffers():
                torch.distributed.broadcast(b.data, 0)
        self.model_epoch = 0
        self.overlap = True          # run the reconstruction branch on a second stream (step_branch.StepBranch)
        self.side_stream = None      # that stream: created at the first overlapped step; set one before it to choose it (a priority stream)
        self._branch = None          # the current step's StepBranch, from run_batch until train_step has joined its backward
        if self.local_rank == 0:
            self.logger = Logger(self.log_path)

    def set_training_args(self, rc_prob_func_weight=[], lr=-1, lr_step=-1, device='null'):
        if len(rc_prob_func_weight) == 3 and list(rc_prob_func_weight) != self.rc_prob_func_weight:
            print('[INFO] Update rc_prob_func_weight from {} to {}'.format(self.rc_prob_func_weight, rc_prob_func_weight))
            self.rc_prob_func_weight = list(rc_prob_func_weight)
        if lr > 0 and lr != self.lr:
            print('[INFO] Update learning rate from {} to {}'.format(self.lr, lr))
            self.lr = lr
            for param_group in self.optimizer.param_groups:
                param_group['lr'] = self.lr
        if lr_step > 0 and lr_step != self.lr_step:
            print('[INFO] Update learning rate step from {} to {}'.format(self.lr_step, lr_step))
            self.lr_step = lr_step
        if device != 'null' and device != self.device:
            print('[INFO] Update device from {} to {}'.format(self.device, device))
            self.device = device
            self.model = self.model.to(self.device)

    def save(self, path):
        torch.save({'epoch': self.model_epoch, 'state_dict': self.model.state_dict(),
                    'optimizer': self.optimizer.state_dict()}, path)

    def load(self, path):
        checkpoint = torch.load(path, map_location='cpu')
        self.optimizer.load_state_dict(checkpoint['optimizer'])
        for param_group in self.optimizer.param_groups:
            self.lr = param_group['lr']
        self.model_epoch = checkpoint['epoch']
        self.model.load(path)
        print('[INFO] Continue training from epoch {:}'.format(self.model_epoch))
        return path

    def resume(self):
        model_path = os.path.join(self.log_dir, 'model_last.pth')
        if os.path.exists(model_path):
            self.model, self.optimizer, self.model_epoch = load_model(self.model, model_path, optimizer=self.optimizer,
                                                                      local_rank=self.local_rank, device=self.device)
            return True
        return False

    def run_batch(self, batch, want_pred=True, want_rank=False, want_func_acc=False, want_recovery=False):
        """Forward + the three losses (trainer.py:131-174).  `general_train_test_split_edges` with zero
        val/test ratios only permutes the edges (preprocessing.py:41-50), to which the mean over edges is
        invariant: train_pos_edge_index is the batch's edge_index.  `want_rank`: also rank the loss's own pairs on the device
        (ROC-AUC / average precision, ops.link_record); the record is returned under 'link_metrics'.  `want_func_acc`: also count
        every comparison of two listed truth-table pairs per circuit at gap 0.05 (ops.function_accuracy); the int64 [G, 3] counts
        {eligible, concordant, tied} are returned under 'func_counts', on the device.  `want_recovery`: also decode hs into a legal
        circuit and count the gates whose whole fan-in set came back (Model.circuit_recovery); the int64 [G, 2] counts {gates, exact}
        are returned under 'recovery_counts', on the device."""
        batch.train_pos_edge_index = batch.edge_index
        neg = getattr(batch, 'neg_edge_index', None)
        # the batch's plan is Model.forward's to build and to pass (every batch has one from there on: the device sampler draws).
        # expect_scale: weighted_loss(...).backward() brings the reconstruction loss exactly its weight as upstream gradient;
        # graph_ptr: the batch's graph table, for a model that draws its negatives inside each circuit (set_negative_sampling)
        recon = dict(pos_edge_index=batch.train_pos_edge_index, neg_edge_index=neg, want_pred=want_pred, want_rank=want_rank,
                     expect_scale=self.rc_prob_func_weight[0], graph_ptr=getattr(batch, 'graph_ptr', None))
        self._branch = None
        if self.overlap and next(self.model.parameters()).is_cuda:
            if self.side_stream is None:
                self.side_stream = torch.cuda.Stream()
            self._branch = StepBranch(self.side_stream, **recon)
            hs, hf = self.model(batch, branch=self._branch)
            loss, pred_bin, gt_bin = self._branch.take(self.model)
        else:
            hs, hf = self.model(batch)
            loss, pred_bin, gt_bin = self.model.recon_loss(hs, plan=batch._mgv_plan, **recon)
        loss_status = {'recon_loss': loss, 'pred_bin': pred_bin, 'gt_bin': gt_bin}
        if getattr(self.model, 'variational', False) or ('VAE' in getattr(self.args, 'model', '') and isinstance(self.model, DirectedGVAE)):
            s_kl, t_kl = self.model.kl_loss()
            loss_status['kl_loss'] = s_kl + t_kl          # computed; added only under a positive kl_weight (weighted_loss)
        # hf has two consumers (trainer.py:155-163): the function loss first, the readout on the hf it passes through, so that the
        # two gradients meet inside the function-loss backward kernel
        loss_status['func_loss'], hf_r = ops.func_loss_passthrough(hf, batch['tt_pair_index'], batch['tt_sim'], cache=batch)
        prob = self.model.pred_prob(hf_r)
        loss_status['prob_loss'] = self.reg_loss(prob, batch['prob'])
        loss_status['confusion'] = self.model.last_confusion
        if want_rank:
            loss_status['link_metrics'] = self.model.last_link_metrics
        if want_func_acc:
            loss_status['func_counts'] = metrics.function_accuracy(hf, batch['tt_pair_index'], batch['tt_sim'],
                                                                   graph_ptr=getattr(batch, 'graph_ptr', None), cache=batch)[1][:, 0]
        if want_recovery:
            loss_status['recovery_counts'] = self.model.circuit_recovery(hs, batch)[0].counts[:, :2]
        return loss_status

    def _encoder_half_rounds(self):
        """2 x rounds of the model's two structural encoders (what GraphPlan.quotient is asked for; a list), 8 when it cannot be told.
        An encoder whose halves exist and have no rounds (the DiGAE baseline, DirectedGCNConvEncoder) has none: an empty list, and
        the prefetcher then prepares neither colour classes nor first-stage tables."""
        enc = getattr(self.model, getattr(self.model, 'ENCODER_ATTR', 'struct_encoder'), None)
        halves = [getattr(enc, a, None) for a in ('source_conv', 'target_conv')]
        counts = {2 * int(getattr(h, 'num_rounds', 4)) for h in halves if h is None or hasattr(h, 'num_rounds')}
        return sorted(counts)                # --s_rounds and --t_rounds may differ: both encoders' stage counts are warmed

    def weighted_loss(self, loss_status):
        w = self.rc_prob_func_weight
        loss = w[0] * loss_status['recon_loss'] + w[1] * loss_status['prob_loss'] + w[2] * loss_status['func_loss']
        if self.kl_weight > 0 and 'kl_loss' in loss_status:
            loss = loss + self.kl_weight * loss_status['kl_loss']
        return loss

    def train_step(self, batch, want_pred=False):
        """zero_grad -> run_batch -> weighted loss -> backward -> (all-reduce) Adam (trainer.py:222-234)."""
        self.optimizer.zero_grad()
        loss_status = self.run_batch(batch, want_pred=want_pred)
        loss = self.weighted_loss(loss_status)
        loss.backward()
        branch, self._branch = self._branch, None
        if branch is not None:
            branch.join()            # backward work queued on the second stream
        self.optimizer.step()
        return loss_status

    # ---- per-step metrics read-back (trainer.py:236-244: three losses + the confusion counters), one step behind -------------
    def enqueue_metrics(self, loss_status):
        """Start the host copy of this step's 7 metrics (3 losses, TP/FP/TN/FN) into pinned memory and return the PREVIOUS
        step's values (None at the first call): the host never waits for the step it has just enqueued, so the next step's
        launches are already queued when the GPU finishes this one.  `flush_metrics()` returns the last step's values.
        A step that has a 'kl_loss' (variational model) carries it in an eighth slot."""
        vals = torch.cat([torch.stack([loss_status['recon_loss'].detach(), loss_status['prob_loss'].detach(),
                                       loss_status['func_loss'].detach()]).double(), loss_status['confusion'].double()])
        if 'kl_loss' in loss_status:
            vals = torch.cat([vals, loss_status['kl_loss'].detach().double().reshape(1)])
        if not vals.is_cuda:
            prev, self._m_last = getattr(self, '_m_last', None), vals.tolist()
            return prev
        if getattr(self, '_m_buf', None) is None or self._m_buf.shape[1] != vals.numel():
            self._m_buf = torch.empty(2, vals.numel(), dtype=torch.float64).pin_memory()
            self._m_ev = [None, None]
            self._m_n = 0
        slot = self._m_n % 2
        prev = self._take_metrics(1 - slot)
        self._m_buf[slot].copy_(vals, non_blocking=True)
        self._m_ev[slot] = torch.cuda.Event()
        self._m_ev[slot].record()
        self._m_n += 1
        return prev

    def _take_metrics(self, slot):
        ev = self._m_ev[slot]
        if ev is None:
            return None
        ev.synchronize()
        self._m_ev[slot] = None
        return self._m_buf[slot].tolist()

    def flush_metrics(self):
        if getattr(self, '_m_buf', None) is None:
            prev, self._m_last = getattr(self, '_m_last', None), None
            return prev
        return self._take_metrics((self._m_n - 1) % 2)

    def _loader(self, dataset, shuffle):
        if isinstance(dataset, GraphLoader):
            return dataset
        return GraphLoader(dataset, self.batch_size, shuffle, self.rank, self.world_size)

    def train(self, num_epoch, train_dataset, val_dataset):
        train_loader = self._loader(train_dataset, shuffle=not self.distributed)
        val_loader = self._loader(val_dataset, shuffle=not self.distributed)
        batch_time = AverageMeter()
        stats = {k: AverageMeter() for k in ('recon', 'prob', 'func', 'acc', 'tp', 'fp', 'tn', 'fn', 'kl')}
        print('[INFO] Start training, lr = {:.4f}'.format(self.optimizer.param_groups[0]['lr']))

        def account(vals):
            if vals is None:
                return
            tot = max(sum(vals[3:7]), 1.0)
            tp, fp, tn, fn = (v / tot for v in vals[3:7])
            if len(vals) > 7:
                stats['kl'].update(vals[7])
            for k, v in zip(('recon', 'prob', 'func', 'acc', 'tp', 'fp', 'tn', 'fn'),
                            (vals[0], vals[1], vals[2], tp + tn, tp, fp, tn, fn)):
                stats[k].update(v)

        val_auc = bool(getattr(self.args, 'val_auc', False))
        val_func_acc = bool(getattr(self.args, 'val_func_acc', False))
        val_recovery = bool(getattr(self.args, 'val_recovery', False))
        for epoch in range(num_epoch):
            for phase in ['train', 'val']:
                rank = val_auc and phase == 'val'
                facc = val_func_acc and phase == 'val'
                recov = val_recovery and phase == 'val'
                records = []             # per-batch link records of the phase, on the device until the phase ends
                func_counts = []         # per-batch [G, 3] comparison counts of the phase, likewise
                recovery_counts = []     # per-batch [G, 2] {gates, exact} of the phase, likewise
                loader = train_loader if phase == 'train' else val_loader
                self.model.train() if phase == 'train' else self.model.eval()
                # collate, host-to-device copy and plan build of the next batches run on worker threads / their own HIP streams
                # beside the current step (deepgate/prefetch.py); the reference does `batch.to(device)` inside the loop (trainer.py:223)
                batches = BatchPrefetcher(loader.chunks(), self.device, gate_ids=[g for _, g in getattr(self.model, 'GATES', [])] or None,
                                          workers=max(self.num_workers, 2), quotient_stages=self._encoder_half_rounds(),
                                          graph_table=self.neg_scope == 'graph')
                try:
                    for iter_id, batch in enumerate(batches):
                        time_stamp = time.time()
                        if phase == 'train':
                            loss_status = self.train_step(batch)
                        else:
                            with torch.no_grad():
                                loss_status = self.run_batch(batch, want_pred=False, **({'want_rank': True} if rank else {}),
                                                             **({'want_func_acc': True} if facc else {}),
                                                             **({'want_recovery': True} if recov else {}))
                            if rank:
                                records.append(loss_status['link_metrics'])
                            if facc:
                                func_counts.append(loss_status['func_counts'])
                            if recov:
                                recovery_counts.append(loss_status['recovery_counts'])
                        # one small device->host copy per step (3 losses + 4 counters), read one step behind so that the host
                        # never waits for the step it has just enqueued
                        account(self.enqueue_metrics(loss_status))
                        batch_time.update(time.time() - time_stamp)
                    account(self.flush_metrics())
                finally:
                    batches.close()          # also when a step raises: worker threads, pinned staging and in-flight batches go
                if phase == 'train' and self.model_epoch % 10 == 0 and self.rank == 0:
                    self.save(os.path.join(self.log_dir, 'model_{:}.pth'.format(self.model_epoch)))
                    self.save(os.path.join(self.log_dir, 'model_last.pth'))
                rank_cols = ''
                if rank:
                    # one host read for the whole phase; raises if a batch ranked a NaN score
                    pairs = metrics.read_link_records(records)
                    if pairs:
                        rank_cols = ' |AUC: {:.4f} |AP: {:.4f}'.format(sum(a for a, _ in pairs) / len(pairs), sum(b for _, b in pairs) / len(pairs))
                if facc and func_counts:
                    # one host read for the whole phase: the mean of concordant / eligible over the circuits that have a comparison
                    c = torch.cat(func_counts).cpu()
                    c = c[c[:, 0] > 0].double()
                    if c.shape[0] > 0:
                        rank_cols += ' |FuncAcc: {:.4f}'.format(float((c[:, 1] / c[:, 0]).mean()))
                if recov and recovery_counts:
                    # one host read for the whole phase: the mean of exact / gates over the circuits that have a gate
                    c = torch.cat(recovery_counts).cpu()
                    c = c[c[:, 0] > 0].double()
                    if c.shape[0] > 0:
                        rank_cols += ' |Recov: {:.4f}'.format(float((c[:, 1] / c[:, 0]).mean()))
                if getattr(self.model, 'variational', False):
                    rank_cols = ' |KL: {:.4f}'.format(stats['kl'].avg) + rank_cols
                if self.local_rank == 0:
                    line = self.LOG_LINE.format(phase, epoch, num_epoch, stats['recon'].avg, stats['acc'].avg * 100, stats['prob'].avg,
                                                stats['func'].avg, batch_time.avg) + rank_cols + '\n'
                    self.logger.write(line)
                    print(line, end='')
            self.model_epoch += 1
            if self.lr_step > 0 and self.model_epoch % self.lr_step == 0:
                self.lr *= 0.1
                if self.local_rank == 0:
                    print('[INFO] Learning rate decay to {}'.format(self.lr))
                for param_group in self.optimizer.param_groups:
                    param_group['lr'] = self.lr
