"""The reconstruction branch of ONE training step on a second HIP stream: everything the step's two streams tell
each other, for the lifetime of that step.  Trainer.run_batch creates one when it overlaps and hands it to Model.forward."""
import torch


class _BeforeBackward(torch.autograd.Function):
    """Identity on x whose backward calls fn() first: fn runs just before the backward of the node that made x, on x's stream."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


class StepBranch:
    def __init__(self, side, **recon_args):
        self.side, self.main = side, torch.cuda.current_stream()
        self.recon_args = recon_args          # Model.recon_loss's arguments behind hs
        self.result = None                    # (loss, pred_bin, gt_bin) between `took` and `take`
        self._sweep_bwd = None                # event, main -> side: the round-1 sweep backward has begun

    def fork(self, hs):
        """Context in which Model.forward runs the branch: the side stream, started behind everything enqueued so far (hs exists)."""
        self.side.wait_stream(self.main)
        hs.record_stream(self.side)
        return torch.cuda.stream(self.side)

    def took(self, loss, pred_bin, gt_bin, hs_pass):
        """Inside `fork`: keep recon_loss's result; its backward is to wait for the sweep's.  Returns the hs the sweep consumes."""
        if loss.requires_grad:
            loss = _BeforeBackward.apply(loss, self._wait_sweep_bwd)
        self.result = (loss, pred_bin, gt_bin)
        return hs_pass

    def sweep_out(self, hf):
        """The round-1 sweep's output, marked: its backward is the start signal of the branch's."""
        return _BeforeBackward.apply(hf, self._record_sweep_bwd) if hf.requires_grad else hf

    def _record_sweep_bwd(self):
        self._sweep_bwd = torch.cuda.Event()
        self._sweep_bwd.record()

    def _wait_sweep_bwd(self):
        if self._sweep_bwd is not None:
            torch.cuda.current_stream().wait_event(self._sweep_bwd)
            self._sweep_bwd = None

    def join(self):
        """side -> main: after the forward (through `take`) and again after backward."""
        self.main.wait_stream(self.side)

    def take(self, model):
        """Join, and hand over (loss, pred_bin, gt_bin): these and the model's result tensors (of a variational model also its KL sums)
        were allocated on the side stream and are read on the main one from here on."""
        self.join()
        out, self.result = self.result, None      # this object must not keep the step's loss graph alive (its nodes hold it)
        for t in (*out, model.last_confusion, model.last_link_metrics, getattr(model, '_klsum', None)):
            if t is not None:
                t.record_stream(self.main)
        return out
