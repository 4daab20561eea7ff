"""Fused relativistic-average GAN iteration of ESRGAN -- ESRGAN/train_esrgan.py:340-431 on the HIP engines.

Order and arithmetic of the reference's loop body:
  generator (discriminator frozen, :361-392): sr = G(lr); gt_out = D(gt); sr_out = D(sr); pixel = w_p * L1(sr, gt);
    content = w_c * L1(vgg(sr)[node], vgg(gt)[node]) (differentiable, one node); adversarial = w_a * 0.5 * (BCE(gt_out - mean(sr_out), 0)
    + BCE(sr_out - mean(gt_out), 1)); backward of the sum into the generator only -- through D's data gradient with BOTH halves of the
    adversarial term reaching sr_out (the first through the mean) -- Adam step, EMA update;
  discriminator (:394-425): gt_out = D(gt); sr_out = D(sr.detach()); 0.5 * BCE(gt_out - mean(sr_out), 1) backward (retain_graph);
    sr_out = D(sr.detach()) again; 0.5 * BCE(sr_out - mean(gt_out), 0) backward; Adam step.
Five training-mode discriminator forwards per iteration (BatchNorm running statistics advance five times, as in the reference).
The two discriminator losses are back-propagated as TWO passes instead of the reference's four graph traversals: the second and third
forwards of sr.detach() are the same function of the same inputs, so the gradients that reach D through them add up to one pass through
the last one with the summed seeds (d loss_gt / d mean(sr_out) + d loss_sr / d sr_out), and likewise for the gt forward.
Every loss, seed, reduction and optimizer step is a HIP kernel (srganfd_l1_loss, srganfd_bce_logits_relativistic, the engines'
convolutions, srganfd_adam_ema); nothing runs as an ATen op.  Mixed precision: trainer.LossScaler, one instance for both networks (:103).
"""
from __future__ import annotations

from typing import Optional

from torch import Tensor

from . import _abi as A
from .engine import _engine, generator_engine
from .engine_e import esrgan_discriminator_engine
from .engine_v import ContentLossGradEngine
from .trainer import FlatAdamEMA, FusedTrainer, check_loss_scaling, check_targets, pin_training_dtype


class EsrganGanTrainer(FusedTrainer):
    def __init__(self, g_model, d_model, content_criterion=None, *, g_lr: float = 1e-4, d_lr: float = 1e-4, betas=(0.9, 0.99),
                 eps: float = 1e-8, weight_decay: float = 0.0, ema_decay: Optional[float] = 0.99998, pixel_weight: float = 0.01,
                 content_weight: float = 1.0, adversarial_weight: float = 0.005, process_group=None):
        # defaults = ESRGAN/esrgan_config.py:75-111
        self.g, self.d, self.content = g_model, d_model, content_criterion
        pin_training_dtype(g_model, d_model, content_criterion)     # train_esrgan.py:370-410 runs under amp.autocast(): float16
        self.ge, self.de = generator_engine(g_model), esrgan_discriminator_engine(d_model)
        if content_criterion is not None and not getattr(content_criterion, "single_node", False):
            raise A.SrganfdError("EsrganGanTrainer: content_criterion must be model.ContentLoss built with ONE node name, a str (ESRGAN's form)")
        self.ce = _engine(content_criterion, lambda: ContentLossGradEngine(content_criterion)) if content_criterion is not None else None
        dev = next(g_model.parameters()).device
        self.dev = dev
        self.g_opt = FlatAdamEMA(self.ge.fp.sync(dev), g_lr, betas, eps, weight_decay, ema_decay, layout=self.ge.fp)
        self.d_opt = FlatAdamEMA(self.de.fp.sync(dev), d_lr, betas, eps, weight_decay, None, layout=self.de.fp)
        self.pw, self.cw, self.aw = float(pixel_weight), float(content_weight), float(adversarial_weight)
        # Under data parallelism the discriminator's BatchNorm layers (ESRGAN/model.py:98-126) use per-rank batch statistics, which is
        # what the unconverted reference does under DistributedDataParallel; there is no SyncBatchNorm hook for this discriminator.
        # scalars: [d_loss, pixel, content, adversarial, D(gt) prob, D(sr) prob, 0, 0]  (train_esrgan.py:416,430-431)
        super().__init__(dev, process_group, 8, g_model, d_model, content_criterion)
        self.sr: Optional[Tensor] = None

    def _rel(self, x: Tensor, other: Tensor, target: float, weight: float, slot: int, accumulate: int, grad_x, acc_x: int, grad_other, acc_o: int,
             seed_weight: Optional[float] = None) -> None:
        """weight * mean BCE(x - mean(other), target) into scalars[slot]; seeds scaled by seed_weight (default: weight) x loss scale"""
        A.check(A.lib().srganfd_bce_logits_relativistic(
            x.data_ptr(), x.numel(), other.data_ptr(), other.numel(), target, weight, self.scalars.data_ptr() + 4 * slot, accumulate,
            grad_x.data_ptr() if grad_x is not None else None, acc_x, grad_other.data_ptr() if grad_other is not None else None, acc_o,
            weight if seed_weight is None else seed_weight, self.scaler.seed_ptr, self.ws.data_ptr(), A.stream_ptr()), "bce_logits_relativistic")

    def step(self, lr_img: Tensor, gt: Tensor) -> Tensor:
        """One iteration; returns the device tensor [d_loss, pixel, content, adversarial, D(gt), D(sr), 0, 0] (no host synchronisation)."""
        check_targets("EsrganGanTrainer.step", self.ge, lr_img, gt=gt)
        ge, de = self.ge, self.de
        gt = gt.contiguous().float()
        check_loss_scaling(self.scaler, self.g, self.d, self.content)
        # ---- generator (train_esrgan.py:361-392) ----
        sr = ge.forward(lr_img, True)
        g_sp, g_tok = ge._last, ge.token
        gt_out = de.forward(gt, True)                                        # constant for the generator: only its mean is used
        sr_out = de.forward(sr, True)
        d_sp, d_tok = de._last, de.token
        dsr = self._buf("dsr", sr)
        self._pixel_loss(sr, gt, self.pw, 1, dsr)
        dl = self._buf("dl", sr_out)
        half = 0.5 * self.aw
        self._rel(gt_out, sr_out, 0.0, half, 3, 0, None, 0, dl, 0)           # reaches sr_out through the mean
        self._rel(sr_out, gt_out, 1.0, half, 3, 1, dl, 1, None, 0)           # reaches sr_out directly; loss values add up in slot 3
        _, dsr_adv = de.backward(d_sp, d_tok, dl, False, True)               # frozen D: data gradient only
        self._add(dsr_adv, dsr)
        if self.ce is not None:
            closs = self.ce.forward(sr, gt)                                  # 1-element device tensor: L1 at the node
            c_sp, c_tok = self.ce._last, self.ce.token
            self._add(closs, self.scalars[2:3], self.cw, 0.0)                # the weighted value into its slot
            self._add(self.ce.backward(c_sp, c_tok, None, self.cw, self.scaler.seed_ptr), dsr)
        self._update_generator(g_sp, g_tok, dsr)                             # scaler.step(g_optimizer); scaler.update(); EMA (:383-389)
        # ---- discriminator (train_esrgan.py:394-425) ----
        gt_out = de.forward(gt, True)
        gt_sp, gt_tok = de._last, de.token
        de.forward(sr, True)                                                 # second forward of the pair: advances the BatchNorm statistics
        sr_out = de.forward(sr, True)                                        # the same logits; this graph takes both seeds
        sr_sp, sr_tok = de._last, de.token
        dgt, dsr_l = self._buf("dgt", gt_out), self._buf("dl", sr_out)
        self._rel(gt_out, sr_out, 1.0, 0.5, 0, 0, dgt, 0, dsr_l, 0)          # d_loss_gt: seeds both graphs
        self._rel(sr_out, gt_out, 0.0, 0.5, 0, 1, dsr_l, 1, dgt, 1)          # d_loss_sr; d_loss = their sum in slot 0
        gd1, _ = de.backward(gt_sp, gt_tok, dgt, True, False)
        gd2, _ = de.backward(sr_sp, sr_tok, dsr_l, True, False)
        self._update_discriminator(gd1, gd2)                                 # scaler.step(d_optimizer); scaler.update() (:419-420)
        de.fp.touch()
        self._prob(gt_out, 4)
        self._prob(sr_out, 5)
        self.sr = sr
        return self.scalars
