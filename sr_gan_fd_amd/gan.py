"""Fused GAN training iteration -- the reference's BSRGAN/train_bsrgan.py:387-483 on the HIP engines
(``generator_first=True``: Real_ESRGAN/train_realesrgan.py:407-476, see ``GanTrainer._step_generator_first``).

Order kept exactly: D(gt) forward+backward, G forward, D(sr.detach())
forward+backward (gradients accumulate), D Adam step, freeze D, pixel (L1) + content (VGG-19, detached:
logged only) + adversarial (BCE vs ones through the UPDATED D; spectral-norm u/v advance a third time),
G backward (through D's data gradient only), G Adam step, EMA update.
Data parallel: one flat-gradient all-reduce per network per iteration (D after its second backward,
G after its backward) over RCCL; losses are means over the local shard, identical maths to the
single-process step on the concatenated batch.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _abi as A
from .engine import generator_engine
from .engine_a import aesrgan_engine
from .engine_d import discriminator_engine
from .parallel import SideStreamReducer, SyncBatchNormReduce
from .trainer import FlatAdamEMA, FusedTrainer, check_generator, check_loss_scaling, check_targets, pin_training_dtype


class GanTrainer(FusedTrainer):
    def __init__(self, g_model, d_model, content_criterion=None, *, g_lr: float = 8e-5, d_lr: float = 2e-4, betas=(0.9, 0.999),
                 eps: float = 1e-4, weight_decay: float = 0.0, ema_decay: float = 0.999, pixel_weight: float = 20.0,
                 content_weight=1.0, adversarial_weight: float = 0.5, train_generator: bool = True, process_group=None,
                 generator_first: bool = False, sync_batchnorm: bool = False):
        # defaults = BSRGAN/bsrgan_config.py:137-159
        self.g, self.d, self.content = g_model, d_model, content_criterion
        pin_training_dtype(g_model, d_model, content_criterion)     # modules left at "follow autocast" train in the loops' float16
        # either discriminator of the reference: DiscriminatorUNet (BSRGAN / Real-ESRGAN) or the A-ESRGAN attention U-Net
        # (A-ESRGAN/train_aesrgan.py:396-483 runs the same statements around it); both engines share one interface
        d_engine = aesrgan_engine if type(d_model).__name__ == "UNetDiscriminatorAesrgan" else discriminator_engine
        self.ge, self.de = generator_engine(g_model), d_engine(d_model)
        check_generator("GanTrainer", self.ge, weight_decay, process_group)
        dev = next(g_model.parameters()).device
        self.dev = dev
        self.g_opt = FlatAdamEMA(self.ge.fp.sync(dev), g_lr, betas, eps, weight_decay, ema_decay, layout=self.ge.fp)
        self.d_opt = FlatAdamEMA(self.de.fp.sync(dev), d_lr, betas, eps, weight_decay, None, layout=self.de.fp)
        self.pw, self.cw, self.aw = pixel_weight, content_weight, adversarial_weight
        # scalars: [d_loss_hr, d_loss_sr, pixel, adversarial, D(gt) prob, D(sr) prob, 0, 0]
        super().__init__(dev, process_group, 8, g_model, d_model)
        # per-node content weights (Real-ESRGAN's list): built once -- a host list turned into a device tensor inside step() is a
        # host->device copy per iteration and cannot be captured into a graph
        self._cw_t = None if isinstance(content_weight, (int, float)) else torch.tensor(list(content_weight), dtype=torch.float32, device=dev)
        self.train_generator = train_generator
        self.generator_first = generator_first
        self.d_reducer = SideStreamReducer(dev, process_group)      # D's gradient exchange + Adam beside the generator-side losses
        if sync_batchnorm:
            # A-ESRGAN's attention blocks carry BatchNorm2d (A-ESRGAN/model.py:233): whole-batch statistics across the ranks
            if not hasattr(self.de, "sync_bn"):
                raise ValueError("sync_batchnorm: this discriminator has no BatchNorm layers served by the two-phase kernels")
            self.de.sync_bn = SyncBatchNormReduce(process_group)
        self.content_vals: Optional[Tensor] = None

    def _bce(self, logits: Tensor, target: float, weight: float, slot: int, prob_slot: Optional[int], dlogits: Tensor) -> None:
        """loss value weighted by ``weight``; its gradient by ``weight`` times the loss scale the device holds when the kernel runs
        (scaler.scale(loss): trainer.LossScaler)"""
        s = self.scalars.data_ptr()
        A.check(A.lib().srganfd_bce_logits(logits.data_ptr(), logits.numel(), target, weight, s + 4 * slot, 0,
                                           (s + 4 * prob_slot) if prob_slot is not None else None, dlogits.data_ptr(), weight,
                                           self.scaler.seed_ptr, self.ws.data_ptr(), A.stream_ptr()), "bce_logits")

    def _content(self, sr: Tensor, gt: Tensor) -> None:
        if self.content is not None:
            cw = self.cw if self._cw_t is None else self._cw_t
            self.content_vals = self.content(sr, gt) * cw      # per-node weights broadcast over the (1, nodes) tensor

    # -- the phases both orders are made of -----------------------------------------------------------------------------
    def _d_pass(self, x: Tensor, target: float, loss_slot: int, prob_slot: int) -> Tensor:
        """D forward on ``x``, BCE against ``target`` (scaler.scale(d_loss_*): train_bsrgan.py:420,430), D backward: the flat
        gradient.  The probability the scripts log is written by the BCE kernel (BSRGAN: mean of sigmoids) or, generator first, as
        sigmoid(mean(logits)) (train_realesrgan.py:475-476)."""
        de = self.de
        out = de.forward(x, True)
        dl = self._buf("dl", out)
        self._bce(out, target, 1.0, loss_slot, None if self.generator_first else prob_slot, dl)
        if self.generator_first:
            self._prob(out, prob_slot)
        return de.backward(de._last, de.token, dl, True, False)[0]

    def _adversarial_update(self, sr: Tensor, dsr: Tensor, g_sp, g_tok) -> None:
        """BCE vs ones through the current D (its SN state advances again, train_bsrgan.py:452); D is frozen: its data gradient
        only, added to the pixel loss's in ``dsr``; then scaler.step(g_optimizer); scaler.update(); EMA (:466-470)"""
        de = self.de
        adv_out = de.forward(sr, True)
        dl = self._buf("dl", adv_out)
        self._bce(adv_out, 1.0, self.aw, 3, None, dl)
        if self.train_generator:
            _, dsr_adv = de.backward(de._last, de.token, dl, False, True)
            self._add(dsr_adv, dsr)
            self._update_generator(g_sp, g_tok, dsr)

    def _step_generator_first(self, lr_img: Tensor, gt: Tensor, gtu: Tensor) -> None:
        """Real_ESRGAN/train_realesrgan.py:407-476: the GENERATOR step first -- pixel and (detached) content loss against the
        USM-sharpened GT, adversarial BCE vs ones through the frozen current D, G Adam step + EMA -- then the discriminator on the
        plain GT and on the detached SR (two backward passes accumulate), D Adam step."""
        ge = self.ge
        self.sr = sr = ge.forward(lr_img, True)
        g_sp, g_tok = ge._last, ge.token
        dsr = self._buf("dsr", sr)
        self._pixel_loss(sr, gtu, self.pw, 2, dsr)
        self._content(sr, gtu)
        self._adversarial_update(sr, dsr, g_sp, g_tok)
        gd1 = self._d_pass(gt, 1.0, 0, 4)
        self._update_discriminator(gd1, self._d_pass(sr, 0.0, 1, 5))

    def step(self, lr_img: Tensor, gt: Tensor, gt_usm: Optional[Tensor] = None) -> Tensor:
        """One iteration; returns the device tensor [d_loss_hr, d_loss_sr, pixel, adversarial, D(gt), D(sr), 0, 0]
        (no host synchronisation inside; content-loss values are in ``self.content_vals``).  ``gt_usm`` (generator-first
        mode): the sharpened GT the generator's pixel / content losses compare against; the discriminator sees ``gt``."""
        check_targets("GanTrainer.step", self.ge, lr_img, gt=gt, gt_usm=gt_usm)
        if gt_usm is not None and not self.generator_first:
            raise A.SrganfdError("GanTrainer.step: gt_usm belongs to the generator-first (Real-ESRGAN) iteration")
        check_loss_scaling(self.scaler, self.g, self.d)
        gt = gt.contiguous().float()
        if self.generator_first:
            self._step_generator_first(lr_img, gt, gt if gt_usm is None else gt_usm.contiguous().float())
            return self.scalars
        ge = self.ge
        # ---- discriminator ----
        gd1 = self._d_pass(gt, 1.0, 0, 4)
        self.sr = sr = ge.forward(lr_img, True)
        g_sp, g_tok = ge._last, ge.token
        gd2 = self._d_pass(sr, 0.0, 1, 5)
        # scaler.step(d_optimizer); scaler.update()  (:436-437).  Under data parallelism the sum of the two gradients, the all-reduce
        # and the Adam kernel go to a side stream: the VGG-19 content forwards below do not read D's parameters
        self.d_reducer.launch(lambda: self._update_discriminator(gd1, gd2), tensors=(gd1, gd2))
        # ---- generator ----
        dsr = self._buf("dsr", sr)
        self._content(sr, gt)
        self.d_reducer.wait()                               # D's updated parameters -- and the loss scale after its update() -- from here on
        # the pixel loss seeds the generator's backward pass with the scale AFTER the discriminator's scaler.update() (:463)
        self._pixel_loss(sr, gt, self.pw, 2, dsr)
        self._adversarial_update(sr, dsr, g_sp, g_tok)
        return self.scalars
