"""Drop-in mirror of the reference's ``model.py`` module surface, running on hand-written HIP kernels.

Same names, constructor kwargs, ``state_dict`` keys/shapes (NCHW fp32 parameters) and ``nn.Module``
protocol as ``BSRGAN/model.py`` (BSRGAN :311-384, DiscriminatorUNet :91-167, ContentLoss :501-554,
factories :557-593) and ``ESRGAN/model.py`` (RRDBNet :144-243, factories :301-322), so that
``model.__dict__[cfg.g_model_arch_name](**kwargs)`` (train_bsrgan.py:274-285), ``AveragedModel``
deep copies, pickling and ``utils.load_state_dict`` keep working.

The sub-modules (``nn.Conv2d``, ``spectral_norm``) are used ONLY as parameter containers: they give
the reference's parameter names, shapes, construction order and therefore the same RNG stream at
init.  Their ``forward`` is never called -- ``forward`` here hands the parameters to the HIP engine
(``engine.py``), which raises if libsrganfd_hip.so or a GPU is missing (no CPU fallback).

Precision follows the reference's own contract (``engine.resolve_compute_dtype``): inside ``torch.autocast("cuda")`` -- the
train loops' ``amp.autocast()``, train_bsrgan.py:415-427,450-457 -- the kernels compute in the autocast dtype (float16 unless
the caller asked autocast for bfloat16: f16 MFMA, fp32 accumulate, fp32 master weights, fp32 SR / logits); outside it --
``validate()``, train_bsrgan.py:563, inference.py -- in float32 (exact-fp32 MFMA, the mode every golden vector is met in).
One knob beyond the reference: ``compute_dtype`` (default ``None`` = follow autocast) pins a module to torch.float32 /
float16 / bfloat16 whatever the autocast state; the fused trainers and bench.py set it explicitly.
"""
from __future__ import annotations

from typing import Any, List

import torch
from torch import Tensor, nn
from torch.nn.utils import spectral_norm

__all__ = [
    "DiscriminatorUNet", "BSRGAN", "RRDBNet", "ContentLoss",
    "discriminator_unet", "bsrgan_x2", "bsrgan_x4", "content_loss",
    "rrdbnet_x1", "rrdbnet_x2", "rrdbnet_x4", "rrdbnet_x8",
    "UNetDiscriminatorAesrgan", "uNetDiscriminatorAesrgan",
    "Discriminator", "discriminator",
    "SelfAttention", "BSRGANsa", "bsrgansa_x2",
    "RPA", "US", "Generator_RPA", "gen_rpa2x",
    "TransformerEncoderLayer", "TransformerEncoder",
    "BSRGANtrans", "bsrgantrans_x2",
]


class _ResidualDenseBlock(nn.Module):
    """Parameter container of BSRGAN/model.py:31-62; standalone forward = a 1-block trunk on the GPU."""

    def __init__(self, channels: int, growth_channels: int, self_init: bool = False) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(channels + growth_channels * 0, growth_channels, (3, 3), (1, 1), (1, 1))
        self.conv2 = nn.Conv2d(channels + growth_channels * 1, growth_channels, (3, 3), (1, 1), (1, 1))
        self.conv3 = nn.Conv2d(channels + growth_channels * 2, growth_channels, (3, 3), (1, 1), (1, 1))
        self.conv4 = nn.Conv2d(channels + growth_channels * 3, growth_channels, (3, 3), (1, 1), (1, 1))
        self.conv5 = nn.Conv2d(channels + growth_channels * 4, channels, (3, 3), (1, 1), (1, 1))
        self.leaky_relu = nn.LeakyReLU(0.2, True)
        self.identity = nn.Identity()
        if self_init:     # Real_ESRGAN/model.py:135-150: its dense block initialises itself (the generator then re-draws everything)
            for module in self.modules():
                if isinstance(module, nn.Conv2d):
                    nn.init.kaiming_normal_(module.weight)
                    module.weight.data *= 0.1
                    if module.bias is not None:
                        nn.init.constant_(module.bias, 0)
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine import trunk_apply
        return trunk_apply(self, x, [self], rrdb=False)


class _ResidualResidualDenseBlock(nn.Module):
    """Parameter container of BSRGAN/model.py:65-88."""

    def __init__(self, channels: int, growth_channels: int, self_init: bool = False) -> None:
        super().__init__()
        self.rdb1 = _ResidualDenseBlock(channels, growth_channels, self_init)
        self.rdb2 = _ResidualDenseBlock(channels, growth_channels, self_init)
        self.rdb3 = _ResidualDenseBlock(channels, growth_channels, self_init)
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine import trunk_apply
        return trunk_apply(self, x, [self.rdb1, self.rdb2, self.rdb3], rrdb=True)


class _RRDBGenerator(nn.Module):
    """Shared body of BSRGAN (BSRGAN/model.py:311-384) and RRDBNet (ESRGAN/model.py:144-243)."""

    def __init__(self, in_channels: int, out_channels: int, channels: int, growth_channels: int,
                 num_blocks: int, upscale_factor: int, always_up1: bool, rdb_self_init: bool = False, unshuffle: int = 1) -> None:
        super().__init__()
        self.upscale_factor = upscale_factor
        # Real-ESRGAN below x4 (Real_ESRGAN/model.py:190-204,248): the input is pixel-unshuffled by `unshuffle` (conv1 sees
        # in_channels * unshuffle^2 channels at 1 / unshuffle of the size) and BOTH nearest-x2 stages always run
        self.unshuffle = unshuffle
        if unshuffle > 1:
            in_channels *= unshuffle * unshuffle
            self.downsampling = nn.PixelUnshuffle(unshuffle)
        self.conv1 = nn.Conv2d(in_channels, channels, (3, 3), (1, 1), (1, 1))
        self.trunk = nn.Sequential(*[_ResidualResidualDenseBlock(channels, growth_channels, rdb_self_init) for _ in range(num_blocks)])
        self.conv2 = nn.Conv2d(channels, channels, (3, 3), (1, 1), (1, 1))
        n_up = {1: 0, 2: 1, 4: 2, 8: 3}[upscale_factor * unshuffle]
        if always_up1:               # BSRGAN builds upsampling1 unconditionally (model.py:337-340)
            n_up = max(n_up, 1)
        for u in range(1, n_up + 1):
            setattr(self, f"upsampling{u}", nn.Sequential(
                nn.Conv2d(channels, channels, (3, 3), (1, 1), (1, 1)), nn.LeakyReLU(0.2, True)))
        self.conv3 = nn.Sequential(nn.Conv2d(channels, channels, (3, 3), (1, 1), (1, 1)), nn.LeakyReLU(0.2, True))
        self.conv4 = nn.Conv2d(channels, out_channels, (3, 3), (1, 1), (1, 1))
        # BSRGAN/model.py:358-363, ESRGAN/model.py:236-242
        for module in self.modules():
            if isinstance(module, nn.Conv2d):
                nn.init.kaiming_normal_(module.weight)
                module.weight.data *= 0.1
                if module.bias is not None:
                    nn.init.constant_(module.bias, 0)
        self.compute_dtype = None

    def n_upsample(self) -> int:
        return {1: 0, 2: 1, 4: 2, 8: 3}[self.upscale_factor * getattr(self, "unshuffle", 1)]

    def forward(self, x: Tensor) -> Tensor:
        return self._forward_impl(x)

    def _forward_impl(self, x: Tensor) -> Tensor:
        from .engine import generator_apply
        # below x4 the engine applies the PixelUnshuffle itself (engine.TrunkEngine.forward), for this path and the fused trainers alike
        return generator_apply(self, x)


class BSRGAN(_RRDBGenerator):
    def __init__(self, in_channels: int = 3, out_channels: int = 3, channels: int = 64, growth_channels: int = 32,
                 num_rrdb: int = 23, upscale_factor: int = 4) -> None:
        super().__init__(in_channels, out_channels, channels, growth_channels, num_rrdb, upscale_factor, always_up1=True)


class BSRGANsa(_RRDBGenerator):
    """BSRGAN/model.py:405-496: despite its name the class holds no attention layer -- its parameters and its forward are BSRGAN's
    (``visualize_attention_map`` reads an attribute nothing sets) -- so configs that name ``bsrgansa_x2`` get the same engine."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, channels: int = 64, growth_channels: int = 32,
                 num_rrdb: int = 23, upscale_factor: int = 4) -> None:
        super().__init__(in_channels, out_channels, channels, growth_channels, num_rrdb, upscale_factor, always_up1=True)


class SelfAttention(nn.Module):
    """BSRGAN/model.py:388-402: ``nn.MultiheadAttention(channels, num_heads)`` over the h*w positions of a (b, c, h, w) map, every
    image its own sequence.  The child module is a parameter container (the reference's state-dict keys, shapes and seeded initial
    values); ``forward`` runs the fused HIP attention (attention.py, csrc/attention.hip) and returns the reference's pair
    ``(attn_output (b, c, h, w), attn_output_weights (b, h*w, h*w))``, both fp32.

    Deviations: the weights come back detached (no consumer in the reference differentiates them); ``need_weights = False`` on the
    module skips the launch that computes them and returns ``None`` in their place; CPU tensors, ``channels % num_heads != 0`` and a
    head size outside {16, 32, 64} raise ``SrganfdError``."""

    def __init__(self, channels: int, num_heads: int = 8) -> None:
        super().__init__()
        if channels % num_heads:
            from ._abi import SrganfdError
            raise SrganfdError(f"SelfAttention: channels {channels} is not a multiple of num_heads {num_heads}")
        self.channels = channels
        self.num_heads = num_heads
        self.multihead_attention = nn.MultiheadAttention(channels, num_heads)
        self.need_weights = True
        self.compute_dtype = None

    def forward(self, x: Tensor):
        from .attention import self_attention_apply
        return self_attention_apply(self, x)


class TransformerEncoderLayer(nn.TransformerEncoderLayer):
    """The layer of the reference's transformer block (A-ESRGAN/model.py:673: ``TransformerEncoderLayer(d_model=channels, nhead=4)``
    with torch's defaults -- post-norm, ReLU, dim_feedforward 2048, dropout 0.1, batch_first=False, LayerNorm eps 1e-5, biases).
    torch's class is the parameter container (its state-dict keys, shapes and seeded initial values); ``forward(src)`` runs the HIP
    engine (transformer.py) on a ``(S, N, E)`` fp32 GPU tensor -- S is the sequence axis -- and returns the same shape in fp32,
    differentiable in ``src`` and every parameter.  In ``.train()`` mode with ``dropout > 0`` all four dropout sites are live;
    ``dropout_masks()`` returns the keep-masks of the last training forward.

    Deviations: ``norm_first=True``, an activation other than ReLU, ``batch_first=True``, ``bias=False``, any mask or ``is_causal``
    argument, ``d_model % 32 != 0``, a head size outside {16, 32, 64}, ``dim_feedforward % 32 != 0``, sequences longer than 128, CPU
    tensors and a wrong last dimension raise ``SrganfdError``."""

    def __init__(self, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)
        from .transformer import check_layer
        check_layer(self)
        self.compute_dtype = None

    def forward(self, src: Tensor, src_mask=None, src_key_padding_mask=None, is_causal=False) -> Tensor:
        from .transformer import check_no_masks, transformer_apply
        check_no_masks("TransformerEncoderLayer", src_mask=src_mask, src_key_padding_mask=src_key_padding_mask, is_causal=is_causal)
        return transformer_apply(self, src)

    def dropout_masks(self) -> dict:
        from .transformer import transformer_engine
        return transformer_engine(self).dropout_masks()


class TransformerEncoder(nn.TransformerEncoder):
    """A-ESRGAN/model.py:674: ``TransformerEncoder(encoder_layer, num_layers)``, torch's class as the parameter container
    (``layers.{i}.*``, ``_get_clones`` copies of the layer given); ``forward(src)`` runs the whole stack as ONE engine (transformer.py).
    ``encoder_layer`` is a TransformerEncoderLayer of this module; a final ``norm`` raises ``SrganfdError``, as does everything the layer
    refuses.  ``dropout_masks()``: the keep-masks of the last training forward, keys ``layers.{i}.<site>``."""

    def __init__(self, encoder_layer: nn.Module, num_layers: int, *args: Any, **kwargs: Any) -> None:
        from ._abi import SrganfdError
        if not isinstance(encoder_layer, TransformerEncoderLayer):
            raise SrganfdError("TransformerEncoder: encoder_layer must be a sr_gan_fd_amd TransformerEncoderLayer")
        kwargs.setdefault("enable_nested_tensor", False)        # torch's fast path, which this class never takes
        super().__init__(encoder_layer, num_layers, *args, **kwargs)
        if self.norm is not None:
            raise SrganfdError("TransformerEncoder: a final norm has no kernel (the reference's stack has none)")
        self.compute_dtype = None

    def forward(self, src: Tensor, mask=None, src_key_padding_mask=None, is_causal=None) -> Tensor:
        from .transformer import check_no_masks, transformer_apply
        check_no_masks("TransformerEncoder", mask=mask, src_key_padding_mask=src_key_padding_mask, is_causal=is_causal)
        return transformer_apply(self, src)

    def dropout_masks(self) -> dict:
        from .transformer import transformer_engine
        return transformer_engine(self).dropout_masks()


class BSRGANtrans(nn.Module):
    """A-ESRGAN/model.py:643-746, the generator A-ESRGAN's configuration names (aesrgan_config.py:50): conv1, the RRDB trunk, a 3x3
    stride-2 conv + LeakyReLU (``downsamplingTrans``), two post-norm transformer layers over the half-size map read as ``(B, h w, C)``
    with batch_first=False -- the sequence axis is the BATCH: one sample's SR depends on the rest of its batch --, nearest x2 + conv
    + LeakyReLU (``upsamplingTrans``), conv2, ``+ out1`` (the trunk's own output is not added back), the tail, clamp to [0, 1].
    Same constructor arguments, state-dict keys and shapes, construction order and therefore seeded initial values: the init loop
    re-draws the nn.Conv2d weights only, the transformer keeps torch's initialisation.  ``transformer_layer`` is registered and never
    called (``transformer_encoder`` holds copies of it): its gradients stay ``None``.  The sub-modules are parameter containers; the
    whole network is ONE HIP engine (engine_trans.py).  In ``.train()`` mode all eight dropout sites are live; ``dropout_masks()``
    returns the last training forward's keep-masks under ``transformer_encoder.layers.{i}.<site>``.

    Deviations: odd H or W (the reference's ``view`` fails there too), a batch above 128, ``channels`` that is no multiple of 32 or
    whose quarter is no attention head size (16, 32, 64), ``growth_channels % 32``, a wrong channel count, CPU tensors and everything
    TransformerEncoderLayer refuses raise ``SrganfdError``."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, channels: int = 64, growth_channels: int = 32,
                 num_rrdb: int = 23, upscale_factor: int = 4) -> None:
        super().__init__()
        self.upscale_factor = upscale_factor
        self.channels = channels
        conv = lambda cin, cout, stride=1: nn.Conv2d(cin, cout, (3, 3), (stride, stride), (1, 1))
        act_conv = lambda stride=1: nn.Sequential(conv(channels, channels, stride), nn.LeakyReLU(0.2, True))
        # the reference's order: it fixes the named_parameters() order and the random stream of a seeded construction
        self.conv1 = conv(in_channels, channels)
        self.trunk = nn.Sequential(*[_ResidualResidualDenseBlock(channels, growth_channels) for _ in range(num_rrdb)])
        self.downsamplingTrans = act_conv(2)
        self.transformer_layer = TransformerEncoderLayer(d_model=channels, nhead=4)
        self.transformer_encoder = TransformerEncoder(self.transformer_layer, num_layers=2)
        self.upsamplingTrans = act_conv()
        self.conv2 = conv(channels, channels)
        self.upsampling1 = act_conv()
        if upscale_factor == 4:
            self.upsampling2 = act_conv()
        self.conv3 = act_conv()
        self.conv4 = conv(channels, out_channels)
        for module in self.modules():
            if isinstance(module, nn.Conv2d):
                nn.init.kaiming_normal_(module.weight)
                module.weight.data *= 0.1
                if module.bias is not None:
                    nn.init.constant_(module.bias, 0)
        self.compute_dtype = None

    def n_upsample(self) -> int:
        return 2 if self.upscale_factor == 4 else 1

    def forward(self, x: Tensor) -> Tensor:
        return self._forward_impl(x)

    def _forward_impl(self, x: Tensor) -> Tensor:
        from .engine import generator_apply
        return generator_apply(self, x)

    def dropout_masks(self) -> dict:
        from .engine import generator_engine
        return generator_engine(self).dropout_masks()


class RRDBNet(_RRDBGenerator):
    """ESRGAN/model.py:144-243 (``num_blocks``) and Real_ESRGAN/model.py:179-262 (``num_rrdb``: x4 as its shipped factory --
    PixelUnshuffle is the identity --, x2 / x1 with PixelUnshuffle(2 / 4) in front of conv1; both upsampling stages always run)."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, channels: int = 64, growth_channels: int = 32,
                 num_blocks: int = 23, upscale_factor: int = 4, num_rrdb: int = None) -> None:
        unshuffle = 1
        if num_rrdb is not None:
            if upscale_factor not in (1, 2, 4):
                raise ValueError("Real-ESRGAN's RRDBNet takes upscale_factor 1, 2 or 4 (Real_ESRGAN/model.py:190-201)")
            unshuffle = 4 // upscale_factor       # x2: PixelUnshuffle(2), x1: PixelUnshuffle(4), x4: identity
            num_blocks = num_rrdb
        # Real-ESRGAN's dense blocks draw their own initialisation first: same random stream, so a seeded construction
        # gives the reference's initial weights
        super().__init__(in_channels, out_channels, channels, growth_channels, num_blocks, upscale_factor, always_up1=False,
                         rdb_self_init=num_rrdb is not None, unshuffle=unshuffle)


class DiscriminatorUNet(nn.Module):
    """BSRGAN/model.py:91-167 (identical Real_ESRGAN/model.py:29-105)."""

    def __init__(self, in_channels: int, out_channels: int, channels: int, upsample_method: str = "bilinear") -> None:
        super().__init__()
        # stored and never read, exactly as the reference does (BSRGAN/model.py:97-100): its forward hard-codes
        # F.interpolate(..., mode="bilinear") at :150,154,158 whatever this says, and so does the HIP path
        self.upsample_method = upsample_method
        self.conv1 = nn.Conv2d(in_channels, 64, (3, 3), (1, 1), (1, 1))

        def sn(cin, cout, k, s):
            return nn.Sequential(spectral_norm(nn.Conv2d(cin, cout, (k, k), (s, s), (1, 1), bias=False)),
                                 nn.LeakyReLU(0.2, True))
        self.down_block1 = sn(channels, int(channels * 2), 4, 2)
        self.down_block2 = sn(int(channels * 2), int(channels * 4), 4, 2)
        self.down_block3 = sn(int(channels * 4), int(channels * 8), 4, 2)
        self.up_block1 = sn(int(channels * 8), int(channels * 4), 3, 1)
        self.up_block2 = sn(int(channels * 4), int(channels * 2), 3, 1)
        self.up_block3 = sn(int(channels * 2), channels, 3, 1)
        self.conv2 = sn(channels, channels, 3, 1)
        self.conv3 = sn(channels, channels, 3, 1)
        self.conv4 = nn.Conv2d(channels, out_channels, (3, 3), (1, 1), (1, 1))
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        return self._forward_impl(x)

    def _forward_impl(self, x: Tensor) -> Tensor:
        from .engine import discriminator_apply
        return discriminator_apply(self, x)


class ContentLoss(nn.Module):
    """BSRGAN/model.py:501-554.  torchvision and the ImageNet VGG-19 weights are not part of the
    reference tree (third-party, network download), so the VGG-19 ``features[0:35]`` topology is
    restated here and its weights come from ``weights_path`` (a torchvision ``vgg19`` state_dict) or,
    when absent, from a seeded random init (benchmarks).  The returned tensor is DETACHED with shape
    (1, len(nodes)) exactly like the reference's ``torch.Tensor([losses])`` (:552).

    ESRGAN's variant (ESRGAN/model.py:258-292) passes ONE node name as a string and keeps the result in the autograd
    graph (``F.l1_loss`` of the two feature maps, a scalar): given a ``str`` this class behaves that way, with the frozen
    extractor's backward pass on the HIP engine (engine_v.py)."""

    def __init__(self, feature_model_extractor_nodes, feature_model_normalize_mean: list,
                 feature_model_normalize_std: list, weights_path: str = "", taps_post_relu: bool = True) -> None:
        super().__init__()
        from .vgg import build_vgg19_features
        self.single_node = isinstance(feature_model_extractor_nodes, str)
        if self.single_node:
            feature_model_extractor_nodes = [feature_model_extractor_nodes]
        self.feature_model_extractor_nodes = list(feature_model_extractor_nodes)
        self.taps_post_relu = taps_post_relu
        self.features = build_vgg19_features(weights_path)
        self.register_buffer("mean", torch.tensor(feature_model_normalize_mean, dtype=torch.float32))
        self.register_buffer("std", torch.tensor(feature_model_normalize_std, dtype=torch.float32))
        for p in self.features.parameters():
            p.requires_grad = False
        self.compute_dtype = None

    def forward(self, sr_tensor: Tensor, gt_tensor: Tensor) -> Tensor:
        assert sr_tensor.size() == gt_tensor.size(), "Two tensor must have the same size"
        if self.single_node:
            from .engine_v import content_loss_single_apply
            return content_loss_single_apply(self, sr_tensor, gt_tensor)
        from .engine import content_loss_apply
        return content_loss_apply(self, sr_tensor, gt_tensor)


class add_attn(nn.Module):
    """Parameter container of the attention gate, A-ESRGAN/model.py:228-254."""

    def __init__(self, x_channels, g_channels=256):
        super().__init__()
        self.W = nn.Sequential(nn.Conv2d(x_channels, x_channels, kernel_size=1, stride=1, padding=0), nn.BatchNorm2d(x_channels))
        self.theta = nn.Conv2d(x_channels, x_channels, kernel_size=2, stride=2, padding=0, bias=False)
        self.phi = nn.Conv2d(g_channels, x_channels, kernel_size=1, stride=1, padding=0, bias=True)
        self.psi = nn.Conv2d(x_channels, out_channels=1, kernel_size=1, stride=1, padding=0, bias=True)


class unetCat(nn.Module):
    """Parameter container of A-ESRGAN/model.py:258-275."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.convU = spectral_norm(nn.Conv2d(dim_in, dim_out, 3, 1, 1, bias=False))


class UNetDiscriminatorAesrgan(nn.Module):
    """A-ESRGAN/model.py:279-345: attention U-Net discriminator with spectral normalisation (BASELINE config 5).
    Same constructor arguments, state_dict keys and construction order (hence the same init RNG stream)."""

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        norm = spectral_norm
        self.conv0 = nn.Conv2d(num_in_ch, num_feat, kernel_size=3, stride=1, padding=1)
        self.conv1 = norm(nn.Conv2d(num_feat, num_feat * 2, 3, 2, 1, bias=False))
        self.conv2 = norm(nn.Conv2d(num_feat * 2, num_feat * 4, 3, 2, 1, bias=False))
        self.conv3 = norm(nn.Conv2d(num_feat * 4, num_feat * 8, 3, 2, 1, bias=False))
        self.gating = norm(nn.Conv2d(num_feat * 8, num_feat * 4, 1, 1, 1, bias=False))
        self.attn_1 = add_attn(x_channels=num_feat * 4, g_channels=num_feat * 4)
        self.attn_2 = add_attn(x_channels=num_feat * 2, g_channels=num_feat * 4)
        self.attn_3 = add_attn(x_channels=num_feat, g_channels=num_feat * 4)
        self.cat_1 = unetCat(dim_in=num_feat * 8, dim_out=num_feat * 4)
        self.cat_2 = unetCat(dim_in=num_feat * 4, dim_out=num_feat * 2)
        self.cat_3 = unetCat(dim_in=num_feat * 2, dim_out=num_feat)
        self.conv4 = norm(nn.Conv2d(num_feat * 8, num_feat * 4, 3, 1, 1, bias=False))
        self.conv5 = norm(nn.Conv2d(num_feat * 4, num_feat * 2, 3, 1, 1, bias=False))
        self.conv6 = norm(nn.Conv2d(num_feat * 2, num_feat, 3, 1, 1, bias=False))
        self.conv7 = norm(nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=False))
        self.conv8 = norm(nn.Conv2d(num_feat, num_feat, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(num_feat, 1, 3, 1, 1)
        self.compute_dtype = None
        self.ly1 = self.ly2 = self.ly3 = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine_a import aesrgan_discriminator_apply
        return aesrgan_discriminator_apply(self, x)

    def getAttentionLayers(self):
        return self.ly1, self.ly2, self.ly3


class Discriminator(nn.Module):
    """ESRGAN/model.py:88-141: VGG-style conv / BatchNorm2d / LeakyReLU stack (3x128x128 -> 512x4x4) and a two-layer
    classifier; used by the relativistic GAN step of ESRGAN/train_esrgan.py:370-425.  Same ``features.*`` /
    ``classifier.*`` state_dict keys; the sub-modules are parameter containers, forward/backward run on the HIP engine."""

    def __init__(self) -> None:
        super().__init__()
        layers = [nn.Conv2d(3, 64, (3, 3), (1, 1), (1, 1), bias=True), nn.LeakyReLU(0.2, True)]
        cin = 64
        for cout, k, s in ((64, 4, 2), (128, 3, 1), (128, 4, 2), (256, 3, 1), (256, 4, 2), (512, 3, 1), (512, 4, 2), (512, 3, 1), (512, 4, 2)):
            layers += [nn.Conv2d(cin, cout, (k, k), (s, s), (1, 1), bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2, True)]
            cin = cout
        self.features = nn.Sequential(*layers)
        self.classifier = nn.Sequential(nn.Linear(512 * 4 * 4, 100), nn.LeakyReLU(0.2, True), nn.Linear(100, 1))
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine_e import esrgan_discriminator_apply
        return esrgan_discriminator_apply(self, x)


class US(nn.Module):
    """A-ESRGAN/model.py:87-109: up-sampling block with pixel attention (nearest x2, 1x1 conv, LeakyReLU, the gate
    ``x * sigmoid(pa_conv(x)) + x``, 3x3 conv, LeakyReLU).  Parameter container; forward and backward run on the HIP engine
    (engine_rpa.py), which applies the per-pixel layers before the up-sampling (same values, a quarter of the work).  Only ``scale`` 2
    has a kernel (the only value the reference's generator passes)."""

    def __init__(self, num_feat, scale):
        super().__init__()
        from .engine_rpa import check_features
        check_features("us", num_feat)
        self.scale = scale
        self.conv1 = nn.Conv2d(num_feat, num_feat, 1)
        self.pa_conv = nn.Conv2d(num_feat, num_feat, 1)
        self.pa_sigmoid = nn.Sigmoid()
        self.conv2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine_rpa import rpa_apply
        return rpa_apply(self, "us", x)


class RPA(nn.Module):
    """A-ESRGAN/model.py:112-140: residual pixel-attention block (1x1 convs F -> 2F -> 4F, 3x3 conv 4F -> F, the gate
    ``x * sigmoid(.) + x``, 3x3 conv F -> F, LeakyReLU).  Parameter container; forward and backward run on the HIP engine
    (engine_rpa.py)."""

    def __init__(self, num_feat):
        super().__init__()
        from .engine_rpa import check_features
        check_features("rpa", num_feat)
        self.conv1 = nn.Conv2d(num_feat, num_feat * 2, 1)
        self.conv2 = nn.Conv2d(num_feat * 2, num_feat * 4, 1)
        self.conv3 = nn.Conv2d(num_feat * 4, num_feat, 3, 1, 1)
        self.conv4 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.sigmoid = nn.Sigmoid()
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        # model.py:125-128, literally: conv3 is drawn twice and conv4 keeps nn.Conv2d's own initialisation -- the same random stream,
        # so a seeded construction gives the reference's initial values
        for layer in [self.conv1, self.conv2, self.conv3, self.conv3]:
            nn.init.kaiming_normal_(layer.weight)
            layer.weight.data *= 0.1
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine_rpa import rpa_apply
        return rpa_apply(self, "rpa", x)


class Generator_RPA(nn.Module):
    """A-ESRGAN/model.py:144-175: conv1, ``num_block`` RPA blocks, the long skip, ceil(log2(scale)) US blocks, conv2, conv3.  Same
    constructor arguments, state_dict keys (``conv1..3``, ``rpa.rpa{i}.conv1..4``, ``us.us{i}.conv1 / pa_conv / conv2``) and
    construction order.  ``num_feat`` must be a multiple of 64 (conv2 writes num_feat // 2 channels)."""

    def __init__(self, num_in_ch=3, num_out_ch=3, scale=2, num_feat=64, num_block=20):
        super().__init__()
        from collections import OrderedDict
        from .engine_rpa import check_features, num_usblock
        check_features("gen", num_feat)
        self.scale = scale
        self.conv1 = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.rpa = nn.Sequential(OrderedDict([("rpa{}".format(i), RPA(num_feat=num_feat)) for i in range(num_block)]))
        self.us = nn.Sequential(OrderedDict([("us{}".format(i), US(num_feat=num_feat, scale=2)) for i in range(num_usblock(scale))]))
        self.conv2 = nn.Conv2d(num_feat, num_feat // 2, 3, 1, 1)
        self.conv3 = nn.Conv2d(num_feat // 2, num_out_ch, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self.compute_dtype = None

    def forward(self, x: Tensor) -> Tensor:
        from .engine_rpa import rpa_apply
        return rpa_apply(self, "gen", x)


def gen_rpa2x() -> Generator_RPA:
    """A-ESRGAN/model.py:217-221"""
    print("* Generator_RPA 2x")
    return Generator_RPA(scale=2)


def discriminator() -> Discriminator:
    """ESRGAN/model.py:293-296"""
    return Discriminator()


def uNetDiscriminatorAesrgan() -> UNetDiscriminatorAesrgan:
    return UNetDiscriminatorAesrgan(3)


def discriminator_unet(**kwargs: Any) -> DiscriminatorUNet:
    return DiscriminatorUNet(**kwargs)


def bsrgansa_x2(**kwargs: Any) -> BSRGANsa:
    """BSRGAN/model.py:570-574"""
    return BSRGANsa(upscale_factor=2, **kwargs)


def bsrgan_x2(**kwargs: Any) -> BSRGAN:
    return BSRGAN(upscale_factor=2, **kwargs)


def bsrgantrans_x2(**kwargs: Any) -> BSRGANtrans:
    """A-ESRGAN/model.py:749-753"""
    print("* BSRGAN TRANSFORMER 2x")
    return BSRGANtrans(upscale_factor=2, **kwargs)


def bsrgan_x4(**kwargs: Any) -> BSRGAN:
    return BSRGAN(upscale_factor=4, **kwargs)


def content_loss(*args: Any, **kwargs: Any) -> ContentLoss:
    """BSRGAN/model.py:568-571 (keyword form) and ESRGAN/model.py:325-332, which passes (node, mean, std) positionally"""
    return ContentLoss(*args, **kwargs)


def rrdbnet_x1(**kwargs: Any) -> RRDBNet:
    return RRDBNet(upscale_factor=1, **kwargs)


def rrdbnet_x2(**kwargs: Any) -> RRDBNet:
    return RRDBNet(upscale_factor=2, **kwargs)


def rrdbnet_x4(**kwargs: Any) -> RRDBNet:
    return RRDBNet(upscale_factor=4, **kwargs)


def rrdbnet_x8(**kwargs: Any) -> RRDBNet:
    return RRDBNet(upscale_factor=8, **kwargs)
