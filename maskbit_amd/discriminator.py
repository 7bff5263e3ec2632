"""The VQGAN+ discriminator and the tokenizer's GAN losses on the device: the reference's ``modeling.modules.discriminator.NLayerDiscriminatorv2``
(the ``VQGAN+Discriminator`` of every MaskBit / VQGAN+ tokenizer config), the loss functions of ``modeling.modules.gan_utils`` and
``modeling.modules.losses.VQGANLoss`` behind ``csrc/discriminator.hip``.  Inference only: no gradients, no optimiser.

``NLayerDiscriminatorv2`` has exactly the reference module's state-dict keys (the ``blocks.{i}.1.kernel`` blur buffers included), so the
``discriminator.*`` entries of a training run's loss-module checkpoint load strictly.  ``forward(x)`` gives the fp32 logits [B, 1, 16, 16];
``logit_stats(x)`` gives, per image, the five float64 sums over its 256 logits that every loss below is a function of:

    0: sum l    1: sum relu(1 - l)    2: sum relu(1 + l)    3: sum softplus(-l)    4: sum softplus(l)

so a held-out pass needs no logits on the host and no synchronisation per batch.  The loss functions here take such ``[..., 5]`` tensors
(``stats_from_logits`` makes one from logits, on any device) and return what the reference's functions return on the logits themselves.

Accepted images: [B, 3, H, W] with H and W multiples of 16 in [32, 512].  Only ``activation_fn="leaky_relu"`` is built.  There is no CPU path
for the network.  Not verified against the reference's ``VQGANLoss`` class itself (its constructor needs torchvision) nor with a trained
discriminator checkpoint: the network is tested against the reference's ``NLayerDiscriminatorv2`` and ``gan_utils`` on seeded weights.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Optional, Text, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .base_model import BaseModel, _init_tensor

LOGIT_SIDE = 16
NUM_LOGITS = LOGIT_SIDE * LOGIT_SIDE
NUM_STATS = 5
MIN_SIDE, MAX_SIDE, SIDE_STEP = 32, 512, 16
MAX_STAGES, MAX_CHANNELS = 4, 2048
BLUR_KERNEL_MAP = {3: (1, 2, 1), 4: (1, 3, 3, 1), 5: (1, 4, 6, 4, 1)}


def blur_kernel(size: int) -> torch.Tensor:
    """BlurBlock's buffer [1, 1, k, k]: the binomial row outer-squared over its sum (exact in fp32)"""
    row = torch.tensor(BLUR_KERNEL_MAP[size], dtype=torch.float32)
    k = row[None, :] * row[:, None]
    return (k / k.sum())[None, None]


def discriminator_keys(num_stages: int = 3, blur_resample: bool = True) -> List[str]:
    """the reference module's state-dict keys in order"""
    keys = ["block_in.0.weight", "block_in.0.bias"]
    for i in range(num_stages):
        keys += [f"blocks.{i}.0.weight", f"blocks.{i}.0.bias"]
        if blur_resample:
            keys.append(f"blocks.{i}.1.kernel")
        keys += [f"blocks.{i}.2.weight", f"blocks.{i}.2.bias"]
    return keys + ["to_logits.0.weight", "to_logits.0.bias", "to_logits.2.weight", "to_logits.2.bias"]


class NLayerDiscriminatorv2(BaseModel):
    _ABI = "disc"
    _COUNTS = "activation groups (4 channels of a convolution, 8 of a GroupNorm) clamped"
    max_images_per_call = 8               # workspace bound: 44 MiB of fp16 activations per 256 x 256 image at hidden 128

    def __init__(self, num_channels: int = 3, hidden_channels: int = 128, num_stages: int = 3, activation_fn: str = "leaky_relu",
                 blur_resample: bool = False, blur_kernel_size: int = 4):
        super().__init__()
        assert num_stages > 0, "Discriminator cannot have 0 stages"
        assert (not blur_resample) or (blur_kernel_size >= 3 and blur_kernel_size <= 5), "Blur kernel size must be in [3,5] when sampling]"
        if activation_fn != "leaky_relu":
            raise NotImplementedError(f"NLayerDiscriminatorv2: activation_fn={activation_fn!r}: the HIP path takes 'leaky_relu' (slope 0.1), the "
                                      "activation of every shipped config; SiLU is not built")
        if num_channels != 3:
            raise ValueError(f"NLayerDiscriminatorv2: num_channels={num_channels}: the HIP path takes 3 (RGB images)")
        if hidden_channels < 32 or hidden_channels % 32:
            raise ValueError(f"NLayerDiscriminatorv2: hidden_channels={hidden_channels}: the HIP path takes multiples of 32 (GroupNorm has 32 groups)")
        if num_stages > MAX_STAGES or (hidden_channels << (num_stages - 1)) > MAX_CHANNELS:
            raise ValueError(f"NLayerDiscriminatorv2: {num_stages} stages from {hidden_channels} channels: the HIP path takes up to {MAX_STAGES} "
                             f"stages and {MAX_CHANNELS} channels in the last")
        self.num_channels, self.hidden_channels, self.num_stages = int(num_channels), int(hidden_channels), int(num_stages)
        self.blur_kernel_size = int(blur_kernel_size) if blur_resample else 0
        h = self.hidden_channels
        mult = (1,) + tuple(2 ** t for t in range(num_stages))
        self._attach("block_in.0.weight", _init_tensor((h, 3, 5, 5), "kaiming"))
        self._attach("block_in.0.bias", torch.zeros(h))
        for i in range(num_stages):
            cin, cout = h * mult[i], h * mult[i + 1]
            self._attach(f"blocks.{i}.0.weight", _init_tensor((cout, cin, 3, 3), "kaiming"))
            self._attach(f"blocks.{i}.0.bias", torch.zeros(cout))
            if blur_resample:
                self._attach(f"blocks.{i}.1.kernel", blur_kernel(self.blur_kernel_size), buffer=True)
            self._attach(f"blocks.{i}.2.weight", torch.ones(cout))
            self._attach(f"blocks.{i}.2.bias", torch.zeros(cout))
        c = h * mult[-1]
        self._attach("to_logits.0.weight", _init_tensor((c, c, 1, 1), "kaiming"))
        self._attach("to_logits.0.bias", torch.zeros(c))
        self._attach("to_logits.2.weight", _init_tensor((1, c, 5, 5), "kaiming"))
        self._attach("to_logits.2.bias", torch.zeros(1))
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    # ---- engine hooks ---------------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        h = C.c_void_p()
        _lib.check(_lib.load().mb_disc_create(capacity, self.hidden_channels, self.num_stages, self.blur_kernel_size, C.byref(h)), "mb_disc_create")
        return h

    @staticmethod
    def check_images(shape) -> None:
        """``ValueError`` for what the engine does not take; no device work."""
        if len(shape) != 4:
            raise ValueError(f"NLayerDiscriminatorv2 expects a [B, 3, H, W] batch, got {tuple(shape)}")
        B, Cc, H, W = (int(v) for v in shape)
        if B < 1:
            raise ValueError(f"NLayerDiscriminatorv2: empty batch {tuple(shape)}")
        if Cc != 3:
            raise ValueError(f"NLayerDiscriminatorv2 takes 3 channels, got {Cc}")
        if not all(MIN_SIDE <= n <= MAX_SIDE and n % SIDE_STEP == 0 for n in (H, W)):
            raise ValueError(f"NLayerDiscriminatorv2: images of {H} x {W}: the HIP engine takes H and W that are multiples of {SIDE_STEP} in "
                             f"[{MIN_SIDE}, {MAX_SIDE}]")

    def _run(self, x: torch.Tensor, clamp: bool, want_logits: bool, want_stats: bool, running_sum: Optional[torch.Tensor] = None):
        self.check_images(x.shape)
        dev = self._require_cuda("forward")
        B, _, H, W = (int(v) for v in x.shape)
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        have = self._engine_key[1] if self._engine_key else 0
        h = self._ensure_engine(max(int(self.max_images_per_call), have))
        logits = torch.empty((B, 1, LOGIT_SIDE, LOGIT_SIDE), dtype=torch.float32, device=dev) if want_logits else None
        stats = torch.empty((B, NUM_STATS), dtype=torch.float64, device=dev) if want_stats or running_sum is not None else None
        with torch.cuda.device(dev):
            rc = _lib.load().mb_disc_forward(h, x.data_ptr(), B, H, W, 1 if clamp else 0, logits.data_ptr() if want_logits else None,
                                             stats.data_ptr() if stats is not None else None,
                                             running_sum.data_ptr() if running_sum is not None else None, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "mb_disc_forward")
        return logits, stats

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The logits, fp32 [B, 1, 16, 16].  No synchronisation."""
        return self._run(x, False, True, False)[0]

    @torch.no_grad()
    def logit_stats(self, x: torch.Tensor, clamp: bool = False, running_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per image the five sums over its logits, float64 [B, 5] on the device (``clamp=True``: the images clamped to [0, 1] on the load;
        ``running_sum``: a float64 [5] device tensor the batch's sums are added to, in image order).  An image's row does not depend on the
        batch.  No synchronisation."""
        if running_sum is not None and (running_sum.dtype != torch.float64 or running_sum.numel() != NUM_STATS or not running_sum.is_contiguous()):
            raise ValueError("logit_stats: running_sum must be a contiguous float64 tensor of 5 values")
        return self._run(x, clamp, False, True, running_sum)[1]


def create_discriminator(discriminator_config) -> torch.nn.Module:
    """The reference's ``gan_utils.create_discriminator``: ``"VQGAN+Discriminator"`` -> ``NLayerDiscriminatorv2``.  ``"Original"`` (the Taming
    PatchGAN, whose BatchNorm runs on batch statistics in training mode) is not built."""
    if discriminator_config.name == "Original":
        raise NotImplementedError("create_discriminator: the 'Original' PatchGAN discriminator is out of scope here -- only the "
                                  "'VQGAN+Discriminator' that the MaskBit and VQGAN+ tokenizer configs use is built on the HIP path")
    if discriminator_config.name == "VQGAN+Discriminator":
        return NLayerDiscriminatorv2(num_channels=discriminator_config.num_channels, num_stages=discriminator_config.num_stages,
                                     hidden_channels=discriminator_config.hidden_channels, blur_resample=discriminator_config.blur_resample,
                                     blur_kernel_size=discriminator_config.get("blur_kernel_size", 4))
    raise ValueError(f"Discriminator {discriminator_config.name} is not implemented.")


# ---- gan_utils, as functions of the five sums ------------------------------------------------------------------------------------------------
def stats_from_logits(logits: torch.Tensor) -> torch.Tensor:
    """logits [B, ...] with 256 values per image -> the float64 [B, 5] sums ``logit_stats`` gives (softplus in the overflow-safe form)"""
    l = logits.detach().double().reshape(logits.shape[0], -1)
    if l.shape[1] != NUM_LOGITS:
        raise ValueError(f"stats_from_logits: {l.shape[1]} logits per image, the discriminator gives {NUM_LOGITS}")
    sp = lambda v: v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))                                # noqa: E731
    return torch.stack([l.sum(1), (1 - l).clamp(min=0).sum(1), (1 + l).clamp(min=0).sum(1), sp(-l).sum(1), sp(l).sum(1)], dim=1)


def _mean(stats: torch.Tensor, k: int) -> torch.Tensor:
    if stats.shape[-1] != NUM_STATS:
        raise ValueError(f"a stats tensor ends in {NUM_STATS} values (logit_stats / stats_from_logits), got {tuple(stats.shape)}")
    return stats[..., k].double().sum() / float(stats.numel() // NUM_STATS * NUM_LOGITS)


def logits_mean(stats: torch.Tensor) -> torch.Tensor:
    """``torch.mean(logits)`` of the images the rows stand for"""
    return _mean(stats, 0)


def adopt_weight(weight: float, global_step: int, threshold: int = 0, value: float = 0.0) -> float:
    """If global_step is less than threshold, return value, else return weight."""
    if global_step < threshold:
        weight = value
    return weight


def compute_lecam_loss(logits_real_mean: torch.Tensor, logits_fake_mean: torch.Tensor, ema_logits_real_mean: torch.Tensor,
                       ema_logits_fake_mean: torch.Tensor) -> torch.Tensor:
    lecam_loss = torch.mean(torch.pow(F.relu(logits_real_mean - ema_logits_fake_mean), 2))
    lecam_loss = lecam_loss + torch.mean(torch.pow(F.relu(ema_logits_real_mean - logits_fake_mean), 2))
    return lecam_loss


def hinge_g_loss(stats_fake: torch.Tensor) -> torch.Tensor:
    return -_mean(stats_fake, 0)


def hinge_d_loss(stats_real: torch.Tensor, stats_fake: torch.Tensor) -> torch.Tensor:
    return 0.5 * (_mean(stats_real, 1) + _mean(stats_fake, 2))


def vanilla_d_loss(stats_real: torch.Tensor, stats_fake: torch.Tensor) -> torch.Tensor:
    return 0.5 * (_mean(stats_real, 3) + _mean(stats_fake, 4))


def non_saturating_d_loss(stats_real: torch.Tensor, stats_fake: torch.Tensor) -> torch.Tensor:
    # sigmoid cross entropy with label 1 is softplus(-x), with label 0 softplus(x)
    return _mean(stats_real, 3) + _mean(stats_fake, 4)


def non_saturating_g_loss(stats_fake: torch.Tensor) -> torch.Tensor:
    return _mean(stats_fake, 3)


D_LOSSES = {"hinge": hinge_d_loss, "vanilla": vanilla_d_loss, "non-saturating": non_saturating_d_loss}
G_LOSSES = {"hinge": hinge_g_loss, "vanilla": hinge_g_loss, "non-saturating": non_saturating_g_loss}      # losses.py:73-78


class VQGANLoss(torch.nn.Module):
    """The reference's ``VQGANLoss`` for held-out scoring: the same submodule names (``discriminator``, ``perceptual_loss``), buffers, asserts,
    defaults, keys and arithmetic, under ``no_grad``.  Results are fp32 tensors as in the reference (the sums behind them are float64).
    ``discriminator_gradient_penalty="adopt_weight"`` needs autograd through the decoder and raises ``NotImplementedError`` at construction."""

    def __init__(self, discriminator_config, loss_config):
        super().__init__()
        assert loss_config.discriminator_loss in ("hinge", "vanilla", "non-saturating")
        assert loss_config.reconstruction_loss in ("l2", "l1")
        assert loss_config.discriminator_gradient_penalty in ("none", "adopt_weight")
        if loss_config.discriminator_gradient_penalty == "adopt_weight":
            raise NotImplementedError("VQGANLoss: discriminator_gradient_penalty='adopt_weight' needs gradients through the decoder's last layer; "
                                      "this inference-only module takes 'none' (what every shipped config has)")
        from .perceptual import create_perception_loss
        self.discriminator = create_discriminator(discriminator_config)
        self.reconstruction_loss = loss_config.reconstruction_loss
        self.reconstruction_weight = loss_config.get("reconstruction_weight", 1.0)
        self.quantizer_weight = loss_config.quantizer_weight
        self.perceptual_loss = create_perception_loss(loss_config.perceptual_loss, loss_config.get("perceptual_loss_on_logits", True))
        self.perceptual_weight = loss_config.perceptual_weight
        self.lecam_regularization_weight = loss_config.lecam_regularization_weight
        self.ema_decay = loss_config.get("ema_decay", 0.999)
        self.entropy_annealing_steps = loss_config.get("entropy_annealing_steps", 2000)
        self.entropy_annealing_factor = loss_config.get("entropy_annealing_factor", 0.0)
        self.discriminator_iter_start = loss_config.discriminator_start
        self.discriminator_loss = D_LOSSES[loss_config.discriminator_loss]
        self.generator_loss = G_LOSSES[loss_config.discriminator_loss]
        self.discriminator_factor = loss_config.discriminator_factor
        self.discriminator_weight = loss_config.discriminator_weight
        self.discriminator_gradient_penalty = ""
        self.discriminator_penalty_cost = loss_config.discriminator_penalty_cost
        if self.lecam_regularization_weight > 0.0:
            self.register_buffer("ema_real_logits_mean", torch.zeros((1)))
            self.register_buffer("ema_fake_logits_mean", torch.zeros((1)))

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """A training run's loss-module checkpoint (``discriminator.*``, ``perceptual_loss.*``, the two EMA buffers).  The perceptual
        loss (ResNet-50 or LPIPS) counts as loaded for the networks the checkpoint holds whole."""
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        prefix = "perceptual_loss."
        note = getattr(self.perceptual_loss, "note_loaded_keys", None)      # LPIPS and PerceptualLoss: which of their networks the checkpoint held
        if note is not None:
            note([k[len(prefix):] for k in state_dict if k.startswith(prefix)])
        return res

    def should_discriminator_be_trained(self, global_step: int):
        """Returns if the discriminator should be trained at given step."""
        return global_step >= self.discriminator_iter_start

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor, reconstructions: torch.Tensor, extra_result_dict: Mapping[Text, torch.Tensor], global_step: int,
                last_layer=None, mode: str = "gen", update_ema: bool = True) -> Tuple[torch.Tensor, Mapping[Text, torch.Tensor]]:
        """``(loss, loss_dict)`` of the generator (``mode="gen"``) or the discriminator (``"disc"``) step, as the training loop logs them.
        ``last_layer`` is not used (there is no adaptive weight).  ``mode="disc"`` moves the LeCam EMA buffers as the reference does;
        ``update_ema=False`` leaves them alone, for scoring held-out images."""
        assert mode in ("gen", "disc")
        if mode == "gen":
            return self._forward_generator(inputs, reconstructions, extra_result_dict, global_step)
        return self._forward_discriminator(inputs, reconstructions, global_step, update_ema)

    def _forward_generator(self, inputs, reconstructions, extra_result_dict, global_step):
        inputs = inputs.contiguous()
        reconstructions = reconstructions.contiguous()
        if self.reconstruction_loss == "l1":
            reconstruction_loss = F.l1_loss(inputs, reconstructions, reduction="mean")
        else:
            reconstruction_loss = F.mse_loss(inputs, reconstructions, reduction="mean")
        reconstruction_loss = reconstruction_loss * self.reconstruction_weight
        perceptual_loss = self.perceptual_loss(inputs, reconstructions).mean()
        generator_loss = torch.zeros((), device=inputs.device)
        extra_generator_loss = torch.zeros((), device=inputs.device)
        discriminator_factor = adopt_weight(self.discriminator_factor, global_step, threshold=self.discriminator_iter_start)
        d_weight = 1.0
        if discriminator_factor > 0.0:
            generator_loss = self.generator_loss(self.discriminator.logit_stats(reconstructions)).to(torch.float32)
        d_weight *= self.discriminator_weight
        quantizer_loss = extra_result_dict["quantizer_loss"]
        if self.entropy_annealing_factor > 0.0:            # (the reference adds in place; the caller's tensor is left alone here)
            quantizer_loss = quantizer_loss + (max(0.0, 1 - global_step / self.entropy_annealing_steps)
                                               * self.entropy_annealing_factor * extra_result_dict["entropy_loss"])
        total_loss = (reconstruction_loss + self.perceptual_weight * perceptual_loss + self.quantizer_weight * quantizer_loss
                      + d_weight * discriminator_factor * (generator_loss + extra_generator_loss))
        loss_dict = dict(
            total_loss=total_loss.clone().detach(),
            reconstruction_loss=reconstruction_loss.detach(),
            perceptual_loss=(self.perceptual_weight * perceptual_loss).detach(),
            quantizer_loss=(self.quantizer_weight * quantizer_loss).detach(),
            weighted_gan_loss=(d_weight * discriminator_factor * (generator_loss + extra_generator_loss)).detach(),
            discriminator_factor=torch.tensor(discriminator_factor),
            commitment_loss=extra_result_dict["commitment_loss"].detach(),
            entropy_loss=extra_result_dict["entropy_loss"].detach(),
            per_sample_entropy=extra_result_dict["per_sample_entropy"],
            avg_entropy=extra_result_dict["avg_entropy"],
            d_weight=d_weight,
            gan_loss=generator_loss.detach(),
        )
        if "codebook_loss" in extra_result_dict:
            loss_dict["codebook_loss"] = extra_result_dict["codebook_loss"].detach()
        return total_loss, loss_dict

    def _forward_discriminator(self, inputs, reconstructions, global_step, update_ema):
        discriminator_factor = adopt_weight(self.discriminator_factor, global_step, threshold=self.discriminator_iter_start)
        stats_real = self.discriminator.logit_stats(inputs)
        stats_fake = self.discriminator.logit_stats(reconstructions)
        mean_real = logits_mean(stats_real).to(torch.float32)
        mean_fake = logits_mean(stats_fake).to(torch.float32)
        discriminator_loss = discriminator_factor * self.discriminator_loss(stats_real, stats_fake).to(torch.float32)
        lecam_loss = torch.zeros((), device=inputs.device)
        if self.lecam_regularization_weight > 0.0:
            lecam_loss = compute_lecam_loss(mean_real, mean_fake, self.ema_real_logits_mean, self.ema_fake_logits_mean) * self.lecam_regularization_weight
            if update_ema:
                self.ema_real_logits_mean = self.ema_real_logits_mean * self.ema_decay + mean_real * (1 - self.ema_decay)
                self.ema_fake_logits_mean = self.ema_fake_logits_mean * self.ema_decay + mean_fake * (1 - self.ema_decay)
        discriminator_loss = discriminator_loss + lecam_loss
        loss_dict = dict(discriminator_loss=discriminator_loss.detach(), logits_real=mean_real, logits_fake=mean_fake, lecam_loss=lecam_loss.detach())
        return discriminator_loss, loss_dict
