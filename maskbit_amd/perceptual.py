"""The ResNet-50 perceptual loss on the device: the reference's ``modeling.modules.perceptual_loss.PerceptualLoss`` (the ``perceptual_loss:
"resnet50"`` of every MaskBit / VQGAN+ tokenizer config, reached through ``losses.create_perception_loss``) behind ``csrc/resnet.hip``.

``PerceptualLoss("resnet50", compute_perceptual_loss_on_logits=True)`` has the reference module's state-dict keys -- ``mean``, ``std`` and
``model.`` + torchvision's ``resnet50`` keys, the ``num_batches_tracked`` counters included, so the ``perceptual_loss.*`` entries of a reference
``VQGANLoss`` checkpoint load strictly -- and ``forward(input, target) -> scalar``.  Inference only: no gradients.

Unlike the reference, construction loads NOTHING: the reference downloads torchvision's ImageNet weights, which cannot ship in this package.  The
user hands them over once:

    loss = PerceptualLoss().to("cuda")
    loss.load_resnet50("resnet50-0676ba61.pth")      # torchvision's checkpoint (conv1.weight, ...), or the reference layout (model.conv1.weight, ...)

A forward before that raises.  ``mb_resnet_forward`` resizes both images to 224 x 224 (bilinear, antialiased) and normalises them in one input
kernel, runs the 2B images as one batch (fp16 NHWC activations, fp32 accumulation on MFMA) and reduces the logits (and, with
``compute_perceptual_loss_on_logits=False``, the ``layer4`` maps) in one float64 distance kernel.  The architecture is the one written out in
DESIGN.md "ResNet-50"; torchvision is not available where this project is built, so the network has NOT been compared with the real checkpoint
or with the reference module: tests hold it to a float64 restatement of that specification on seeded weights.  Accepted images:
[B, 3, H, W] with 32 <= H, W <= 1024.  ``convnext_s`` is not built.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _lib
from .base_model import PairLoss, StateLike, read_state
from .synth import RESNET50_FC, resnet50_convs

_BN = ("weight", "bias", "running_mean", "running_var")
MIN_SIDE, MAX_SIDE = 32, 1024
WEIGHTS_FILE = "resnet50-0676ba61.pth"


def resnet50_keys(counters: bool = True) -> List[str]:
    """torchvision's resnet50 state-dict keys in order (320; without the ``num_batches_tracked`` counters 267)"""
    keys = []
    for conv, bn, *_ in resnet50_convs():
        keys.append(conv + ".weight")
        keys += [f"{bn}.{p}" for p in _BN]
        if counters:
            keys.append(bn + ".num_batches_tracked")
    return keys + ["fc.weight", "fc.bias"]


def perceptual_keys() -> List[str]:
    """the reference module's state-dict keys: its two buffers, then the network under ``model.``"""
    return ["mean", "std"] + ["model." + k for k in resnet50_keys()]


class PerceptualLoss(PairLoss):
    _ABI = "resnet"
    _INPUT = "ResNet-50"
    _COUNTS = "4-channel activation groups the convolutions clamped"
    max_pairs_per_call = 16               # workspace bound: 10.7 MiB of fp16 activations per image, two images per pair

    def __init__(self, model_name: str = "resnet50", compute_perceptual_loss_on_logits: bool = True):
        super().__init__()
        if model_name == "convnext_s":
            raise NotImplementedError("PerceptualLoss('convnext_s'): ConvNeXt-S is out of scope here -- only the 'resnet50' network that the "
                                      "MaskBit and VQGAN+ tokenizer configs use is built on the HIP path")
        if model_name != "resnet50":
            raise ValueError(f"PerceptualLoss: unknown model {model_name!r} (the reference has 'resnet50' and 'convnext_s'; 'resnet50' is built)")
        self.model_name = model_name
        self.compute_perceptual_loss_on_logits = bool(compute_perceptual_loss_on_logits)
        self._attach("mean", torch.tensor([0.485, 0.456, 0.406])[None, :, None, None], buffer=True)        # perceptual_loss.py:33-34
        self._attach("std", torch.tensor([0.229, 0.224, 0.225])[None, :, None, None], buffer=True)
        for conv, bn, cin, cout, k, _stride in resnet50_convs():
            self._attach_convbn("model." + conv, "model." + bn, (cout, cin, k, k), counter=True)
        self._attach("model.fc.weight", torch.zeros(*RESNET50_FC))
        self._attach("model.fc.bias", torch.zeros(RESNET50_FC[0]))
        for p in self.parameters():
            p.requires_grad = False
        self._loaded = False
        self.eval()

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self.note_loaded_keys(state_dict)
        return res

    def note_loaded_keys(self, keys) -> None:
        keys = set(keys)
        self._loaded = self._loaded or all("model." + k in keys for k in resnet50_keys(counters=False))

    def load_resnet50(self, path_or_state_dict: StateLike) -> None:
        """The network from a checkpoint path or a state dict in torchvision's layout (``conv1.weight``, ...) or the reference's
        (``model.conv1.weight``, ...).  All 267 weight and BatchNorm entries must be there; the ``num_batches_tracked`` counters and the
        ``mean`` / ``std`` buffers are taken when present."""
        src = read_state(path_or_state_dict)
        sd: Dict[str, torch.Tensor] = {}
        missing = []
        for k in resnet50_keys():
            for cand in ("model." + k, k):
                if cand in src:
                    sd["model." + k] = src[cand]
                    break
            else:
                if not k.endswith(".num_batches_tracked"):
                    missing.append(k)
        if missing:
            raise KeyError(f"load_resnet50: {len(missing)} entries missing, e.g. {missing[:3]} (looked for them with and without 'model.')")
        sd.update({k: src[k] for k in ("mean", "std") if k in src})
        super().load_state_dict(sd, strict=False)
        self._loaded = True

    # ---- engine hooks ---------------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        h = C.c_void_p()
        _lib.check(_lib.load().mb_resnet_create(capacity, C.byref(h)), "mb_resnet_create")
        return h

    # ---- forward ----------------------------------------------------------------------------------
    @staticmethod
    def _size_error(H: int, W: int) -> Optional[str]:
        return None if MIN_SIDE <= H <= MAX_SIDE and MIN_SIDE <= W <= MAX_SIDE else f"{MIN_SIDE} <= H, W <= {MAX_SIDE}"

    def _no_weights(self) -> Optional[str]:
        return None if self._loaded else f"load_resnet50(path to torchvision's {WEIGHTS_FILE})"

    def _forward_chunk(self, h, a, b, n, H, W, clamp, out, running_sum, stream) -> int:
        return _lib.load().mb_resnet_forward(h, a, b, n, H, W, clamp, 1 if self.compute_perceptual_loss_on_logits else 0, out, running_sum, stream)

    @torch.no_grad()
    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """The reference's scalar: ``mse_loss(..., reduction="mean")`` over the batch = the mean of the per-pair values, fp32."""
        return self._run(input, target, False).mean().to(torch.float32)


def create_perception_loss(perception_loss: str, compute_on_logits: bool = True) -> torch.nn.Module:
    """The reference's ``losses.create_perception_loss``: ``"lpips"`` -> ``LPIPS``, ``"resnet50"`` -> ``PerceptualLoss`` (``"convnext_s"`` raises
    ``NotImplementedError``).  Neither has weights yet: load them (``load_vgg16`` + ``load_linear``, ``load_resnet50``) and move the module to the GPU."""
    if perception_loss == "lpips":
        from .lpips import LPIPS
        return LPIPS().eval()
    if perception_loss in ("resnet50", "convnext_s"):
        return PerceptualLoss(model_name=perception_loss, compute_perceptual_loss_on_logits=compute_on_logits).eval()
    raise ValueError(f"Perception loss {perception_loss} is not supported.")
