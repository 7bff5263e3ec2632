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
import os
from typing import Dict, List, Mapping, Optional, Union

import torch

from . import _lib
from .base_model import BaseModel
from .synth import RESNET50_FC, resnet50_convs

StateLike = Union[str, os.PathLike, Mapping[str, torch.Tensor]]
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


class PerceptualLoss(BaseModel):
    _ABI = "resnet"
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
            self._attach(f"model.{conv}.weight", torch.zeros(cout, cin, k, k))
            self._attach(f"model.{bn}.weight", torch.zeros(cout))
            self._attach(f"model.{bn}.bias", torch.zeros(cout))
            self._attach(f"model.{bn}.running_mean", torch.zeros(cout), buffer=True)
            self._attach(f"model.{bn}.running_var", torch.zeros(cout), buffer=True)
            self._attach(f"model.{bn}.num_batches_tracked", torch.zeros((), dtype=torch.int64), buffer=True)
        self._attach("model.fc.weight", torch.zeros(*RESNET50_FC))
        self._attach("model.fc.bias", torch.zeros(RESNET50_FC[0]))
        for p in self.parameters():
            p.requires_grad = False
        self._loaded = False
        self.eval()

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        keys = set(state_dict)
        self._loaded = self._loaded or all("model." + k in keys for k in resnet50_keys(counters=False))
        return res

    def load_resnet50(self, path_or_state_dict: StateLike) -> None:
        """The network from a checkpoint path or a state dict in torchvision's layout (``conv1.weight``, ...) or the reference's
        (``model.conv1.weight``, ...).  All 267 weight and BatchNorm entries must be there; the ``num_batches_tracked`` counters and the
        ``mean`` / ``std`` buffers are taken when present."""
        src = path_or_state_dict
        if isinstance(src, (str, os.PathLike)):
            src = torch.load(os.fspath(src), map_location="cpu")
        src = dict(src)
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

    def engine(self, pairs: int):
        have = self._engine_key[1] if self._engine_key else 0
        return self._ensure_engine(max(pairs, have))

    # ---- forward ----------------------------------------------------------------------------------
    @staticmethod
    def check_images(shape_a, shape_b) -> None:
        """``ValueError`` for what the engine does not take; no device work."""
        if len(shape_a) != 4 or tuple(shape_a) != tuple(shape_b):
            raise ValueError(f"PerceptualLoss expects two [B, 3, H, W] batches of one shape, got {tuple(shape_a)} and {tuple(shape_b)}")
        B, Cc, H, W = (int(v) for v in shape_a)
        if B < 1:
            raise ValueError(f"PerceptualLoss: empty batch {tuple(shape_a)}")
        if Cc != 3:
            raise ValueError(f"PerceptualLoss takes 3 channels (the ResNet-50 input), got {Cc}")
        if not (MIN_SIDE <= H <= MAX_SIDE and MIN_SIDE <= W <= MAX_SIDE):
            raise ValueError(f"PerceptualLoss: images of {H} x {W}: the HIP engine takes {MIN_SIDE} <= H, W <= {MAX_SIDE}")

    def _run(self, a: torch.Tensor, b: torch.Tensor, clamp: bool, running_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
        self.check_images(a.shape, b.shape)
        if not self._loaded:
            raise RuntimeError(f"PerceptualLoss has no weights yet: call load_resnet50(path to torchvision's {WEIGHTS_FILE}) first "
                               "(nothing is loaded at construction)")
        dev = self._require_cuda("forward")
        B, _, H, W = (int(v) for v in a.shape)
        a = a.to(device=dev, dtype=torch.float32).contiguous()
        b = b.to(device=dev, dtype=torch.float32).contiguous()
        chunk = max(1, min(B, int(self.max_pairs_per_call)))
        h = self.engine(chunk)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for b0 in range(0, B, chunk):
                n = min(chunk, B - b0)
                _lib.check(lib.mb_resnet_forward(h, a[b0:b0 + n].data_ptr(), b[b0:b0 + n].data_ptr(), n, H, W, 1 if clamp else 0,
                                                 1 if self.compute_perceptual_loss_on_logits else 0, out[b0:b0 + n].data_ptr(),
                                                 running_sum.data_ptr() if running_sum is not None else None, stream), "mb_resnet_forward")
        return out

    @torch.no_grad()
    def per_image(self, input: torch.Tensor, target: torch.Tensor, clamp: bool = False) -> torch.Tensor:
        """The loss of every pair as float64 [B] on the device (``clamp=True``: both images clamped to [0, 1] inside the input kernel).  Batches
        beyond ``max_pairs_per_call`` are walked in chunks; a pair's value does not depend on the chunking.  No synchronisation."""
        return self._run(input, target, clamp)

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
