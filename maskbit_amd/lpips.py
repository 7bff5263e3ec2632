"""LPIPS on the device: the reference's ``modeling.modules.lpips.LPIPS`` (lpips.py:11-52) behind ``csrc/lpips.hip``.

``LPIPS(use_dropout=True)`` has the reference's 33 state-dict entries -- ``scaling_layer.shift`` / ``.scale``, the thirteen VGG16 convolutions
as ``net.slice{1..5}.{N}.weight`` / ``.bias`` (N = torchvision's ``features`` index) and ``lin{0..4}.model.1.weight`` (``model.0`` without
dropout) -- and ``forward(input, target) -> [B, 1, 1, 1]``.  Inference only; dropout is the identity in evaluation, which is all there is here.

Unlike the reference, construction loads NOTHING: the reference downloads torchvision's ImageNet VGG16 and reads ``pretrained/vgg_lpips.pth``
next to its own sources; neither can ship in this package.  The user hands both over once:

    lpips = LPIPS().to("cuda")
    lpips.load_vgg16("vgg16-397923af.pth")          # torchvision's checkpoint (features.N.*), or the reference layout, or bare N.*
    lpips.load_linear("pretrained/vgg_lpips.pth")   # the reference's file

A forward before both are loaded raises.  ``mb_lpips_forward`` runs the scaling layer, the convolutions (fp16 NHWC on MFMA, both images of a pair
in one batch), the pools and one fused distance kernel per tap; features are stored as fp16, which costs about 0.5 % of the value at LPIPS 5e-5 and
1e-4 of it at 8e-3 (DESIGN.md "Precision"; negligible at the 0.05 - 0.3 of real reconstructions).  Accepted images: [B, 3, H, W] with
H % 128 == 0 and W % 256 == 0 (256^2, 512^2, ...).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib
from .base_model import PairLoss, StateLike, read_state
from .synth import VGG16_CONVS

_SLICE_END = (4, 9, 16, 23, 30)            # lpips.py:94-103: features [0, 4) -> slice1, [4, 9) -> slice2, ...
_TAP_CHANNELS = (64, 128, 256, 512, 512)


def _slice_of(idx: int) -> int:
    return next(k for k, end in enumerate(_SLICE_END) if idx < end) + 1


def vgg16_keys() -> List[str]:
    """the 26 VGG16 entries in the reference layout"""
    return [f"net.slice{_slice_of(i)}.{i}.{p}" for i, _cin, _cout in VGG16_CONVS for p in ("weight", "bias")]


class LPIPS(PairLoss):
    _ABI = "lpips"
    _INPUT = "VGG16"
    _COUNTS = "4-channel activation groups the convolutions clamped (ImageNet VGG16 activations are unnormalised)"
    max_pairs_per_call = 16               # workspace bound at 256 x 256 (two fp16 buffers of 8 MiB per image); scaled down with the image area

    def __init__(self, use_dropout: bool = True):
        super().__init__()
        self.use_dropout = bool(use_dropout)
        self.chns = list(_TAP_CHANNELS)
        self._attach("scaling_layer.shift", torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None], buffer=True)      # lpips.py:58-59
        self._attach("scaling_layer.scale", torch.tensor([0.458, 0.448, 0.450])[None, :, None, None], buffer=True)
        for idx, cin, cout in VGG16_CONVS:
            p = f"net.slice{_slice_of(idx)}.{idx}"
            self._attach(p + ".weight", torch.zeros(cout, cin, 3, 3))
            self._attach(p + ".bias", torch.zeros(cout))
        self._lin_index = 1 if self.use_dropout else 0                                                                   # lpips.py:71-81
        for k, c in enumerate(_TAP_CHANNELS):
            self._attach(f"lin{k}.model.{self._lin_index}.weight", torch.zeros(1, c, 1, 1))
        for p in self.parameters():
            p.requires_grad = False
        self._vgg_loaded = False
        self._lin_loaded = False
        self._cap_hw = (256, 256)
        self.eval()

    # ---- weights ------------------------------------------------------------------------------
    def lin_keys(self) -> List[str]:
        return [f"lin{k}.model.{self._lin_index}.weight" for k in range(5)]

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self.note_loaded_keys(state_dict)
        return res

    def note_loaded_keys(self, keys) -> None:
        keys = set(keys)
        self._vgg_loaded = self._vgg_loaded or all(k in keys for k in vgg16_keys())
        self._lin_loaded = self._lin_loaded or all(k in keys for k in self.lin_keys())

    def load_vgg16(self, path_or_state_dict: StateLike) -> None:
        """The thirteen convolutions from a checkpoint path or state dict in the reference layout (``net.sliceK.N.*``), torchvision's
        (``features.N.*``; its ``classifier.*`` entries are ignored) or a bare ``N.*``.  All 26 entries must be there."""
        src = read_state(path_or_state_dict)
        sd = {}
        for idx, _cin, _cout in VGG16_CONVS:
            for p in ("weight", "bias"):
                own = f"net.slice{_slice_of(idx)}.{idx}.{p}"
                for cand in (own, f"features.{idx}.{p}", f"{idx}.{p}"):
                    if cand in src:
                        sd[own] = src[cand]
                        break
                else:
                    raise KeyError(f"load_vgg16: no entry for VGG16 features.{idx}.{p} (looked for {own}, features.{idx}.{p}, {idx}.{p})")
        super().load_state_dict(sd, strict=False)
        self._vgg_loaded = True

    def load_linear(self, path_or_state_dict: StateLike) -> None:
        """The five 1x1 weight vectors (and the scaling buffers, when present) from the reference's ``pretrained/vgg_lpips.pth``; non-strict, as
        the reference loads it (lpips.py:37).  Either lin index (``model.1`` / ``model.0``) is accepted."""
        src = read_state(path_or_state_dict)
        sd = {k: v for k, v in src.items() if k.startswith("scaling_layer.")}
        for k in range(5):
            for j in (1, 0):
                cand = f"lin{k}.model.{j}.weight"
                if cand in src:
                    sd[f"lin{k}.model.{self._lin_index}.weight"] = src[cand]
                    break
            else:
                raise KeyError(f"load_linear: no entry lin{k}.model.1.weight (or model.0)")
        super().load_state_dict(sd, strict=False)
        self._lin_loaded = True

    # ---- engine hooks ---------------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        h = C.c_void_p()
        _lib.check(_lib.load().mb_lpips_create(capacity, self._cap_hw[0], self._cap_hw[1], C.byref(h)), "mb_lpips_create")
        return h

    def engine(self, pairs: int, H: int, W: int):
        if H * W > self._cap_hw[0] * self._cap_hw[1]:
            self._drop_engine()
            self._cap_hw = (H, W)
        return super().engine(pairs)

    # ---- forward ----------------------------------------------------------------------------------
    @staticmethod
    def _size_error(H: int, W: int) -> Optional[str]:
        if H < 128 or W < 256 or H % 128 or W % 256:
            return "H % 128 == 0 and W % 256 == 0 (whole 8 x 16-pixel convolution tiles at 1/16 resolution), e.g. 256 x 256 or 512 x 512"
        return None

    def _no_weights(self) -> Optional[str]:
        return " and ".join(n for n, ok in (("load_vgg16", self._vgg_loaded), ("load_linear", self._lin_loaded)) if not ok) or None

    def _chunk(self, H: int, W: int) -> int:
        return int(self.max_pairs_per_call) * 65536 // (H * W)

    def _forward_chunk(self, h, a, b, n, H, W, clamp, out, running_sum, stream) -> int:
        return _lib.load().mb_lpips_forward(h, a, b, n, H, W, clamp, out, running_sum, stream)

    @torch.no_grad()
    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self._run(input, target, False).to(torch.float32).view(-1, 1, 1, 1)
