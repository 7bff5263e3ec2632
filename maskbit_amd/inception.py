"""The FID Inception-v3 on the device: the feature extractor the reference gets from ``metrics.inception.get_inception_model()`` (torch_fidelity's
``FeatureExtractorInceptionV3``: pytorch-fid's ``pt_inception-2015-12-05-6726825d.pth``), behind ``csrc/inception.hip``.

    net = get_inception_model("pt_inception-2015-12-05-6726825d.pth").to("cuda")     # or InceptionV3(...); load_weights(...)
    out = net(images_uint8)                       # {"2048": [B, 2048], "logits_unbiased": [B, 1008]} fp32 on the device, no synchronisation
    evaluator.use_inception(net, real_statistics)

Construction loads NOTHING and never touches the network: the reference downloads the checkpoint through ``torch_fidelity``; here the user hands
the file (or a state dict with its keys) over once.  A forward before that raises.  The architecture is the one written out in DESIGN.md
"Inception-v3" -- the reference only names the blocks, and ``torch_fidelity`` is not available where this project is built, so the network has
NOT been compared against the real thing: tests hold it to a float64 restatement of that specification on seeded weights.

``forward`` takes uint8 ``[B, 3, H, W]`` of any H, W >= 2 (resized to 299 x 299 inside the input kernel) and returns the keys of ``features_list``
(``'64'``, ``'192'``, ``'768'``, ``'2048'``, ``'logits_unbiased'``, ``'logits'``, and ``'spatial'``: fp32 ``[B, 2023]``, the first 7 channels of
``Mixed_6d.branch1x1`` after BatchNorm and ReLU on the 17 x 17 map in (h, w, c) order -- ADM's sFID tap ``mixed_6/conv:0``[..., :7] as far as it can
be told without the TensorFlow graph, DESIGN.md "sFID").  Activations are fp16 with fp32 accumulation where the reference runs
float64; what that costs is stated in DESIGN.md "Precision" and measured in profiles/inception.md.  A row is bitwise independent of the batch it
sits in and of the chunking.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from .base_model import BaseModel, StateLike, read_state
from .synth import INCEPTION_FC, inception_convs

WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"
WEIGHTS_ENV = "MASKBIT_INCEPTION_WEIGHTS"
FEATURE_KEYS = ("64", "192", "768", "2048", "logits_unbiased", "logits", "spatial")
SPATIAL_WIDTH = 17 * 17 * 7              # the sFID tap: Mixed_6d.branch1x1[..., :7] on the 17 x 17 map, (h, w, c) order
FEATURE_WIDTH = {"64": 64, "192": 192, "768": 768, "2048": 2048, "logits_unbiased": INCEPTION_FC[0], "logits": INCEPTION_FC[0],
                 "spatial": SPATIAL_WIDTH}
DEFAULT_FEATURES = ("2048", "logits_unbiased")
_BN = ("weight", "bias", "running_mean", "running_var")


def inception_keys() -> List[str]:
    """the 472 entries of the checkpoint that the network reads"""
    keys = []
    for name, *_ in inception_convs():
        keys.append(f"{name}.conv.weight")
        keys += [f"{name}.bn.{p}" for p in _BN]
    return keys + ["fc.weight", "fc.bias"]


class InceptionV3(BaseModel):
    _ABI = "inception"
    _COUNTS = "4-channel activation groups the convolutions clamped"
    max_images_per_call = 32              # workspace bound: 5.5 MiB of fp16 activations per image

    def __init__(self, features_list: Sequence[str] = DEFAULT_FEATURES):
        super().__init__()
        self.features_list = [str(k) for k in features_list]
        bad = [k for k in self.features_list if k not in FEATURE_KEYS]
        if bad or not self.features_list:
            raise ValueError(f"InceptionV3: unknown features {bad}; supported: {list(FEATURE_KEYS)}")
        for name, cin, cout, (kh, kw), _stride, _pad in inception_convs():
            self._attach_convbn(name + ".conv", name + ".bn", (cout, cin, kh, kw), counter=False)
        self._attach("fc.weight", torch.zeros(*INCEPTION_FC))
        self._attach("fc.bias", torch.zeros(INCEPTION_FC[0]))
        for p in self.parameters():
            p.requires_grad = False
        self._loaded = False
        self.eval()

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: v for k, v in dict(state_dict).items() if not k.endswith(".num_batches_tracked")}
        res = super().load_state_dict(sd, strict=strict, **kw)
        self._loaded = self._loaded or all(k in sd for k in inception_keys())
        return res

    def load_weights(self, path_or_state_dict: StateLike) -> None:
        """The checkpoint from a path or a state dict with the keys of ``pt_inception-2015-12-05-6726825d.pth``.  All 472 entries must be there;
        ``num_batches_tracked`` and entries the network does not read (the auxiliary classifier's) are ignored."""
        src = read_state(path_or_state_dict)
        missing = [k for k in inception_keys() if k not in src]
        if missing:
            raise KeyError(f"load_weights: {len(missing)} entries missing, e.g. {missing[:3]}")
        super().load_state_dict({k: src[k] for k in inception_keys()}, strict=True)
        self._loaded = True

    # ---- engine hooks ---------------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        h = C.c_void_p()
        _lib.check(_lib.load().mb_inception_create(capacity, C.byref(h)), "mb_inception_create")
        return h

    def engine(self, images: int):
        have = self._engine_key[1] if self._engine_key else 0
        return self._ensure_engine(max(images, have))

    # ---- forward ----------------------------------------------------------------------------------
    @staticmethod
    def check_images(x) -> None:
        """``ValueError`` / ``TypeError`` for what the engine does not take; no device work."""
        if not torch.is_tensor(x):
            raise TypeError(f"InceptionV3 takes a uint8 tensor [B, 3, H, W], got {type(x).__name__}")
        if x.dtype != torch.uint8:
            raise ValueError(f"InceptionV3 takes uint8 images in [0, 255] (the reference's contract), got {x.dtype}")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"InceptionV3 takes [B, 3, H, W], got {tuple(x.shape)}")
        B, _, H, W = (int(v) for v in x.shape)
        if B < 1 or H < 2 or W < 2 or H > 16384 or W > 16384:
            raise ValueError(f"InceptionV3: batch of {tuple(x.shape)}: B >= 1 and 2 <= H, W <= 16384")

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        self.check_images(x)
        if not self._loaded:
            raise RuntimeError(f"InceptionV3 has no weights yet: call load_weights(path to {WEIGHTS_FILE}) first (nothing is loaded at construction)")
        dev = self._require_cuda("forward")
        B, _, H, W = (int(v) for v in x.shape)
        x = x.to(dev).contiguous()
        chunk = max(1, min(B, int(self.max_images_per_call)))
        h = self.engine(chunk)
        out = {k: torch.empty(B, FEATURE_WIDTH[k], dtype=torch.float32, device=dev) for k in self.features_list}
        lib = _lib.load()
        taps = any(k in out for k in ("64", "192", "768"))
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for b0 in range(0, B, chunk):
                n = min(chunk, B - b0)
                ptr = {k: (out[k][b0:b0 + n].data_ptr() if k in out else None) for k in FEATURE_KEYS}
                src = x[b0:b0 + n].data_ptr()
                if taps:
                    _lib.check(lib.mb_inception_taps(h, src, n, H, W, None, None, None, None, ptr["64"], ptr["192"], ptr["768"], ptr["2048"],
                                                     ptr["logits_unbiased"], ptr["logits"], stream), "mb_inception_taps")
                    if "spatial" in out:   # the pooled taps and the spatial one together: a second pass for the latter alone
                        _lib.check(lib.mb_inception_forward_spatial(h, src, n, H, W, ptr["spatial"], None, None, None, stream),
                                   "mb_inception_forward_spatial")
                elif "spatial" in out:
                    _lib.check(lib.mb_inception_forward_spatial(h, src, n, H, W, ptr["spatial"], ptr["2048"], ptr["logits_unbiased"], ptr["logits"],
                                                                stream), "mb_inception_forward_spatial")
                else:
                    _lib.check(lib.mb_inception_forward(h, src, n, H, W, ptr["2048"], ptr["logits_unbiased"], ptr["logits"], stream), "mb_inception_forward")
        return out


def get_inception_model(weights: Optional[StateLike] = None) -> InceptionV3:
    """The reference's ``get_inception_model()``: an ``InceptionV3`` with ``features_list = ["2048", "logits_unbiased"]``, loaded from ``weights``
    (a path or a state dict), else from the file the environment variable ``MASKBIT_INCEPTION_WEIGHTS`` names.  Nothing is ever downloaded:
    without either it raises with the name of the file to fetch.  Move the result to the GPU with ``.to("cuda")``."""
    if weights is None:
        weights = os.environ.get(WEIGHTS_ENV) or None
    if weights is None:
        raise RuntimeError(f"get_inception_model: no weights given. Pass the path of pytorch-fid's {WEIGHTS_FILE} (or a state dict with its keys), or "
                           f"set {WEIGHTS_ENV} to that path; this package downloads nothing.")
    m = InceptionV3(list(DEFAULT_FEATURES))
    m.load_weights(weights)
    return m
