"""Taming VQGAN tokenizer backed by the gfx950 engine.

Call surface of the reference's ``modeling.taming_vqgan.OriginalVQModel`` (taming_vqgan.py:19-123): ``OriginalVQModel(config)`` ignores its
argument -- the network is fixed (taming_vqgan.py:26-43) --, the reference's 343 checkpoint keys (``encoder.*``, ``decoder.*``, ``quantize.*``,
``quant_conv.*``, ``post_quant_conv.*``), ``encode(x) -> (z_quantized, result_dict)``, ``decode(z)``, ``decode_tokens(tokens)``,
``forward(x)`` and its own ``load_pretrained``.  Images are in [0, 1]; ``encode`` scales them to [-1, 1] and ``decode`` back, as the reference does.

The whole forward is ``mb_taming_encode`` / ``mb_taming_decode`` / ``mb_taming_decode_latent`` (csrc/taming.hip): the convolution launchers of the
other tokenizers, the spatial self-attention kernel of csrc/spatial_attention.hip for the seven AttnBlocks and the nearest-codeword search of the
lookup tokenizer.  Inference only.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import os
from typing import List, Optional, Union

import torch

from . import _lib
from .base_model import ParamSpec
from .tokenizer import TokenizerModel

CH, CH_MULT, NUM_RES_BLOCKS, Z_CHANNELS = 128, (1, 1, 2, 2, 4), 2, 256
CODEBOOK_SIZE, TOKEN_SIZE, COMMITMENT_COST = 1024, 256, 0.25
ATTN_LEVEL = len(CH_MULT) - 1          # resolution 256 / 2^4 = 16 is the one in attn_resolutions


def _conv(p: str, cout: int, cin: int, k: int) -> List[ParamSpec]:
    return [(p + ".weight", (cout, cin, k, k), "kaiming"), (p + ".bias", (cout,), "zeros")]


def _norm(p: str, c: int) -> List[ParamSpec]:
    return [(p + ".weight", (c,), "ones"), (p + ".bias", (c,), "zeros")]


def _res_block(p: str, cin: int, cout: int) -> List[ParamSpec]:
    s = _norm(p + ".norm1", cin) + _conv(p + ".conv1", cout, cin, 3) + _norm(p + ".norm2", cout) + _conv(p + ".conv2", cout, cout, 3)
    if cin != cout:
        s += _conv(p + ".nin_shortcut", cout, cin, 1)
    return s


def _attn_block(p: str, c: int) -> List[ParamSpec]:
    s = _norm(p + ".norm", c)
    for n in ("q", "k", "v", "proj_out"):
        s += _conv(f"{p}.{n}", c, c, 1)
    return s


def _level(p: str, cin: int, cout: int, nblocks: int, attn: bool) -> List[ParamSpec]:
    s: List[ParamSpec] = []
    for r in range(nblocks):
        s += _res_block(f"{p}.block.{r}", cin if r == 0 else cout, cout)
    if attn:
        for r in range(nblocks):
            s += _attn_block(f"{p}.attn.{r}", cout)
    return s


def _mid(p: str, c: int) -> List[ParamSpec]:
    return _res_block(p + ".block_1", c, c) + _attn_block(p + ".attn_1", c) + _res_block(p + ".block_2", c, c)


def taming_specs() -> List[ParamSpec]:
    """The state dict of OriginalVQModel in the reference's order (Encoder / Decoder of taming_autoencoder.py:176-338)."""
    R = len(CH_MULT)
    top = CH * CH_MULT[-1]
    s = _conv("encoder.conv_in", CH, 3, 3)
    cin = CH
    for l in range(R):
        cout = CH * CH_MULT[l]
        s += _level(f"encoder.down.{l}", cin, cout, NUM_RES_BLOCKS, l == ATTN_LEVEL)
        if l != R - 1:
            s += _conv(f"encoder.down.{l}.downsample.conv", cout, cout, 3)
        cin = cout
    s += _mid("encoder.mid", top) + _norm("encoder.norm_out", top) + _conv("encoder.conv_out", Z_CHANNELS, top, 3)
    s += _conv("decoder.conv_in", top, Z_CHANNELS, 3) + _mid("decoder.mid", top)
    ups = {}
    cin = top
    for l in reversed(range(R)):                                 # built from the coarsest level down, stored with level 0 first
        cout = CH * CH_MULT[l]
        ups[l] = _level(f"decoder.up.{l}", cin, cout, NUM_RES_BLOCKS + 1, l == ATTN_LEVEL)
        if l != 0:
            ups[l] += _conv(f"decoder.up.{l}.upsample.conv", cout, cout, 3)
        cin = cout
    for l in range(R):
        s += ups[l]
    s += _norm("decoder.norm_out", CH) + _conv("decoder.conv_out", 3, CH, 3)
    return s


class OriginalVQModel(TokenizerModel):
    """Images in [0, 1] nominally; ``decode`` takes any float latent [b, 256, h, w] (taming_vqgan.py:52-56), ``_encode`` always returns
    (zq, idx, zraw, dist)."""
    _ABI, _DECODE, _DECODE_LATENT, _ENCODE = "taming", "mb_taming_decode", "mb_taming_decode_latent", "mb_taming_encode"
    _COUNTS = "4-channel activation groups clamped: conv outputs (q, k, v among them), attention outputs and latent packs"
    codebook_size = CODEBOOK_SIZE
    token_size = TOKEN_SIZE
    commitment_cost = COMMITMENT_COST
    num_channels = 3
    num_resolutions = len(CH_MULT)
    quantizer_type = "lookup"

    def __init__(self, config=None):
        super().__init__()
        self.config = config
        self._build(taming_specs())
        self._attach("quantize.embedding.weight",
                     torch.empty(CODEBOOK_SIZE, TOKEN_SIZE).uniform_(-1.0 / CODEBOOK_SIZE, 1.0 / CODEBOOK_SIZE))       # quantizer.py:36-37
        for p in ("quant_conv", "post_quant_conv"):
            self._build(_conv(p, TOKEN_SIZE, Z_CHANNELS, 1))

    def load_pretrained(self, pretrained_model_path: Union[str, os.PathLike], strict_loading: bool = True,
                        torch_dtype: Optional[torch.dtype] = None) -> None:
        """A checkpoint file, or a directory holding ``pytorch_model.bin``; a top-level ``"state_dict"`` is unwrapped and the ``loss.*`` entries
        of the original Taming checkpoints are dropped (taming_vqgan.py:71-123)."""
        path = str(pretrained_model_path)
        if os.path.isdir(path):
            path = os.path.join(path, "pytorch_model.bin")
        if not os.path.isfile(path):
            raise ValueError(f"{path} does not exist")
        ckpt = torch.load(path, map_location="cpu")
        if "state_dict" in ckpt.keys():
            ckpt = ckpt["state_dict"]
        ckpt = {k: copy.deepcopy(v) for k, v in ckpt.items() if not k.startswith("loss.")}
        self.load_state_dict(ckpt, strict=strict_loading)
        if torch_dtype is not None:
            if not isinstance(torch_dtype, torch.dtype):
                raise ValueError(f"{torch_dtype} needs to be of type `torch.dtype`, e.g. `torch.float16`, but is {type(torch_dtype)}.")
            self.to(torch_dtype)
        self.eval()

    # ---- engine hooks ---------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        h = C.c_void_p()
        _lib.check(_lib.load().mb_taming_create(capacity, self._latent_size, C.byref(h)), "mb_taming_create")
        return h

    # ---- shapes -----------------------------------------------------------------------------
    def _grid_side(self, n: int) -> int:
        side = int(math.sqrt(float(n)))
        if side * side != n or side not in (16, 32):
            raise ValueError(f"OriginalVQModel takes 16 x 16 or 32 x 32 token grids (256 x 256 or 512 x 512 images), got {n} tokens")
        return side

    def _latent_side(self, h: int, w: int) -> int:
        if h != w or h not in (16, 32):
            raise ValueError(f"decode expects a 16 x 16 or 32 x 32 latent grid, got {h}x{w}")
        return h

    def _image_side(self, H: int, W: int) -> int:
        if H != W or H not in (256, 512):
            raise ValueError(f"OriginalVQModel takes square images of side 256 or 512, got {H}x{W}")
        return H >> (self.num_resolutions - 1)
