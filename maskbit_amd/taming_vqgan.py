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
from .base_model import BaseModel, ParamSpec

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


class OriginalVQModel(BaseModel):
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
        self._latent_size = 16

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

    def _engine_destroy(self, h) -> None:
        _lib.load().mb_taming_destroy(h)

    def _engine_load(self, h, key: str, t: torch.Tensor, stream: int) -> None:
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(_lib.load().mb_taming_load(h, key.encode(), t.data_ptr(), shape, t.dim(), stream), f"mb_taming_load({key})")

    def engine(self, min_batch: int, latent_size: int = 16):
        if latent_size != self._latent_size:
            self._drop_engine()
            self._latent_size = latent_size
        have = self._engine_key[1] if self._engine_key else 0
        return self._ensure_engine(max(min_batch, have, 8))

    def saturation_count(self, reset: bool = True) -> int:
        """4-channel activation groups the engine clamped at the fp16 range (+-65504) since the last reset: conv outputs (q, k, v among them),
        attention outputs and latent packs of the current engine.  Synchronises the current stream."""
        if self._engine is None:
            return 0
        n = C.c_uint(0)
        dev = self._require_cuda("saturation_count")
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mb_taming_saturation_count(self._engine, C.byref(n), 1 if reset else 0, torch.cuda.current_stream().cuda_stream),
                       "mb_taming_saturation_count")
        return int(n.value)

    # ---- shapes -----------------------------------------------------------------------------
    @staticmethod
    def _latent_side(n: int) -> int:
        side = int(math.sqrt(float(n)))
        if side * side != n or side not in (16, 32):
            raise ValueError(f"OriginalVQModel takes 16 x 16 or 32 x 32 token grids (256 x 256 or 512 x 512 images), got {n} tokens")
        return side

    def _check_codes(self, tokens: torch.Tensor) -> None:
        """Host-resident codes are range-checked (nn.Embedding raises IndexError, quantizer.py:115); device-resident ones are clamped to
        [0, 1024) in the gather kernel, with no host synchronisation."""
        if tokens.device.type == "cpu" and tokens.numel():
            t = tokens.long()
            if int(t.min()) < 0 or int(t.max()) >= CODEBOOK_SIZE:
                raise IndexError(f"code outside [0, {CODEBOOK_SIZE})")

    # ---- decode -----------------------------------------------------------------------------
    def _decode_codes(self, codes: torch.Tensor, want_u8: bool = False):
        if codes.dim() != 2:
            raise ValueError(f"decode_tokens expects tokens [b, n], got {tuple(codes.shape)}")
        side = self._latent_side(codes.shape[1])
        dev = self._require_cuda("decode_tokens")
        b, res = codes.shape[0], side << (self.num_resolutions - 1)
        img = torch.empty((b, 3, res, res), dtype=torch.float32, device=dev)
        u8 = torch.empty((b, res, res, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        h = self.engine(b, side)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mb_taming_decode(h, codes.data_ptr(), img.data_ptr(), u8.data_ptr() if want_u8 else None, b,
                                                    torch.cuda.current_stream().cuda_stream), "mb_taming_decode")
        return (img, u8) if want_u8 else img

    @torch.no_grad()
    def decode_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [b, n] -> image [b, 3, H, W] float32 in [0, 1] nominally, unclamped (taming_vqgan.py:58-64)."""
        if tokens.dim() == 2:
            self._latent_side(tokens.shape[1])
        self._check_codes(tokens)
        dev = self._require_cuda("decode_tokens")
        return self._decode_codes(tokens.to(dev).long().contiguous())

    @torch.no_grad()
    def decode_tokens_uint8(self, tokens: torch.Tensor):
        """-> (image fp32 NCHW, uint8 NHWC = trunc(clamp(x,0,1)*255)) in one pass."""
        if tokens.dim() == 2:
            self._latent_side(tokens.shape[1])
        self._check_codes(tokens)
        dev = self._require_cuda("decode_tokens")
        return self._decode_codes(tokens.to(dev).long().contiguous(), want_u8=True)

    @torch.no_grad()
    def decode(self, z_quantized: torch.Tensor) -> torch.Tensor:
        """z [b, 256, h, w], any float latent -> image (taming_vqgan.py:52-56)."""
        if z_quantized.dim() != 4 or z_quantized.shape[1] != TOKEN_SIZE:
            raise ValueError(f"decode expects [b, {TOKEN_SIZE}, h, w], got {tuple(z_quantized.shape)}")
        b, _, hh, ww = z_quantized.shape
        if hh != ww or hh not in (16, 32):
            raise ValueError(f"decode expects a 16 x 16 or 32 x 32 latent grid, got {hh}x{ww}")
        dev = self._require_cuda("decode")
        z = z_quantized.to(device=dev, dtype=torch.float32).contiguous()
        res = hh << (self.num_resolutions - 1)
        img = torch.empty((b, 3, res, res), dtype=torch.float32, device=dev)
        h = self.engine(b, hh)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mb_taming_decode_latent(h, z.data_ptr(), img.data_ptr(), None, b, torch.cuda.current_stream().cuda_stream),
                       "mb_taming_decode_latent")
        return img

    # ---- encode -----------------------------------------------------------------------------
    @torch.no_grad()
    def _encode(self, x: torch.Tensor, want_raw: bool = False, want_dist: bool = False):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"encode expects [b, 3, H, W], got {tuple(x.shape)}")
        b, _, H, W = x.shape
        if H != W or H not in (256, 512):
            raise ValueError(f"OriginalVQModel takes square images of side 256 or 512, got {H}x{W}")
        dev = self._require_cuda("encode")
        side = H >> (self.num_resolutions - 1)
        img = x.to(device=dev, dtype=torch.float32).contiguous()
        idx = torch.empty((b, side, side), dtype=torch.int64, device=dev)
        zq = torch.empty((b, TOKEN_SIZE, side, side), dtype=torch.float32, device=dev)
        zraw = torch.empty_like(zq) if want_raw else None
        dist = torch.empty((b, side, side), dtype=torch.float32, device=dev) if want_dist else None
        h = self.engine(b, side)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mb_taming_encode(h, img.data_ptr(), idx.data_ptr(), zq.data_ptr(), zraw.data_ptr() if want_raw else None,
                                                    dist.data_ptr() if want_dist else None, b, torch.cuda.current_stream().cuda_stream),
                       "mb_taming_encode")
        return zq, idx, zraw, dist

    def encode(self, x: torch.Tensor):
        """OriginalVQModel.encode (taming_vqgan.py:45-50; SimpleVectorizer.forward in eval mode, quantizer.py:45-103): z_quantized = the selected
        codebook rows; codebook_loss = mean((zq - z)^2) from the kernel's per-row squared distances, commitment_loss = 0.25 * codebook_loss,
        quantizer_loss their sum; the entropy terms are zero, as for the lookup ``ConvVQModel``."""
        zq, idx, _, dist = self._encode(x, want_dist=True)
        codebook_loss = (dist.sum() / float(dist.numel() * TOKEN_SIZE)).reshape(())
        commitment_loss = COMMITMENT_COST * codebook_loss
        zero = torch.zeros((), device=zq.device)
        return zq, dict(quantizer_loss=commitment_loss + codebook_loss, commitment_loss=commitment_loss, codebook_loss=codebook_loss,
                        entropy_loss=zero, per_sample_entropy=zero, avg_entropy=zero, min_encoding_indices=idx)

    def forward(self, input: torch.Tensor):
        """OriginalVQModel.forward (taming_vqgan.py:66-69): (decode(encode(x)), result_dict)."""
        zq, result = self.encode(input)
        codes = result["min_encoding_indices"].reshape(zq.shape[0], -1)
        return self._decode_codes(codes.contiguous()), result
