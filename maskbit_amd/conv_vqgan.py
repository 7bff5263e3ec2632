"""MaskBit tokenizer (decoder and encoder) backed by the gfx950 engine.

Call surface of the reference's ``modeling.conv_vqgan.ConvVQModel`` (conv_vqgan.py:40-112):
``ConvVQModel(config)`` with an attribute-style config (+ ``.get``), the reference's checkpoint keys
(``encoder.*``, ``decoder.*``, ``quantize.*``), ``decode_tokens(tokens [b, n]) -> image
[b, 3, H, W]`` float32 unclamped and ``decode(z [b, K, h, w])``.  The decode itself is
``mb_dec_decode``: NHWC fp16 implicit-GEMM convolutions on MFMA with fused GroupNorm+SiLU
prologue, fused nearest-2x upsampling, bias and residual epilogues.

The encoder half (image -> tokens; stage-I plumbing outside the sampling hot path, SURVEY.md 8f
next-1) runs on the same kernels through ``mb_enc_encode``: ``encode(x) -> (z_quantized,
result_dict)`` with ``min_encoding_indices`` and ``forward(x) -> (reconstruction, result_dict)``
(conv_vqgan.py:70-83,114-127), inference only.

Both quantizers of the reference are built: ``quantizer_type="lookup-free"`` (LFQ, the MaskBit tokenizers) and ``"lookup"``
(``SimpleVectorizer``, modeling/quantizer/quantizer.py: the VQGAN+ and MaskGIT tokenizers, a learned codebook
``quantize.embedding.weight`` [codebook_size, token_size], optionally L2-normalised).  The lookup encoder ends in the fused
nearest-codeword search of vq.hip (``mb_enc_encode_vq``), its decoder input is the codebook row gather.  ``legacy=True``
(``ConvDecoderLegacy``, modeling/modules/autoencoder.py:289-353: the MaskGIT checkpoint layout) is a naming switch only: the
same decoder with ``decoder.up.{i}`` holding level ``i`` (0 = finest) and ``num_res_blocks`` everywhere; its keys are
remapped onto the canonical layout when the engine is loaded.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import torch

from . import _lib
from .base_model import ParamSpec
from .tokenizer import TokenizerModel, _ptr


def _cfg_get(config, key, default=None):
    if hasattr(config, "get"):
        try:
            v = config.get(key, default)
            return default if v is None else v
        except TypeError:
            pass
    return getattr(config, key, default)


def _res_block(p: str, cin: int, cout: int) -> List[ParamSpec]:
    s = [(p + ".norm1.weight", (cin,), "ones"), (p + ".norm1.bias", (cin,), "zeros"),
         (p + ".conv1.weight", (cout, cin, 3, 3), "kaiming"),
         (p + ".norm2.weight", (cout,), "ones"), (p + ".norm2.bias", (cout,), "zeros"),
         (p + ".conv2.weight", (cout, cout, 3, 3), "kaiming")]
    if cin != cout:
        s.append((p + ".nin_shortcut.weight", (cout, cout, 1, 1), "kaiming"))
    return s


def _tokenizer_specs(K, hc, mult, R, nrb_enc, nrb_dec, nch, sample_with_conv) -> List[ParamSpec]:
    s: List[ParamSpec] = []
    # ---- encoder (autoencoder.py:230-286)
    emult = (1,) + tuple(mult)
    s.append(("encoder.conv_in.weight", (hc, nch, 3, 3), "kaiming"))
    c = hc
    for lvl in range(R):
        cin, cout = hc * emult[lvl], hc * emult[lvl + 1]
        c = cin
        for r in range(nrb_enc):
            s += _res_block(f"encoder.down.{lvl}.res_blocks.{r}", c, cout)
            c = cout
        if lvl < R - 1 and sample_with_conv:
            s += [(f"encoder.down.{lvl}.down_conv.weight", (cout, cout, 3, 3), "kaiming"), (f"encoder.down.{lvl}.down_conv.bias", (cout,), "zeros")]
    for r in range(nrb_enc):
        s += _res_block(f"encoder.mid.res_blocks.{r}", c, c)
    s += [("encoder.norm_out.weight", (c,), "ones"), ("encoder.norm_out.bias", (c,), "zeros"),
          ("encoder.conv_out.weight", (K, c, 1, 1), "kaiming"), ("encoder.conv_out.bias", (K,), "zeros")]
    # ---- decoder (autoencoder.py:358-397): up.0 is the coarsest level
    dmult = tuple(mult) + (mult[-1],)
    top = hc * mult[R - 1]
    s += [("decoder.conv_in.weight", (top, K, 3, 3), "kaiming"), ("decoder.conv_in.bias", (top,), "zeros")]
    for r in range(nrb_dec):
        s += _res_block(f"decoder.mid.res_blocks.{r}", top, top)
    last = top
    for i, lvl in enumerate(reversed(range(R))):
        cin, cout = hc * dmult[lvl + 1], hc * dmult[lvl]
        c = cin
        for r in range(nrb_dec):
            s += _res_block(f"decoder.up.{i}.res_blocks.{r}", c, cout)
            c = cout
        if lvl > 0:
            s += [(f"decoder.up.{i}.upsample_conv.weight", (cout, cout, 3, 3), "kaiming"), (f"decoder.up.{i}.upsample_conv.bias", (cout,), "zeros")]
        last = cout
    s += [("decoder.norm_out.weight", (last,), "ones"), ("decoder.norm_out.bias", (last,), "zeros"),
          ("decoder.conv_out.weight", (nch, last, 3, 3), "kaiming"), ("decoder.conv_out.bias", (nch,), "zeros")]
    return s


def _legacy_level(key: str, num_resolutions: int) -> str:
    """``decoder.up.{i}.*`` of one layout -> the other (level i <-> stage R-1-i; the map is its own inverse); other keys unchanged."""
    if not key.startswith("decoder.up."):
        return key
    rest = key[len("decoder.up."):]
    i, tail = rest.split(".", 1)
    return f"decoder.up.{num_resolutions - 1 - int(i)}.{tail}"


def legacy_to_canonical(state_dict, num_resolutions: int):
    """A ``legacy=True`` (ConvDecoderLegacy) state dict with its keys renamed to the ``legacy=False`` layout (same tensors)."""
    return {_legacy_level(k, num_resolutions): v for k, v in state_dict.items()}


class ConvVQModel(TokenizerModel):
    _ABI, _DECODE, _DECODE_LATENT, _ENCODE = "dec", "mb_dec_decode", "mb_dec_decode_latent", "mb_enc_encode_vq"
    _COUNTS = ("4-channel activation groups clamped (the activations are stored as fp16), over every conv layer of decode / encode calls: 0 for "
               "every configuration tested")

    def __init__(self, config, legacy: bool = False, finetune_decoder: bool = False):
        super().__init__()
        qt = _cfg_get(config, "quantizer_type", "lookup-free")
        if qt == "vae":
            raise NotImplementedError("quantizer_type='vae' is not supported (the reference does not implement it either)")
        if qt not in ("lookup-free", "lookup"):
            raise NotImplementedError(f"quantizer_type={qt!r}: only the lookup-free (LFQ) and lookup (VQ) tokenizers are built")
        self.quantizer_type = qt
        self.legacy = bool(legacy)
        self.config = config
        self.finetune_decoder = finetune_decoder
        self.token_size = int(config.token_size)
        self.hidden_channels = int(config.hidden_channels)
        self.channel_mult = tuple(int(v) for v in config.channel_mult)
        self.num_resolutions = int(config.num_resolutions)
        self.num_res_blocks = int(config.num_res_blocks)
        self.num_res_blocks_decoder = self.num_res_blocks if self.legacy else int(_cfg_get(config, "num_res_blocks_decoder", self.num_res_blocks))
        self.num_channels = int(_cfg_get(config, "num_channels", 3))
        self.sample_with_conv = bool(_cfg_get(config, "sample_with_conv", False))
        if qt == "lookup":
            self.codebook_size = int(config.codebook_size)
            if not 1 <= self.token_size <= 256:
                raise ValueError(f"token_size={self.token_size}: the lookup tokenizer supports 1 .. 256 channels")
            if not 2 <= self.codebook_size <= 65536:
                raise ValueError(f"codebook_size={self.codebook_size}: the lookup tokenizer supports 2 .. 65536 entries")
            self.use_l2_normalisation = bool(_cfg_get(config, "use_l2_normalisation", False))
            self.commitment_cost = float(_cfg_get(config, "commitment_cost", 0.25))
        else:
            self.codebook_size = 2 ** self.token_size
        specs = _tokenizer_specs(self.token_size, self.hidden_channels, self.channel_mult, self.num_resolutions,
                                 self.num_res_blocks, self.num_res_blocks_decoder, self.num_channels,
                                 bool(_cfg_get(config, "sample_with_conv", False)))
        if self.legacy:
            specs = [(_legacy_level(k, self.num_resolutions), shape, kind) for k, shape, kind in specs]
        self._build(specs)
        if qt == "lookup":                                                                  # quantizer.py:36-37
            self._attach("quantize.embedding.weight",
                         torch.empty(self.codebook_size, self.token_size).uniform_(-1.0 / self.codebook_size, 1.0 / self.codebook_size))
            return
        weights = (2 ** torch.arange(self.token_size)).to(torch.int32)
        self._attach("quantize.bits_to_indices", weights, buffer=True)                      # lookup_free.py:38-39
        codes = torch.arange(2 ** self.token_size)
        self._attach("quantize.codebook", ((codes[:, None] & weights) != 0).float() * 2.0 - 1.0, buffer=True)   # :41-43

    def get_last_layer(self):
        return self.decoder.conv_out.weight

    # ---- engine hooks ---------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        cfg = _lib.DecCfg()
        cfg.token_size, cfg.hidden_channels = self.token_size, self.hidden_channels
        cfg.num_resolutions, cfg.num_res_blocks, cfg.num_channels = self.num_resolutions, self.num_res_blocks_decoder, self.num_channels
        for i, v in enumerate(self.channel_mult):
            cfg.channel_mult[i] = v
        cfg.latent_size = self._latent_size
        cfg.sample_with_conv = 1 if self.sample_with_conv else 0
        cfg.build_encoder = 1
        cfg.enc_res_blocks = self.num_res_blocks
        h = C.c_void_p()
        if self.quantizer_type == "lookup":
            _lib.check(_lib.load().mb_dec_create_vq(C.byref(cfg), self.codebook_size, 1 if self.use_l2_normalisation else 0, capacity, C.byref(h)),
                       "mb_dec_create_vq")
            return h
        _lib.check(_lib.load().mb_dec_create(C.byref(cfg), capacity, C.byref(h)), "mb_dec_create")
        return h

    def _engine_load(self, h, key: str, t: torch.Tensor, stream: int) -> None:
        if self.legacy:
            key = _legacy_level(key, self.num_resolutions)                  # the engine speaks the canonical layout
        super()._engine_load(h, key, t, stream)

    # ---- shapes -----------------------------------------------------------------------------
    def _grid_side(self, n: int) -> int:
        side = int(math.sqrt(float(n)))
        if side * side != n:
            raise ValueError(f"decode_tokens expects a square token grid, got {n} tokens")
        return side

    def _latent_side(self, h: int, w: int) -> int:
        if h != w or h % 16:
            raise ValueError(f"decode expects a square latent grid with a side that is a multiple of 16, got {h}x{w}")
        return h

    def _image_side(self, H: int, W: int) -> int:
        down = 1 << (self.num_resolutions - 1)
        if H != W or H % (16 * down):
            raise ValueError(f"encode expects square images with a side that is a multiple of {16 * down}, got {H}x{W}")
        return H // down

    # ---- the LFQ branches ---------------------------------------------------------------------
    def _decode_latent(self, z_quantized: torch.Tensor) -> torch.Tensor:
        """Lookup tokenizer: any float latent (ConvDecoder.forward on it, ``mb_dec_decode_latent``).  LFQ: z in {-1,+1} only; LFQ latents are
        exactly the bit pattern of a code, so the latent is re-packed to codes (sign -> bit, LSB first) and decoded through the token path."""
        if self.quantizer_type == "lookup":
            return super()._decode_latent(z_quantized)
        z = z_quantized.to(self._require_cuda("decode"))
        if not bool(((z == 1) | (z == -1)).all()):
            raise ValueError("decode(): the HIP decoder takes quantized LFQ latents (+-1) only")
        w = (2 ** torch.arange(self.token_size, device=z.device)).view(1, -1, 1, 1)
        codes = ((z > 0).long() * w).sum(1).reshape(z.shape[0], -1)
        return self._decode_codes(codes.contiguous())

    def _encode_call(self, h, img, idx, zq, zraw, dist, b: int) -> None:
        if self.quantizer_type == "lookup":
            return super()._encode_call(h, img, idx, zq, zraw, dist, b)
        self._call("mb_enc_encode", h, img.data_ptr(), idx.data_ptr(), zq.data_ptr(), _ptr(zraw), b)

    def _encode(self, x: torch.Tensor, want_raw: bool = False, want_dist: bool = False):
        """-> (zq, idx, zraw), and (zq, idx, zraw, dist) only for a lookup tokenizer asked for the distances"""
        want_dist = want_dist and self.quantizer_type == "lookup"
        out = super()._encode(x, want_raw, want_dist)
        return out if want_dist else out[:3]

    def encode(self, x: torch.Tensor):
        """ConvVQModel.encode (conv_vqgan.py:70-83): image -> (z_quantized [b,K,h,w], result_dict) with ``min_encoding_indices`` [b,h,w].
        LFQ (lookup_free.py:57-95): z_quantized in {-1,+1}; inference only: the quantizer losses are returned as zeros except the commitment
        term, which needs the pre-sign latent and is not computed on this path.  Lookup tokenizer: ``TokenizerModel.encode``."""
        if self.quantizer_type == "lookup":
            return super().encode(x)
        zq, idx, _ = self._encode(x)
        zero = torch.zeros((), device=zq.device)
        return zq, dict(quantizer_loss=zero, commitment_loss=zero, entropy_loss=zero, per_sample_entropy=zero, avg_entropy=zero,
                        min_encoding_indices=idx)
