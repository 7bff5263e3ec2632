"""What the image tokenizers (``ConvVQModel``, ``OriginalVQModel``) share on top of ``BaseModel``: the engine keyed by the latent side, the decode of
token grids and of float latents, the encode call with its output buffers, the result dict of a lookup quantizer and ``forward``.

A subclass supplies ``_ABI`` and the names of its decode / decode-latent / encode entry points, ``num_channels``, ``num_resolutions``,
``token_size``, ``codebook_size``, ``commitment_cost`` and ``quantizer_type``, and three validators that return a latent side or raise
``ValueError``.  Arguments are checked before the device is asked for: shape, then (host-resident codes of a lookup tokenizer) range, then device.
"""
from __future__ import annotations

import torch

from . import _lib
from .base_model import BaseModel


def _ptr(t):
    return t.data_ptr() if t is not None else None


class TokenizerModel(BaseModel):
    _DECODE = _DECODE_LATENT = _ENCODE = ""           # entry points: tokens -> image, float latent -> image, image -> lookup codes
    _latent_size = 16

    def _grid_side(self, n: int) -> int:
        """Side of a grid of ``n`` tokens."""
        raise NotImplementedError

    def _latent_side(self, h: int, w: int) -> int:
        """Side of an ``h`` x ``w`` latent handed to ``decode``."""
        raise NotImplementedError

    def _image_side(self, H: int, W: int) -> int:
        """Latent side of an ``H`` x ``W`` image handed to ``encode``."""
        raise NotImplementedError

    def engine(self, min_batch: int, latent_size: int = 16):
        if latent_size != self._latent_size:
            self._drop_engine()
            self._latent_size = latent_size
        have = self._engine_key[1] if self._engine_key else 0
        return self._ensure_engine(max(min_batch, have, 8))

    def _call(self, entry: str, *args) -> None:
        """One entry point on the current device and stream; the stream is its last argument."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), entry)(*args, torch.cuda.current_stream().cuda_stream), entry)

    # ---- decode -----------------------------------------------------------------------------
    def _check_codes(self, tokens: torch.Tensor) -> None:
        """Host-resident codes of a lookup tokenizer are range-checked (nn.Embedding raises IndexError, quantizer.py:115); device-resident
        ones are clamped to [0, codebook_size) in the gather kernel, with no host synchronisation."""
        if self.quantizer_type == "lookup" and tokens.device.type == "cpu" and tokens.numel():
            t = tokens.long()
            if int(t.min()) < 0 or int(t.max()) >= self.codebook_size:
                raise IndexError(f"code outside [0, {self.codebook_size})")

    def _decode_codes(self, codes: torch.Tensor, want_u8: bool = False):
        if codes.dim() != 2:
            raise ValueError(f"decode_tokens expects tokens [b, n], got {tuple(codes.shape)}")
        side = self._grid_side(codes.shape[1])
        dev = self._require_cuda("decode_tokens")
        b, res = codes.shape[0], side << (self.num_resolutions - 1)
        img = torch.empty((b, self.num_channels, res, res), dtype=torch.float32, device=dev)
        u8 = torch.empty((b, res, res, self.num_channels), dtype=torch.uint8, device=dev) if want_u8 else None
        self._call(self._DECODE, self.engine(b, side), codes.data_ptr(), img.data_ptr(), _ptr(u8), b)
        return (img, u8) if want_u8 else img

    def _decode_tokens(self, tokens: torch.Tensor, want_u8: bool):
        if tokens.dim() == 2:
            self._grid_side(tokens.shape[1])
        self._check_codes(tokens)
        dev = self._require_cuda("decode_tokens")
        return self._decode_codes(tokens.to(dev).long().contiguous(), want_u8)

    @torch.no_grad()
    def decode_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens [b, n] of any numeric dtype (the sampler hands float32, factorization.py:19) -> image [b, C, H, W] float32, unclamped."""
        return self._decode_tokens(tokens, False)

    @torch.no_grad()
    def decode_tokens_uint8(self, tokens: torch.Tensor):
        """-> (image fp32 NCHW, uint8 NHWC = trunc(clamp(x,0,1)*255)) in one pass (eval_maskbit.py:134-135 fused)."""
        return self._decode_tokens(tokens, True)

    @torch.no_grad()
    def decode(self, z_quantized: torch.Tensor) -> torch.Tensor:
        """z [b, token_size, h, w] -> image: see the subclass's ``_decode_latent``."""
        if z_quantized.dim() != 4 or z_quantized.shape[1] != self.token_size:
            raise ValueError(f"decode expects [b, {self.token_size}, h, w], got {tuple(z_quantized.shape)}")
        return self._decode_latent(z_quantized)

    def _decode_latent(self, z_quantized: torch.Tensor) -> torch.Tensor:
        """Any float latent of a lookup tokenizer: the decoder's forward on it."""
        b, _, hh, ww = z_quantized.shape
        side = self._latent_side(hh, ww)
        dev = self._require_cuda("decode")
        z = z_quantized.to(device=dev, dtype=torch.float32).contiguous()
        res = side << (self.num_resolutions - 1)
        img = torch.empty((b, self.num_channels, res, res), dtype=torch.float32, device=dev)
        self._call(self._DECODE_LATENT, self.engine(b, side), z.data_ptr(), img.data_ptr(), None, b)
        return img

    # ---- encode -----------------------------------------------------------------------------
    def _encode_call(self, h, img, idx, zq, zraw, dist, b: int) -> None:
        self._call(self._ENCODE, h, img.data_ptr(), idx.data_ptr(), zq.data_ptr(), _ptr(zraw), _ptr(dist), b)

    @torch.no_grad()
    def _encode(self, x: torch.Tensor, want_raw: bool = False, want_dist: bool = False):
        """-> (z_quantized [b, K, h, w], indices [b, h, w], the raw latent or None, the rows' squared distances [b, h, w] or None)"""
        if x.dim() != 4 or x.shape[1] != self.num_channels:
            raise ValueError(f"encode expects [b, {self.num_channels}, H, W], got {tuple(x.shape)}")
        b, _, H, W = x.shape
        side = self._image_side(H, W)
        dev = self._require_cuda("encode")
        img = x.to(device=dev, dtype=torch.float32).contiguous()
        idx = torch.empty((b, side, side), dtype=torch.int64, device=dev)
        zq = torch.empty((b, self.token_size, side, side), dtype=torch.float32, device=dev)
        zraw = torch.empty_like(zq) if want_raw else None
        dist = torch.empty((b, side, side), dtype=torch.float32, device=dev) if want_dist else None
        self._encode_call(self.engine(b, side), img, idx, zq, zraw, dist, b)
        return zq, idx, zraw, dist

    def encode(self, x: torch.Tensor):
        """Lookup quantizer (SimpleVectorizer.forward, quantizer.py:45-103, eval mode): -> (z_quantized = the selected codebook rows, L2-normalised
        when configured, result_dict) with ``min_encoding_indices`` [b, h, w]; codebook_loss = mean((zq - z)^2) from the kernel's per-row squared
        distances, commitment_loss = commitment_cost * codebook_loss, quantizer_loss their sum; the entropy terms are zero (the reference computes
        them only in training)."""
        zq, idx, _, dist = self._encode(x, want_dist=True)
        codebook_loss = (dist.sum() / float(dist.numel() * self.token_size)).reshape(())
        commitment_loss = self.commitment_cost * codebook_loss
        zero = torch.zeros((), device=zq.device)
        return zq, dict(quantizer_loss=commitment_loss + codebook_loss, commitment_loss=commitment_loss, codebook_loss=codebook_loss,
                        entropy_loss=zero, per_sample_entropy=zero, avg_entropy=zero, min_encoding_indices=idx)

    def forward(self, input: torch.Tensor):
        """(decode(encode(x)), result_dict), as the reference's forward (conv_vqgan.py:114-127, taming_vqgan.py:66-69)."""
        zq, result = self.encode(input)
        codes = result["min_encoding_indices"].reshape(zq.shape[0], -1)
        return self._decode_codes(codes.contiguous()), result
