"""Float64 restatement of the Taming VQGAN tokenizer's forward (the reference's OriginalVQModel) from a state dict, for the tests.

Test infrastructure, written from the behaviour of the reference's modules (paths relative to the reference root): it is pinned to the
fixture the real reference produced (tests/test_taming_cpu.py), and the GPU tests compare the engine against it where the fixture holds no
tensor (512 x 512 images).  Nothing of the product imports it.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

CH_MULT = (1, 1, 2, 2, 4)
ATTN = ("encoder.down.4.attn.0", "encoder.down.4.attn.1", "encoder.mid.attn_1", "decoder.mid.attn_1",
        "decoder.up.4.attn.0", "decoder.up.4.attn.1", "decoder.up.4.attn.2")


def _p(sd, key):
    return sd[key].double()


def conv(sd, p, x, stride=1, padding=0):
    return F.conv2d(x, _p(sd, p + ".weight"), _p(sd, p + ".bias"), stride=stride, padding=padding)


def norm(sd, p, x):
    """Normalize: GroupNorm(32 groups, eps 1e-6, affine) (modeling/taming/taming_autoencoder.py:15-16)."""
    return F.group_norm(x, 32, _p(sd, p + ".weight"), _p(sd, p + ".bias"), eps=1e-6)


def swish(x):
    return x * torch.sigmoid(x)                                   # taming_autoencoder.py:10-12


def res_block(sd, p, x):
    """ResnetBlock.forward without temb and dropout (taming_autoencoder.py:98-118): the 1x1 nin_shortcut is applied to the block INPUT."""
    h = conv(sd, p + ".conv1", swish(norm(sd, p + ".norm1", x)), padding=1)
    h = conv(sd, p + ".conv2", swish(norm(sd, p + ".norm2", h)), padding=1)
    if p + ".nin_shortcut.weight" in sd:
        x = conv(sd, p + ".nin_shortcut", x)
    return x + h


def attention(q, k, v):
    """q, k, v [b, n, c] -> softmax(q k^T c^-0.5) v (taming_autoencoder.py:157-168)."""
    w = torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (q.shape[-1] ** -0.5), dim=2)
    return torch.bmm(w, v)


def attn_block(sd, p, x, taps=None):
    """AttnBlock.forward (taming_autoencoder.py:149-173): GroupNorm without nonlinearity, 1x1 q / k / v, single-head attention over the h w
    pixels, 1x1 proj_out, + x."""
    b, c, h, w = x.shape
    hn = norm(sd, p + ".norm", x)
    q, k, v = (conv(sd, f"{p}.{n}", hn).reshape(b, c, h * w).transpose(1, 2) for n in ("q", "k", "v"))
    o = attention(q, k, v).transpose(1, 2).reshape(b, c, h, w)
    out = x + conv(sd, p + ".proj_out", o)
    if taps is not None:
        taps[p] = out
    return out


def downsample(sd, p, x):
    """Downsample.forward (taming_autoencoder.py:49-53): one zero column on the right and one zero row at the bottom, then 3x3 stride 2, no padding."""
    return conv(sd, p + ".conv", F.pad(x, (0, 1, 0, 1)), stride=2)


def upsample(sd, p, x):
    """Upsample.forward (taming_autoencoder.py:30-34): nearest 2x, then 3x3."""
    return conv(sd, p + ".conv", x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), padding=1)


def encoder(sd, x, taps=None):
    """Encoder.forward (taming_autoencoder.py:240-267) on an image already scaled to [-1, 1]."""
    h = conv(sd, "encoder.conv_in", x, padding=1)
    R = len(CH_MULT)
    for l in range(R):
        for r in range(2):
            h = res_block(sd, f"encoder.down.{l}.block.{r}", h)
            if l == R - 1:
                h = attn_block(sd, f"encoder.down.{l}.attn.{r}", h, taps)
        if l != R - 1:
            h = downsample(sd, f"encoder.down.{l}.downsample", h)
    h = res_block(sd, "encoder.mid.block_1", h)
    h = attn_block(sd, "encoder.mid.attn_1", h, taps)
    h = res_block(sd, "encoder.mid.block_2", h)
    return conv(sd, "encoder.conv_out", swish(norm(sd, "encoder.norm_out", h)), padding=1)


def decoder(sd, z, taps=None):
    """Decoder.forward (taming_autoencoder.py:340-370): up.{i} holds level i (0 the finest), the levels run from 4 down to 0, three blocks each."""
    h = conv(sd, "decoder.conv_in", z, padding=1)
    h = res_block(sd, "decoder.mid.block_1", h)
    h = attn_block(sd, "decoder.mid.attn_1", h, taps)
    h = res_block(sd, "decoder.mid.block_2", h)
    R = len(CH_MULT)
    for l in reversed(range(R)):
        for r in range(3):
            h = res_block(sd, f"decoder.up.{l}.block.{r}", h)
            if l == R - 1:
                h = attn_block(sd, f"decoder.up.{l}.attn.{r}", h, taps)
        if l != 0:
            h = upsample(sd, f"decoder.up.{l}.upsample", h)
    return conv(sd, "decoder.conv_out", swish(norm(sd, "decoder.norm_out", h)), padding=1)


def latent(sd, x, taps=None):
    """The pre-quantisation latent of OriginalVQModel.encode (modeling/taming_vqgan.py:45-48): quant_conv(encoder(x * 2 - 1))."""
    return conv(sd, "quant_conv", encoder(sd, x.double() * 2.0 - 1.0, taps))


def quantize(sd, z, commitment_cost=0.25):
    """SimpleVectorizer.forward in eval mode without normalisation (modeling/quantizer/quantizer.py:45-103): nearest codebook row by squared
    distance -> (zq [b, c, h, w], indices [b, h, w], per-row distances to every entry, losses)."""
    b, c, h, w = z.shape
    zf = z.permute(0, 2, 3, 1).reshape(-1, c)
    e = _p(sd, "quantize.embedding.weight")
    d = zf.pow(2).sum(1, keepdim=True) + e.pow(2).sum(1)[None] - 2.0 * zf @ e.t()
    idx = d.argmin(1)
    zq = e[idx].reshape(b, h, w, c).permute(0, 3, 1, 2)
    codebook_loss = (zq - z).pow(2).mean()
    commitment_loss = commitment_cost * codebook_loss
    return zq, idx.reshape(b, h, w), d, dict(codebook_loss=codebook_loss, commitment_loss=commitment_loss, quantizer_loss=codebook_loss + commitment_loss)


def decode(sd, zq, taps=None):
    """OriginalVQModel.decode (modeling/taming_vqgan.py:52-56): (decoder(post_quant_conv(zq)) + 1) / 2."""
    return (decoder(sd, conv(sd, "post_quant_conv", zq.double()), taps) + 1.0) / 2.0


def decode_tokens(sd, idx, taps=None):
    """OriginalVQModel.decode_tokens (modeling/taming_vqgan.py:58-64): idx [b, h, w] or [b, n] with a square grid."""
    b = idx.shape[0]
    side = int(round(idx[0].numel() ** 0.5))
    zq = _p(sd, "quantize.embedding.weight")[idx.reshape(b, -1)].reshape(b, side, side, -1).permute(0, 3, 1, 2)
    return decode(sd, zq, taps)
