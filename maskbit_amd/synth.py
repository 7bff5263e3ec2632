"""Seeded synthetic checkpoints with the reference's key names and shapes.

No checkpoint or dataset can be downloaded here, so benchmarks, tests and the golden fixtures all run on random-init
weights of the real architectures.  This module is the single source of those weights (pure PyTorch CPU, deterministic
from a seed): ``bench.py`` times them, ``tests/`` and ``oracle/`` load the same tensors into the HIP engine, the CPU
oracle and -- in the build container -- the real reference (``oracle/make_golden.py``), and the fixtures under
``tests/golden/`` guard them with sha256 sentinels.  It contains no part of the algorithm.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

Tensor = torch.Tensor
StateDict = Dict[str, Tensor]


# --------------------------------------------------------------------------- configs
@dataclass(frozen=True)
class GenCfg:
    """Generator hyper-parameters (bert.py:345-358 constructor arguments)."""
    bits: int = 12            # K = log2(codebook_size)
    splits: int = 2           # m
    hidden: int = 1024        # d
    depth: int = 24           # L
    heads: int = 16           # H
    mlp: int = 4096           # f
    seq: int = 256            # (img_size // input_stride) ** 2
    nclass: int = 1000
    prenorm: bool = False     # use_prenorm (bert.py:49-59,106-123,326-327,498-499)
    kind: str = "lfq"         # "lfq": LFQBert (bit-vector input projection); "bert": Bert (embedding tables, tied output head)

    @property
    def group_bits(self) -> int:
        return self.bits // self.splits

    @property
    def group_codes(self) -> int:          # C, also the mask token id
        return 1 << self.group_bits


@dataclass(frozen=True)
class TokCfg:
    """Tokenizer hyper-parameters (configs/tokenizer/*.yaml, model.vq_model)."""
    token_size: int = 12
    hidden_channels: int = 128
    channel_mult: Tuple[int, ...] = (1, 1, 2, 2, 4)
    num_resolutions: int = 5
    num_res_blocks: int = 2
    num_channels: int = 3
    sample_with_conv: bool = True


def _index_to_bits(idx: Tensor, nbits: int) -> Tensor:
    """LSB-first {-1,+1} expansion of integer codes (the lookup-free codebook buffer, lookup_free.py:96-111)."""
    weights = (1 << torch.arange(nbits, dtype=torch.int64))
    return ((idx.long().unsqueeze(-1) & weights) != 0).to(torch.float32) * 2.0 - 1.0


# --------------------------------------------------------------------------- seeded synthetic weights
def make_generator_weights(cfg: GenCfg, seed: int = 0, head_gain: float = 1.0, style: str = "gaussian") -> StateDict:
    """Build-own seeded weights with the reference checkpoint's key names and shapes
    (SURVEY.md 8b).  randn*0.02 for Linear / Embedding / pos_emb, LN gamma=1 beta=0;
    ``head_gain`` scales prediction_layer.weight so the softmax is peaky enough to
    make logit errors visible in the sampled tokens.  ``style`` "outlier": see _trained_like."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.02
    d, f = cfg.hidden, cfg.mlp
    if cfg.kind == "bert":            # Bert (bert.py:222-262): embedding tables instead of the bit projection, tied head + per-position bias
        sd: StateDict = {"pos_emb": rn(1, cfg.seq + 1, d), "class_emb.weight": rn(cfg.nclass + 1, d)}
        for q in range(cfg.splits):
            sd[f"tok_emb_list.{q}.weight"] = rn(cfg.group_codes + 1, d) * (head_gain if head_gain != 1.0 else 1.0)
        sd["first_layer.0.weight"] = torch.ones(d) + rn(d); sd["first_layer.0.bias"] = rn(d)
    else:
        sd = {
            "pos_emb": rn(1, cfg.seq + 1, d),
            "bits_to_indices": (1 << torch.arange(cfg.group_bits)).to(torch.int32),
            "class_emb.weight": rn(cfg.nclass + 1, d),
            "input_proj.weight": rn(d, cfg.bits), "input_proj.bias": rn(d),
            "first_layer.0.weight": torch.ones(d) + rn(d), "first_layer.0.bias": rn(d),
        }
    for l in range(cfg.depth):
        a, ff = f"transformer.layers.{l}.0", f"transformer.layers.{l}.1"
        sd[a + ".mha.in_proj_weight"] = rn(3 * d, d); sd[a + ".mha.in_proj_bias"] = rn(3 * d)
        sd[a + ".mha.out_proj.weight"] = rn(d, d); sd[a + ".mha.out_proj.bias"] = rn(d)
        sd[a + ".norm.weight"] = torch.ones(d) + rn(d); sd[a + ".norm.bias"] = rn(d)
        sd[ff + ".net.0.weight"] = rn(f, d); sd[ff + ".net.0.bias"] = rn(f)
        sd[ff + ".net.2.weight"] = rn(d, f); sd[ff + ".net.2.bias"] = rn(d)
        sd[ff + ".norm.weight"] = torch.ones(d) + rn(d); sd[ff + ".norm.bias"] = rn(d)
    sd["last_layer.0.weight"] = rn(d, d); sd["last_layer.0.bias"] = rn(d)
    sd["last_layer.2.weight"] = torch.ones(d) + rn(d); sd["last_layer.2.bias"] = rn(d)
    if cfg.kind == "bert":
        for q in range(cfg.splits):
            sd[f"bias.{q}"] = rn(cfg.seq, cfg.group_codes)
    else:
        sd["prediction_layer.weight"] = rn(cfg.splits * cfg.group_codes, d) * head_gain
        sd["prediction_layer.bias"] = rn(cfg.splits * cfg.group_codes)
    if cfg.prenorm:                   # drawn last: the streams of the post-norm configurations are unchanged
        sd["norm_after_transformer.weight"] = torch.ones(d) + rn(d); sd["norm_after_transformer.bias"] = rn(d)
    if style != "gaussian":
        _trained_like(sd, cfg, seed, style)
    return sd


OUTLIER_CHANNELS = 6       # "trained-like" style: hidden channels that carry massive, nearly input-independent LayerNorm outputs
OUTLIER_BETA = 12.0        # ... of this magnitude (LayerNorm beta = +-OUTLIER_BETA, gamma x OUTLIER_GAMMA there): ~16x the rms of a normal channel
OUTLIER_GAMMA = 0.1
OUTLIER_CONSUMER = 0.0625  # the consumers' columns of those channels (an outlier channel then contributes about a normal channel's share of an output)


# 48 x 0.75, 12 x 1.5, 3 x 2.5, 1 x 4 of 64, normalised to unit second moment: kurtosis 10.9 (a Gaussian's: 3; Student-t_6: 6)
_HEAVY_TAIL_SCALES = torch.tensor([0.75] * 48 + [1.5] * 12 + [2.5] * 3 + [4.0]) / math.sqrt((48 * 0.75 ** 2 + 12 * 1.5 ** 2 + 3 * 2.5 ** 2 + 16.0) / 64)
# style "outlier2" (round 6: the held-out trained-like family): HEAVIER tails -- 48 x 0.7, 12 x 1.5, 3 x 3.0, 1 x 5.0 of 64: kurtosis 17.2, one weight in 64 is 7.1x
# the typical one -- and ten massive-activation channels instead of six
_HEAVIER_TAIL_SCALES = torch.tensor([0.7] * 48 + [1.5] * 12 + [3.0] * 3 + [5.0]) / math.sqrt((48 * 0.7 ** 2 + 12 * 1.5 ** 2 + 3 * 3.0 ** 2 + 25.0) / 64)
_STYLES = {"outlier": (_HEAVY_TAIL_SCALES, OUTLIER_CHANNELS), "outlier2": (_HEAVIER_TAIL_SCALES, 10)}


def _trained_like(sd: StateDict, cfg: GenCfg, seed: int, style: str) -> None:
    """Post-transform of the Gaussian draw towards the statistics trained transformers show and Gaussian weights do not (what per-row / per-block
    MX-fp4 scales and fp16 activations are sensitive to):  style "outlier" = (1) heavy-tailed Linear weights -- every 2-D trunk / head weight is
    multiplied elementwise by a random scale from _HEAVY_TAIL_SCALES (a scale mixture of normals with the Gaussian draw's standard deviation and
    kurtosis 10.9: one weight in 64 is 4.7x its draw, three are 2.9x);
    (2) OUTLIER_CHANNELS hidden channels carry massive LayerNorm outputs, the same channels in every layer ("massive activations"): beta =
    +-OUTLIER_BETA and gamma x OUTLIER_GAMMA in first_layer.0 and both norms of every layer -- in a post-norm trunk the residual stream then holds
    +-12 in those channels next to ~0.75 rms in the others, a stable fixed point at which the logits still depend on tokens and class as much as
    the Gaussian draw's do (a large gamma instead runs away -- the next LayerNorm divides everything else by the outliers' magnitude -- and from
    +-15 on the random trunk stops passing information) -- and the matching in_proj / net.0 / last_layer.0 columns x OUTLIER_CONSUMER.  Deterministic
    from the seed (a generator of its own, so the Gaussian draw and every existing fixture stay what they were)."""
    if style not in _STYLES:
        raise ValueError(f"unknown weight style '{style}'")
    tail_scales, n_outlier = _STYLES[style]
    g = torch.Generator().manual_seed(1_000_003 * (seed + 1))
    d = cfg.hidden
    for k in sorted(sd):
        v = sd[k]
        if v.dim() == 2 and (k.startswith("transformer.layers.") or k.startswith("last_layer.0") or k.startswith("prediction_layer")):
            # a scale mixture of normals from an integer draw and a table of exact constants: one multiply per weight, bit-reproducible on any host
            # (torch's CPU exponential_ and even sqrt are not: both differ between this build container and the GPU boxes' hosts)
            sd[k] = v * tail_scales[torch.randint(0, 64, v.shape, generator=g)]
    ch = torch.randperm(d, generator=g)[:n_outlier]
    sign = torch.where(torch.rand(n_outlier, generator=g) < 0.5, -1.0, 1.0)
    norms = ["first_layer.0"] + [f"transformer.layers.{l}.{s}.norm" for l in range(cfg.depth) for s in (0, 1)]
    for n in norms:
        sd[n + ".weight"][ch] *= OUTLIER_GAMMA
        sd[n + ".bias"][ch] = OUTLIER_BETA * sign
    for l in range(cfg.depth):
        sd[f"transformer.layers.{l}.0.mha.in_proj_weight"][:, ch] *= OUTLIER_CONSUMER
        sd[f"transformer.layers.{l}.1.net.0.weight"][:, ch] *= OUTLIER_CONSUMER
    sd["last_layer.0.weight"][:, ch] *= OUTLIER_CONSUMER       # the last layer's second norm feeds the head


def decoder_plan(cfg: TokCfg) -> List[Tuple[str, int, int, bool]]:
    """(stage prefix, Cin, Cout, has_upsample) for decoder.up.* following autoencoder.py:370-392."""
    mult = tuple(cfg.channel_mult) + (cfg.channel_mult[-1],)
    out = []
    for s, lvl in enumerate(reversed(range(cfg.num_resolutions))):
        out.append((f"decoder.up.{s}", cfg.hidden_channels * mult[lvl + 1], cfg.hidden_channels * mult[lvl], lvl > 0))
    return out


TOK_OFFSET_GROUPS = 3      # tokenizer style "trained": GroupNorm groups of every residual block's output that carry a large constant offset ...
TOK_OFFSET_DC = 12.0       # ... of this size per block (|mean| / std of those groups ~ 8 .. 36 at the next GroupNorm)
TOK_OFFSET_BETA = 6.0      # the norm2 beta of the channel that feeds it (SiLU(6) = 5.985, gamma x 0.1 there: nearly input-independent)
TOK_STREAM_GAIN = 1.2      # conv2 of every residual block: the residual stream grows along the stages


def _trained_like_tokenizer(sd: StateDict, seed: int) -> None:
    """Post-transform of the Gaussian tokenizer draw towards what trained VQGAN decoders show and the Gaussian draw does not (what the fp32
    E[x^2] - mean^2 GroupNorm statistics and the fp16 activations are sensitive to): (1) heavy-tailed conv weights (_HEAVY_TAIL_SCALES, as _trained_like);
    (2) in every residual block one norm2 channel with beta = TOK_OFFSET_BETA feeds, through the centre tap of conv2 alone (so the offset is the same at the
    borders), TOK_OFFSET_GROUPS whole GroupNorm groups of the block's output with a constant +-TOK_OFFSET_DC: the next GroupNorm sees groups whose
    |mean| is 8 .. 36 x their std (less where an up- / downsampling conv has mixed the channels in between); (3) conv2 x TOK_STREAM_GAIN: a residual stream that grows from block to block.  Deterministic from the seed (a
    generator of its own: the Gaussian draw and every existing fixture stay what they were)."""
    g = torch.Generator().manual_seed(1_000_003 * (seed + 1) + 17)
    for k in sorted(sd):
        if sd[k].dim() == 4:
            sd[k] = sd[k] * _HEAVY_TAIL_SCALES[torch.randint(0, 64, sd[k].shape, generator=g)]
    for k in sorted(sd):
        if not k.endswith(".norm2.weight"):
            continue
        p = k[: -len(".norm2.weight")]
        w = sd[p + ".conv2.weight"] * TOK_STREAM_GAIN
        co = w.shape[0]
        cpg = co // 32
        src = int(torch.randint(0, co, (1,), generator=g))
        groups = torch.randperm(32, generator=g)[:TOK_OFFSET_GROUPS]
        sign = torch.where(torch.rand(TOK_OFFSET_GROUPS, generator=g) < 0.5, -1.0, 1.0)
        sd[p + ".norm2.weight"][src] *= 0.1
        sd[p + ".norm2.bias"][src] = TOK_OFFSET_BETA
        for gi, sg in zip(groups.tolist(), sign.tolist()):
            w[gi * cpg:(gi + 1) * cpg, src] = 0.0
            w[gi * cpg:(gi + 1) * cpg, src, 1, 1] = sg * TOK_OFFSET_DC / 5.985
            if p + ".nin_shortcut.weight" in sd:           # out = h + W h: the shortcut does not smear the offset over the other groups
                sd[p + ".nin_shortcut.weight"][:, gi * cpg:(gi + 1) * cpg] = 0.0
        sd[p + ".conv2.weight"] = w


def make_tokenizer_weights(cfg: TokCfg, seed: int = 0, with_encoder: bool = False, lfq_buffers: bool = True, style: str = "gaussian") -> StateDict:
    """Seeded conv weights randn/sqrt(fan_in), GN gamma ~ 1, with the reference's key names.  ``lfq_buffers=False``: without the LFQ
    quantizer's derived buffers (a lookup tokenizer's codebook comes from make_vq_codebook instead).  ``style`` "trained": see
    _trained_like_tokenizer."""
    if style not in ("gaussian", "trained"):
        raise ValueError(f"unknown tokenizer weight style '{style}'")
    g = torch.Generator().manual_seed(seed)

    def conv(co, ci, k):
        return torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k)

    def vec(c, base=0.0, s=0.05):
        return base + torch.randn(c, generator=g) * s

    sd: StateDict = {}

    def res_block(p, ci, co):
        sd[p + ".norm1.weight"] = vec(ci, 1.0); sd[p + ".norm1.bias"] = vec(ci)
        sd[p + ".conv1.weight"] = conv(co, ci, 3)
        sd[p + ".norm2.weight"] = vec(co, 1.0); sd[p + ".norm2.bias"] = vec(co)
        sd[p + ".conv2.weight"] = conv(co, co, 3)
        if ci != co:
            sd[p + ".nin_shortcut.weight"] = conv(co, co, 1)

    top = cfg.hidden_channels * cfg.channel_mult[cfg.num_resolutions - 1]
    sd["decoder.conv_in.weight"] = conv(top, cfg.token_size, 3); sd["decoder.conv_in.bias"] = vec(top)
    for r in range(cfg.num_res_blocks):
        res_block(f"decoder.mid.res_blocks.{r}", top, top)
    last = top
    for p, ci, co, up in decoder_plan(cfg):
        c = ci
        for r in range(cfg.num_res_blocks):
            res_block(f"{p}.res_blocks.{r}", c, co)
            c = co
        if up:
            sd[p + ".upsample_conv.weight"] = conv(co, co, 3); sd[p + ".upsample_conv.bias"] = vec(co)
        last = co
    sd["decoder.norm_out.weight"] = vec(last, 1.0); sd["decoder.norm_out.bias"] = vec(last)
    sd["decoder.conv_out.weight"] = conv(cfg.num_channels, last, 3); sd["decoder.conv_out.bias"] = vec(cfg.num_channels, 0.5, 0.1)
    if with_encoder:
        emult = (1,) + tuple(cfg.channel_mult)
        sd["encoder.conv_in.weight"] = conv(cfg.hidden_channels, cfg.num_channels, 3)
        c = cfg.hidden_channels
        for s in range(cfg.num_resolutions):
            ci, co = cfg.hidden_channels * emult[s], cfg.hidden_channels * emult[s + 1]
            c = ci
            for r in range(cfg.num_res_blocks):
                res_block(f"encoder.down.{s}.res_blocks.{r}", c, co)
                c = co
            if s < cfg.num_resolutions - 1 and cfg.sample_with_conv:
                sd[f"encoder.down.{s}.down_conv.weight"] = conv(co, co, 3); sd[f"encoder.down.{s}.down_conv.bias"] = vec(co)
        for r in range(cfg.num_res_blocks):
            res_block(f"encoder.mid.res_blocks.{r}", c, c)
        sd["encoder.norm_out.weight"] = vec(c, 1.0); sd["encoder.norm_out.bias"] = vec(c)
        sd["encoder.conv_out.weight"] = conv(cfg.token_size, c, 1); sd["encoder.conv_out.bias"] = vec(cfg.token_size)
        if lfq_buffers:
            sd["quantize.bits_to_indices"] = (1 << torch.arange(cfg.token_size)).to(torch.int32)
            sd["quantize.codebook"] = _index_to_bits(torch.arange(1 << cfg.token_size), cfg.token_size)
    if style == "trained":
        _trained_like_tokenizer(sd, seed)
    return sd


def make_taming_weights(seed: int = 0, qk_gain: float = 1.0) -> StateDict:
    """Seeded weights of the Taming VQGAN tokenizer (``OriginalVQModel``) with the reference's 343 key names and shapes, in the state dict's own
    order: conv weights randn / sqrt(fan_in), conv biases ~ 0.05, GroupNorm gamma ~ 1 -- O(1) activations through the depth, as
    make_tokenizer_weights.  ``qk_gain`` multiplies the q and k weights and biases of the seven AttnBlocks: with the plain draw the scores have
    unit variance and the softmax over 256 keys is nearly uniform, which would leave the attention untested end to end; the scores' spread grows
    with the square of the gain.  ``quantize.embedding.weight`` is a placeholder of zeros: the codebook comes from make_vq_codebook on the
    latent statistics, as for the other lookup tokenizers."""
    from .taming_vqgan import CODEBOOK_SIZE, TOKEN_SIZE, taming_specs, _conv
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}
    specs = taming_specs() + [("quantize.embedding.weight", (CODEBOOK_SIZE, TOKEN_SIZE), "codebook")] + \
        _conv("quant_conv", TOKEN_SIZE, TOKEN_SIZE, 1) + _conv("post_quant_conv", TOKEN_SIZE, TOKEN_SIZE, 1)
    for key, shape, kind in specs:
        if kind == "codebook":
            sd[key] = torch.zeros(shape)
        elif len(shape) == 4:
            sd[key] = torch.randn(*shape, generator=g) / math.sqrt(shape[1] * shape[2] * shape[3])
        elif kind == "ones":
            sd[key] = 1.0 + torch.randn(*shape, generator=g) * 0.05
        else:
            sd[key] = torch.randn(*shape, generator=g) * 0.05
        if key.rsplit(".", 2)[-2] in ("q", "k"):
            sd[key] = sd[key] * qk_gain
    return sd


def make_vq_codebook(codebook_size: int, token_size: int, seed: int, mean, std) -> Tensor:
    """Seeded lookup-quantizer codebook [C, K] = randn * std + mean (per channel): entries at the scale of the encoder's latents, so that the
    nearest-entry search is not trivial (the reference's uniform(+-1/C) init puts every entry next to the origin)."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(1, -1)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(1, -1)
    return torch.randn(codebook_size, token_size, generator=g) * std + mean


EVAL_FAMILIES = ("noise", "sin", "flat", "bright")


def make_eval_images(family: str, err_sigma: float, B: int, H: int, W: int, seed: int, C: int = 3) -> Tuple[Tensor, Tensor]:
    """Seeded (real, fake) fp32 [B, C, H, W] image pairs for the evaluator's fixtures, fake = real + err_sigma * randn (not clamped).
    Families: ``noise`` uniform [0, 1); ``sin`` smooth sinusoids around 0.5; ``flat`` a 0.8 field with 0.002 noise; ``bright`` uniform
    [0.9, 1.0) -- the last two are where E[x^2] - E[x]^2 cancels and the fp32 rounding of the SSIM filter shows."""
    g = torch.Generator().manual_seed(seed)
    if family == "noise":
        real = torch.rand(B, C, H, W, generator=g)
    elif family == "sin":
        f = torch.rand(B, C, 2, generator=g) * 6.0 + 0.5
        ph = torch.rand(B, C, generator=g) * (2.0 * math.pi)
        yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / H
        xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / W
        f, ph = f.double(), ph.double()
        arg = 2.0 * math.pi * (f[..., 0].view(B, C, 1, 1) * yy + f[..., 1].view(B, C, 1, 1) * xx) + ph.view(B, C, 1, 1)
        real = (0.5 + 0.4 * torch.sin(arg)).float()            # evaluated in fp64: the fp32 rounding hides the last-bit spread of libm's sin
    elif family == "flat":
        real = 0.8 + 0.002 * torch.randn(B, C, H, W, generator=g)
    elif family == "bright":
        real = 0.9 + 0.1 * torch.rand(B, C, H, W, generator=g)
    else:
        raise ValueError(f"unknown image family {family!r}")
    fake = real + err_sigma * torch.randn(B, C, H, W, generator=g)
    return real.contiguous(), fake.contiguous()


def make_eval_indices(kind: str, K: int, shape, seed: int) -> Tensor:
    """Seeded int64 codebook indices in [0, K): ``uniform`` over all entries, or ``skew`` (a cubed uniform draw over the first third of the
    codebook: repeated entries, most of the codebook unused)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.randint(0, K, tuple(shape), generator=g)
    if kind == "skew":
        return (torch.rand(tuple(shape), generator=g).pow(3) * (K // 3)).long()
    raise ValueError(f"unknown index kind {kind!r}")


EVAL_FEATURE_KINDS = ("real", "fake")


def make_eval_features(D: int, C: int, N: int, seed: int, kind: str = "fake") -> Tuple[Tensor, Tensor]:
    """Seeded float64 inputs of the FID / Inception-score fixtures: features [N, D], non-negative and correlated like pooled ReLU activations
    (a per-sample common factor and a neighbour term under the ReLU), and logits [N, C] = 3 * randn with one boosted class per sample, so that
    the score is neither 1 nor C.  ``kind``: ``real`` or ``fake`` -- the fake features are shifted and widened, for a Frechet distance well
    above its rounding.  Element-wise operations only: the same bits on every machine."""
    if kind not in EVAL_FEATURE_KINDS:
        raise ValueError(f"unknown feature kind {kind!r}")
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, D, generator=g, dtype=torch.float64)
    common = torch.randn(N, 1, generator=g, dtype=torch.float64)
    bias = torch.rand(1, D, generator=g, dtype=torch.float64)
    gain, shift = (1.0, 0.0) if kind == "real" else (1.15, 0.1)
    feats = torch.relu(gain * (z + 0.7 * torch.roll(z, 1, dims=1) + 0.5 * common) + 0.4 * bias + shift)
    logits = 3.0 * torch.randn(N, C, generator=g, dtype=torch.float64)
    hot = torch.randint(0, C, (N, 1), generator=g)
    logits.scatter_add_(1, hot, torch.full((N, 1), 4.0, dtype=torch.float64))
    return feats.contiguous(), logits.contiguous()


def make_eval_statistics(D: int, N: int, seed: int) -> Tuple[Tensor, Tensor]:
    """Seeded "real" statistics for the FID fixtures, in the format of the reference's ImageNet statistics file: ``mu`` [D] and the sample
    covariance ``sigma`` [D, D] (float64) of N ``real`` features (N > D: full rank)."""
    x, _ = make_eval_features(D, 1, N, seed, "real")
    mu = x.mean(0)
    xc = x - mu
    return mu, (xc.T @ xc) / (N - 1)


def make_mlm_case(b: int, n: int, m: int, C: int, seed: int) -> Tuple[Tensor, Tensor]:
    """Seeded inputs of the masked-token validation fixtures: logits fp32 [b, n, m, C] = 4 * randn, and targets int64 [b, n, m] = the row's
    argmax on a seeded half of the rows, a uniform draw elsewhere -- accuracies near 0.5, so that ``accuracy ** m`` is not degenerate."""
    g = torch.Generator().manual_seed(seed)
    logits = 4.0 * torch.randn(b, n, m, C, generator=g)
    easy = torch.rand(b, n, m, generator=g) < 0.5
    other = torch.randint(0, C, (b, n, m), generator=g)
    return logits.contiguous(), torch.where(easy, logits.argmax(-1), other)


def make_mlm_tokens(b: int, n: int, m: int, C: int, seed: int) -> Tensor:
    """Seeded int64 tokens [b, n, m] in [0, C) for the masking fixtures."""
    return torch.randint(0, C, (b, n, m), generator=torch.Generator().manual_seed(seed))


VGG16_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
               (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))   # (features index, Cin, Cout)
VGG16_GROWN_GAIN = 1.45


def make_vgg16_weights(seed: int, style: str = "he") -> StateDict:
    """Seeded weights of torchvision's VGG16-D ``features`` stack (thirteen 3x3 convolutions with bias) under bare ``N.weight`` / ``N.bias`` keys,
    as ``nn.Sequential.load_state_dict`` and ``LPIPS.load_vgg16`` take them.  ImageNet VGG16 is not available here; these stand in for it.

    ``"he"``: He-normal weights (std = sqrt(2 / fan_in)), bias N(0, 0.05): activations stay O(1) through the stack.  On
    ``make_eval_images("noise", ...)`` inputs of 256 x 256 the five taps (relu1_2 .. relu5_3) have rms 1.4 / 2.4 / 3.2 / 3.1 / 3.0 and maxima
    10 / 13 / 18 / 18 / 14 (seed 4100; on the ``"bright"`` family 1.7 / 1.8 / 1.8 / 1.3 / 0.7).
    (The ``"kaiming"`` uniform init of the model classes would shrink activations about 0.4 x per layer into fp16 subnormals.)

    ``"grown"``: the same draws with every layer's weights times 1.45 and its bias times the accumulated gain, so the activations grow as those
    of ImageNet VGG16 do (unnormalised, large at the deep taps): tap rms 2.9 / 11 / 43 / 128 / 371, maxima 20 / 66 / 236 / 781 / 1 860 on the
    same inputs -- what the fp16 range and the saturation counter have to see."""
    if style not in ("he", "grown"):
        raise ValueError(f"unknown VGG16 weight style {style!r}")
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}
    gain = 1.0
    for idx, cin, cout in VGG16_CONVS:
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
        b = torch.randn(cout, generator=g) * 0.05
        if style == "grown":
            gain *= VGG16_GROWN_GAIN
            w, b = w * VGG16_GROWN_GAIN, b * gain
        sd[f"{idx}.weight"], sd[f"{idx}.bias"] = w.contiguous(), b.contiguous()
    return sd


InceptionConv = Tuple[str, int, int, Tuple[int, int], int, Tuple[int, int]]     # (name, Cin, Cout, (kh, kw), stride, (ph, pw))
INCEPTION_CONCAT = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
                    "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
INCEPTION_FC = (1008, 2048)


def inception_convs() -> List[InceptionConv]:
    """The 94 ``BasicConv2d`` layers of the FID Inception-v3 (pytorch-fid's ``pt_inception-2015-12-05``) in forward order: the table of shapes
    behind the state dict.  (The wiring -- which layer reads what -- is DESIGN.md "Inception-v3"; it is not here.)"""
    L: List[InceptionConv] = []

    def add(name, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
        L.append((name, cin, cout, k, stride, pad))

    add("Conv2d_1a_3x3", 3, 32, (3, 3), 2)
    add("Conv2d_2a_3x3", 32, 32, (3, 3))
    add("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1))
    add("Conv2d_3b_1x1", 64, 80)
    add("Conv2d_4a_3x3", 80, 192, (3, 3))
    for n, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(n + ".branch1x1", cin, 64)
        add(n + ".branch5x5_1", cin, 48)
        add(n + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2))
        add(n + ".branch3x3dbl_1", cin, 64)
        add(n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
        add(n + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1))
        add(n + ".branch_pool", cin, pf)
    add("Mixed_6a.branch3x3", 288, 384, (3, 3), 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1))
    add("Mixed_6a.branch3x3dbl_3", 96, 96, (3, 3), 2)
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(n + ".branch1x1", 768, 192)
        add(n + ".branch7x7_1", 768, c7)
        add(n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(n + ".branch7x7dbl_1", 768, c7)
        add(n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(n + ".branch_pool", 768, 192)
    add("Mixed_7a.branch3x3_1", 768, 192)
    add("Mixed_7a.branch3x3_2", 192, 320, (3, 3), 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, (3, 3), 2)
    for n, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(n + ".branch1x1", cin, 320)
        add(n + ".branch3x3_1", cin, 384)
        add(n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(n + ".branch3x3dbl_1", cin, 448)
        add(n + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1))
        add(n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(n + ".branch_pool", cin, 192)
    return L


def make_inception_weights(seed: int, style: str = "he") -> StateDict:
    """Seeded weights of the FID Inception-v3 under the keys of pytorch-fid's ``pt_inception-2015-12-05-6726825d.pth``: per ``BasicConv2d``
    ``<name>.conv.weight`` (OIHW, no bias) and ``<name>.bn.{weight,bias,running_mean,running_var}``, then ``fc.weight`` [1008, 2048] and
    ``fc.bias`` [1008]: 94 x 5 + 2 = 472 entries.  The real checkpoint is not available here; these stand in for it.

    ``"he"``: He-normal convolutions (std = sqrt(2 / fan_in)); BatchNorm gamma in [0.8, 1.2), beta N(0, 0.1), running mean N(0, 0.1) and
    running variance in [0.8, 1.25): the epilogue scale is near 1 and every layer hands on what a He-initialised ReLU layer does.

    ``"tf"``: gamma exactly 1, as the TF checkpoint has it, and running variances 10^U(-3, 1) per channel -- four decades.  The convolution
    weights of a channel are the He draw times sqrt(var + 1e-3) and its running mean N(0, 0.1) times the same factor, so that the epilogue
    scale 1 / sqrt(var + 1e-3) in [0.3, 31] brings every channel back to O(1): an engine that folded the scale into fp16 weights, or dropped
    it, is far off on these.

    Measured on the real half of ``make_eval_images("noise", 0.05, 2, 64, 64, 5)`` as uint8 (seed 4400; rms / maximum / share of exact zeros of
    the ReLU outputs behind the taps -- the two pooled taps '64' and '192' read Conv2d_2b and Conv2d_4a through a 3 x 3 maximum, which has next to
    no zeros itself):
      he: Conv2d_2b 0.30 / 2.9 / 0.53, Conv2d_4a 0.42 / 3.8 / 0.54, Mixed_5d 0.52 / 3.5 / 0.47, Mixed_6e 0.50 / 3.3 / 0.49, Mixed_7c 0.58 / 3.5 / 0.50
      tf: Conv2d_2b 0.36 / 3.3 / 0.44, Conv2d_4a 0.52 / 4.1 / 0.59, Mixed_5d 0.61 / 4.1 / 0.51, Mixed_6e 0.72 / 4.4 / 0.48, Mixed_7c 0.83 / 4.6 / 0.48
    The fp32 taps '64' / '192' / '768' / '2048' have rms 0.45 / 0.60 / 0.46 / 0.53 (he) and 0.53 / 0.69 / 0.66 / 0.77 (tf).
    No tap is dead or saturated and the zeros stay between 20 % and 80 % (tests/test_inception_cpu.py holds both styles to that).
    ``fc``: N(0, 1 / sqrt(2048)) weights and N(0, 0.1) bias: logits of order 1."""
    if style not in ("he", "tf"):
        raise ValueError(f"unknown Inception weight style {style!r}")
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}
    for name, cin, cout, (kh, kw), _stride, _pad in inception_convs():
        w = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cin * kh * kw))
        beta = torch.randn(cout, generator=g) * 0.1
        mean = torch.randn(cout, generator=g) * 0.1
        u = torch.rand(cout, generator=g)
        if style == "he":
            gamma = 0.8 + 0.4 * torch.rand(cout, generator=g)
            var = 0.8 + 0.45 * u
        else:
            gamma = torch.ones(cout)
            var = torch.pow(10.0, 4.0 * u - 3.0)
            s = torch.sqrt(var + 1e-3)
            w, mean = w * s.view(-1, 1, 1, 1), mean * s
        sd[name + ".conv.weight"] = w.contiguous()
        sd[name + ".bn.weight"], sd[name + ".bn.bias"] = gamma, beta
        sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = mean, var
    n, d = INCEPTION_FC
    sd["fc.weight"] = torch.randn(n, d, generator=g) / math.sqrt(d)
    sd["fc.bias"] = torch.randn(n, generator=g) * 0.1
    return sd


# torchvision's resnet50 (v1.5; DESIGN.md "ResNet-50"): (convolution key, BatchNorm key, Cin, Cout, kernel, stride), in state-dict order
ResNetConv = Tuple[str, str, int, int, int, int]
RESNET50_BLOCKS = (3, 4, 6, 3)
RESNET50_FC = (1000, 2048)
RESNET50_RESIDUAL_GAIN = 0.3


def resnet50_convs() -> List[ResNetConv]:
    convs: List[ResNetConv] = [("conv1", "bn1", 3, 64, 7, 2)]
    cin = 64
    for layer, blocks in enumerate(RESNET50_BLOCKS):
        width = 64 << layer
        for b in range(blocks):
            p = f"layer{layer + 1}.{b}"
            stride = 2 if (b == 0 and layer > 0) else 1
            convs += [(p + ".conv1", p + ".bn1", cin, width, 1, 1), (p + ".conv2", p + ".bn2", width, width, 3, stride),
                      (p + ".conv3", p + ".bn3", width, 4 * width, 1, 1)]
            if b == 0:
                convs.append((p + ".downsample.0", p + ".downsample.1", cin, 4 * width, 1, stride))
            cin = 4 * width
    return convs


def make_resnet50_weights(seed: int) -> StateDict:
    """Seeded weights of torchvision's resnet50 under its own keys (``conv1.weight``, ``bn1.*``, ``layerL.B.*``, ``fc.*``; the
    ``num_batches_tracked`` counters included, as 0): 53 convolutions x 6 + 2 = 320 entries, 25 557 032 parameters.  The ImageNet checkpoint is not
    available here; these stand in for it.

    He-normal convolutions (std = sqrt(2 / fan_in)); BatchNorm gamma in [0.8, 1.2), beta N(0, 0.1), running mean N(0, 0.1), running variance in
    [0.8, 1.25) -- except the last BatchNorm of every bottleneck (``bn3``), whose gamma is times RESNET50_RESIDUAL_GAIN: sixteen residual adds of
    unit-variance branches would otherwise grow the stream fourfold, which trained networks do not do.  ``fc``: N(0, 1 / sqrt(2048)) weights and
    N(0, 0.1) bias: logits of order 1."""
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}
    for conv, bn, cin, cout, k, _stride in resnet50_convs():
        sd[conv + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        gamma = 0.8 + 0.4 * torch.rand(cout, generator=g)
        if bn.endswith(".bn3"):
            gamma = gamma * RESNET50_RESIDUAL_GAIN
        sd[bn + ".weight"], sd[bn + ".bias"] = gamma, torch.randn(cout, generator=g) * 0.1
        sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.randn(cout, generator=g) * 0.1, 0.8 + 0.45 * torch.rand(cout, generator=g)
        sd[bn + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    n, d = RESNET50_FC
    sd["fc.weight"] = torch.randn(n, d, generator=g) / math.sqrt(d)
    sd["fc.bias"] = torch.randn(n, generator=g) * 0.1
    return sd


DISC_LOGIT_GAIN = 1.5


def make_discriminator_weights(seed: int, hidden_channels: int = 128, num_stages: int = 3, blur_kernel_size: int = 4) -> StateDict:
    """Seeded weights of the reference's ``NLayerDiscriminatorv2`` under its own keys (``blur_kernel_size`` 3, 4, 5: with the
    ``blocks.{i}.1.kernel`` buffers of ``blur_resample=True``; 0: the average-pool variant, without).  No trained discriminator is available
    here; these stand in for one.

    He-normal convolutions (std = sqrt(2 / fan_in)) with N(0, 0.1) biases; GroupNorm gamma in [0.6, 1.4), beta N(0, 0.2) -- neither the unit
    nor the zero of a fresh module; ``to_logits.2``: N(0, DISC_LOGIT_GAIN / sqrt(fan_in)) weights and a bias of 0.1, which spreads the logits of
    uniform-noise images over roughly +-2: a hinge sum has terms on both sides of its kink, and nothing comes near the fp16 range."""
    g = torch.Generator().manual_seed(seed)
    sd: StateDict = {}

    def conv(key: str, cout: int, cin: int, k: int, gain: float = math.sqrt(2.0)) -> None:
        sd[key + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (gain / math.sqrt(cin * k * k))
        sd[key + ".bias"] = torch.randn(cout, generator=g) * 0.1

    conv("block_in.0", hidden_channels, 3, 5)
    cin = hidden_channels
    for i in range(num_stages):
        cout = hidden_channels << i
        conv(f"blocks.{i}.0", cout, cin, 3)
        if blur_kernel_size:
            row = torch.tensor({3: (1, 2, 1), 4: (1, 3, 3, 1), 5: (1, 4, 6, 4, 1)}[blur_kernel_size], dtype=torch.float32)
            k2 = row[None, :] * row[:, None]
            sd[f"blocks.{i}.1.kernel"] = (k2 / k2.sum())[None, None]
        sd[f"blocks.{i}.2.weight"] = 0.6 + 0.8 * torch.rand(cout, generator=g)
        sd[f"blocks.{i}.2.bias"] = torch.randn(cout, generator=g) * 0.2
        cin = cout
    conv("to_logits.0", cin, cin, 1)
    conv("to_logits.2", 1, cin, 5, gain=DISC_LOGIT_GAIN)
    sd["to_logits.2.bias"] = torch.full((1,), 0.1)
    return sd
