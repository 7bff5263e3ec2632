"""MaskBit generator (LFQBert) backed by the gfx950 engine.

Call surface of the reference's ``modeling.bert.LFQBert`` (bert.py:344-508): same constructor
keywords, same checkpoint keys, ``model(img_tokens, class_labels, drop_label_mask)
-> logits [b, seq, m, C]`` float32.  The forward itself is ``mb_gen_forward`` in
libmaskbit_hip.so: fused bit-token embed + LayerNorm, 24 x (fp16 MFMA QKV GEMM, LDS-resident
attention, out-proj GEMM + residual, LayerNorm, FFN GEMMs with fused erf-GELU / residual), head.
Both the post-norm (every shipped config) and the pre-norm variant run on the engine; ``Bert`` is the
embedding-table sibling of ``LFQBert``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional

import torch

from . import _lib
from .base_model import BaseModel, ParamSpec

# Precision mode of the engine (mb_gen_cfg.precision, include/maskbit_hip.h) -- one knob:
#   PREC_FP16  0  single fp16 operands, the guided forward as independent streams (1.4e-3 token mismatch on configs[2]: a baseline, not a product mode)
#   PREC_DIFF  1  classifier-free guidance in differential form; plain forwards with the LayerNorm outputs as fp16 hi + lo pairs (~1.0e-3: AT the bound)
#   PREC_WCORR 2  + MX-fp4 weight-correction mini-tiles on every trunk GEMM, guided and plain (5.5e-4 over three reference runs of configs[2]; 5.3e-4 on configs[1])
#   PREC_ALO   3  + activation-lo mini-tiles in out-proj (attention outputs) and FFN-up (LayerNorm outputs) of every layer of the guided forward (3.8e-4 over four 14-bit / 256-step runs)
#   PREC_ALO_ALL 4 + activation-lo mini-tiles in FFN-down (FFN hiddens) as well, zero-scale steps through the guided forward: heavy-tailed checkpoints
#   PREC_F32   5  the fp32 REFERENCE mode: fp32 weights, fp32 workspace, every GEMM an ascending-k fmaf chain on the f32-input MFMA -- any shape, about 1/16
#                 of the fp16 rate; what check_checkpoint() measures the other modes against.  Only ever chosen explicitly.
# -1 = auto: 2, or 3 from 7 bits per group on, or 4 when the checkpoint's statistics ask for it (weight_statistics()), degraded to what the shape allows
# (resolved_precision()).
PREC_AUTO, PREC_FP16, PREC_DIFF, PREC_WCORR, PREC_ALO, PREC_ALO_ALL, PREC_F32 = -1, 0, 1, 2, 3, 4, 5
# Load-time escalation rule of the auto mode (round 6).  What the default modes are sensitive to, and Gaussian-like weights do not show: (a) HEAVY-TAILED
# Linear weights -- an fp16 rounding error is +-ulp(w) / 2, so a few large weights per row set the scale of the e2m1 weight-error operand for the rest
# (residual 9 % of the error energy at kurtosis 10.9 against 3 % at 3); measured as the pooled kurtosis of the trunk's Linear weights standardised per
# row; (b) MASSIVE-ACTIVATION channels -- LayerNorm outputs sqrt(gamma^2 + beta^2) many times the typical channel's: they take the resolution of their
# 64-column block in every e2m1 token operand.  A Gaussian / trunc-normal init measures 2.9-3.0 and 1.0-1.1; the trained-like family of maskbit_amd/synth.py
# 10.9 and ~16; the thresholds sit where a Student-t_8 weight distribution (kurtosis 4.5) or one channel at 6x the median would.
ESCALATE_KURTOSIS = 4.5
ESCALATE_CHANNEL_RATIO = 6.0
DEFAULT_PRECISION = PREC_AUTO


def pair_capable(seq_len: int, hidden: int, mlp: int, prenorm: bool) -> bool:
    """Shapes the differential guided forward serves (mb_gen_create: pair_ok); post- and (round 4) pre-norm."""
    return seq_len in (256, 1024) and hidden in (768, 1024) and mlp % 256 == 0


def mini_capable(seq_len: int, hidden: int, mlp: int, heads: int) -> bool:
    """Shapes the MX-fp4 mini-tile passes serve (mb_gen_create: mini_ok)."""
    return seq_len in (256, 1024) and hidden in (768, 1024) and mlp % 256 == 0 and hidden // heads == 64


def _generator_specs(d: int, f: int, depth: int, seq: int, bits: int, nclass: int, out: int, prenorm: bool = False,
                     tables: int = 0, codes: int = 0) -> List[ParamSpec]:
    """Checkpoint entries in the reference's registration order.  ``tables`` > 0: the embedding-table `Bert` (bert.py:222-262)
    with that many groups of ``codes`` + 1 rows; otherwise LFQBert (bert.py:386-417)."""
    s: List[ParamSpec] = []
    if tables:
        s += [("class_emb.weight", (nclass + 1, d), "normal")]
        s += [(f"tok_emb_list.{g}.weight", (codes + 1, d), "normal") for g in range(tables)]
        s += [("pos_emb", (1, seq + 1, d), "normal")]
    else:
        s += [("pos_emb", (1, seq + 1, d), "normal"), ("class_emb.weight", (nclass + 1, d), "normal"),
              ("input_proj.weight", (d, bits), "normal"), ("input_proj.bias", (d,), "zeros")]
    s += [("first_layer.0.weight", (d,), "ones"), ("first_layer.0.bias", (d,), "zeros")]
    for l in range(depth):
        a, m = f"transformer.layers.{l}.0", f"transformer.layers.{l}.1"
        s += [(a + ".mha.in_proj_weight", (3 * d, d), "normal"), (a + ".mha.in_proj_bias", (3 * d,), "zeros"),
              (a + ".mha.out_proj.weight", (d, d), "normal"), (a + ".mha.out_proj.bias", (d,), "zeros"),
              (a + ".norm.weight", (d,), "ones"), (a + ".norm.bias", (d,), "zeros"),
              (m + ".net.0.weight", (f, d), "normal"), (m + ".net.0.bias", (f,), "zeros"),
              (m + ".net.2.weight", (d, f), "normal"), (m + ".net.2.bias", (d,), "zeros"),
              (m + ".norm.weight", (d,), "ones"), (m + ".norm.bias", (d,), "zeros")]
    if prenorm:
        s += [("norm_after_transformer.weight", (d,), "ones"), ("norm_after_transformer.bias", (d,), "zeros")]
    s += [("last_layer.0.weight", (d, d), "normal"), ("last_layer.0.bias", (d,), "zeros"),
          ("last_layer.2.weight", (d,), "ones"), ("last_layer.2.bias", (d,), "zeros")]
    if tables:
        s += [(f"bias.{g}", (seq, codes), "zeros") for g in range(tables)]
    else:
        s += [("prediction_layer.weight", (out, d), "normal"), ("prediction_layer.bias", (out,), "zeros")]
    return s


class LFQBert(BaseModel):
    _ABI = "gen"
    _COUNTS = "lanes of the trunk's fp16 QKV / FFN-up epilogues that clamped a value: 0 for every configuration tested"

    def __init__(self, img_size=256, hidden_dim=768, codebook_size=1024, codebook_splits=1, depth=24, heads=8,
                 mlp_dim=3072, dropout=0.1, nclass=1000, input_stride: int = 16, use_prenorm: bool = False):
        super().__init__()
        self.nclass = nclass
        self.drop_label = nclass
        self.seq_len = (img_size // input_stride) ** 2
        self.splits = codebook_splits
        self.bits = int(math.log2(codebook_size))
        if self.bits % self.splits:
            raise ValueError(f"log2(codebook_size)={self.bits} is not divisible by codebook_splits={self.splits}")
        group_bits = self.bits // self.splits
        self.effective_codebook_size = 2 ** group_bits
        self.mask_token = self.effective_codebook_size
        self.hidden_dim, self.depth, self.heads, self.mlp_dim = hidden_dim, depth, heads, mlp_dim
        self.dropout = dropout            # inference only: dropout is the identity in eval mode
        self.use_prenorm = bool(use_prenorm)
        self.embed_tables = bool(getattr(self, "_EMBED_TABLES", False))
        # Precision mode of the device engine (not a reference argument; see PREC_* above).  Default from MASKBIT_AMD_PRECISION; may be changed before a
        # call (the engine is rebuilt and the checkpoint repacked).
        self.precision = int(os.environ.get("MASKBIT_AMD_PRECISION", str(DEFAULT_PRECISION)))
        self._engine_split = None
        self._wstats = None               # (weight signature, statistics) of the last weight_statistics() call
        if not self.embed_tables:
            self._attach("bits_to_indices", (2 ** torch.arange(group_bits)).to(torch.int32), buffer=True)
        self._build(_generator_specs(hidden_dim, mlp_dim, depth, self.seq_len, self.bits, nclass,
                                     self.splits * self.effective_codebook_size, prenorm=self.use_prenorm,
                                     tables=self.splits if self.embed_tables else 0, codes=self.effective_codebook_size))

    def get_group_splits(self) -> int:
        return self.splits

    # ---- engine hooks ---------------------------------------------------------------------
    def _engine_create(self, capacity: int):
        cfg = _lib.GenCfg(self.bits, self.splits, self.hidden_dim, self.heads, self.depth, self.mlp_dim, self.seq_len, self.nclass,
                          int(self.use_prenorm), int(self.embed_tables), self.resolved_precision())
        self._engine_split = self.resolved_precision()
        h = C.c_void_p()
        _lib.check(_lib.load().mb_gen_create(C.byref(cfg), capacity, C.byref(h)), "mb_gen_create")
        return h

    @torch.no_grad()
    def weight_statistics(self) -> dict:
        """Statistics of the CHECKPOINT the auto precision mode escalates on (cached per weight signature): ``kurtosis`` = pooled fourth moment of the trunk's
        Linear weights (in_proj, out_proj, net.0, net.2 of every layer) standardised per output row (a Gaussian's: 3); ``channel_ratio`` = the largest
        LayerNorm output channel magnitude sqrt(gamma^2 + beta^2) over the median channel's, maximised over the trunk's LayerNorms."""
        sig = self._weight_signature()
        if self._wstats is not None and self._wstats[0] == sig:
            return self._wstats[1]
        sd = self.state_dict(keep_vars=True)
        m4 = n = 0.0
        ratio = 1.0
        for k, t in sd.items():
            if not (t.is_floating_point() and k.startswith("transformer.layers.")):
                continue
            w = t.detach().float()
            if w.dim() == 2:
                z = w - w.mean(1, keepdim=True)
                z = z / z.pow(2).mean(1, keepdim=True).clamp_min(1e-30).sqrt()
                m4 += float(z.pow(4).sum()); n += z.numel()
            elif k.endswith("norm.weight"):
                mag = (w.pow(2) + sd[k[:-6] + "bias"].detach().float().pow(2)).sqrt()
                ratio = max(ratio, float(mag.max() / mag.median().clamp_min(1e-30)))
        stats = {"kurtosis": m4 / max(n, 1.0), "channel_ratio": ratio}
        stats["heavy_tailed"] = stats["kurtosis"] > ESCALATE_KURTOSIS or stats["channel_ratio"] > ESCALATE_CHANNEL_RATIO
        self._wstats = (sig, stats)
        return stats

    def resolved_precision(self) -> int:
        """The precision mode handed to the engine.  The default (-1) means "meet the <= 1e-3 token mismatch with margin": the fp16 rounding of the trunk
        WEIGHTS is ~80 % of the sampled-logit error variance in every configuration (tests/diag/error_budget.py), so wherever the shape allows it every
        trunk GEMM carries the MX-fp4 weight-correction mini-tiles (PREC_WCORR; PREC_ALO from 7 bits per group on) -- guided forwards in differential form,
        plain forwards with the LayerNorm outputs as fp16 hi + lo pairs as well.  Measured (profiles/r04_parity.md, r05): 12-bit / 64 steps 5.5e-4 over
        three reference runs, 10-bit / 16 steps / no guidance 5.3e-4, 14-bit / 256 steps 5.5e-4, the 1024 + 1-token models 5.6e-4.  Shapes the mini-tile
        kernels do not serve fall back to the differential form alone, shapes the pair tiles do not serve to independent streams (with hi + lo LayerNorm
        outputs: the engine keeps those for every requested precision >= 1).
        Round 6: the default ESCALATES to PREC_ALO_ALL from the checkpoint's own statistics (weight_statistics(): heavy-tailed Linear weights or
        massive-activation channels) -- on such weights the lower modes sit at or over the bound (two trained-like 12-bit runs 7.2e-4 / 1.06e-3 at
        precision 2; profiles/r06_parity.md for precision 4)."""
        capable = pair_capable(self.seq_len, self.hidden_dim, self.mlp_dim, self.use_prenorm)
        mini = mini_capable(self.seq_len, self.hidden_dim, self.mlp_dim, self.heads)
        prec = int(self.precision)
        if prec == PREC_F32:
            return prec                                            # the fp32 reference mode serves every shape: no fallback touches it
        if prec < 0:
            prec = PREC_ALO if self.bits // self.splits >= 7 else PREC_WCORR
            if capable and mini and self.weight_statistics()["heavy_tailed"]:
                prec = PREC_ALO_ALL
        if prec >= PREC_WCORR and not (capable and mini):
            prec = PREC_DIFF
        return prec

    def engine(self, min_seqs: int):
        """Device engine able to hold ``min_seqs`` sequences (CFG needs 2 x batch)."""
        self._sig_hint = None
        self._sig_hint = self._weight_signature()                  # one walk over the parameters for the auto rule AND the reload check of this call
        try:
            if self._engine is not None and self._engine_split != self.resolved_precision():
                self._drop_engine()                                # precision mode changed (the knob, or new weights under the auto rule): rebuild and repack
            have = self._engine_key[1] if self._engine_key else 0
            h = self._ensure_engine(max(min_seqs, have, 16))
        finally:
            self._sig_hint = None
        return h

    def _check_labels(self, labels: torch.Tensor) -> None:
        """Host-resident labels are range-checked here (an out-of-range class would index past class_emb, where the
        reference raises an IndexError); device-resident labels are clamped inside the kernel instead of forcing a sync."""
        if labels.device.type == "cpu" and labels.numel() and (int(labels.min()) < 0 or int(labels.max()) > self.nclass):
            raise IndexError(f"class label outside [0, {self.nclass}]")

    # ---- forward ----------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, img_tokens: torch.Tensor, class_labels: torch.Tensor,
                drop_label_mask: Optional[torch.Tensor] = None, return_attn: bool = False):
        """-> logits [b, seq, m, C]; with ``return_attn`` (bert.py:461, 505-508) the tuple (logits, [one head-averaged attention map
        [b, seq+1, seq+1] per layer]) -- the maps come from a separate plain kernel reading the same Q/K rows."""
        dev = self._require_cuda("forward")
        if img_tokens.dim() != 3 or img_tokens.shape[1] != self.seq_len or img_tokens.shape[2] != self.splits:
            raise ValueError(f"img_tokens must be [b, {self.seq_len}, {self.splits}], got {tuple(img_tokens.shape)}")
        b = img_tokens.shape[0]
        if class_labels.numel() != b:
            raise ValueError(f"class_labels must hold {b} labels, got {tuple(class_labels.shape)}")
        self._check_labels(class_labels)
        if self.embed_tables and img_tokens.device.type == "cpu" and img_tokens.numel() and \
                (int(img_tokens.min()) < 0 or int(img_tokens.max()) > self.effective_codebook_size):
            raise IndexError(f"token outside [0, {self.effective_codebook_size}]")          # nn.Embedding would raise (bert.py:313)
        toks = img_tokens.to(device=dev, dtype=torch.int64).contiguous()
        labs = class_labels.to(device=dev, dtype=torch.int64).reshape(b).contiguous()     # never mutated (cf. bert.py:482-484)
        drop = None
        if drop_label_mask is not None:
            drop = drop_label_mask.to(device=dev).reshape(b).to(torch.uint8).contiguous()
        logits = torch.empty((b, self.seq_len, self.splits, self.effective_codebook_size), dtype=torch.float32, device=dev)
        h = self.engine(b)
        with torch.cuda.device(dev):
            if return_attn:
                n1 = self.seq_len + 1
                attn = torch.empty((self.depth, b, n1, n1), dtype=torch.float32, device=dev)
                _lib.check(_lib.load().mb_gen_forward_attn(h, toks.data_ptr(), labs.data_ptr(), drop.data_ptr() if drop is not None else None,
                                                           logits.data_ptr(), attn.data_ptr(), b, torch.cuda.current_stream().cuda_stream),
                           "mb_gen_forward_attn")
                return logits, list(attn.unbind(0))
            _lib.check(_lib.load().mb_gen_forward(h, toks.data_ptr(), labs.data_ptr(), drop.data_ptr() if drop is not None else None,
                                                  logits.data_ptr(), b, torch.cuda.current_stream().cuda_stream), "mb_gen_forward")
        return logits


    @torch.no_grad()
    def forward_cfg(self, img_tokens: torch.Tensor, class_labels: torch.Tensor) -> torch.Tensor:
        """The guided forward of sample() (sampling.py:83-88) in one call: logits [2b, seq, m, C], rows [0, b) = model(tokens, labels, ~drop),
        rows [b, 2b) = the label-dropped forward of the same tokens.  On the engine the two streams run in differential form (precision >= 1),
        whatever guidance scale the caller combines them with."""
        dev = self._require_cuda("forward_cfg")
        if img_tokens.dim() != 3 or img_tokens.shape[1] != self.seq_len or img_tokens.shape[2] != self.splits:
            raise ValueError(f"img_tokens must be [b, {self.seq_len}, {self.splits}], got {tuple(img_tokens.shape)}")
        b = img_tokens.shape[0]
        if class_labels.numel() != b:
            raise ValueError(f"class_labels must hold {b} labels, got {tuple(class_labels.shape)}")
        self._check_labels(class_labels)
        toks = img_tokens.to(device=dev, dtype=torch.int64).contiguous()
        labs = class_labels.to(device=dev, dtype=torch.int64).reshape(b).contiguous()
        logits = torch.empty((2 * b, self.seq_len, self.splits, self.effective_codebook_size), dtype=torch.float32, device=dev)
        h = self.engine(2 * b)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mb_gen_forward_cfg(h, toks.data_ptr(), labs.data_ptr(), logits.data_ptr(), b,
                                                      torch.cuda.current_stream().cuda_stream), "mb_gen_forward_cfg")
        return logits


class Bert(LFQBert):
    """The embedding-table generator (reference bert.py:184-340): per-group ``nn.Embedding(C + 1, hidden)`` inputs summed, the
    output head tied to those tables (``x @ tok_emb.weight.T[:, :C]``) plus a per-position bias [seq, C].  Same trunk, same
    engine: only the embed kernel's input mode and the head GEMM's weight / bias sources differ."""
    _EMBED_TABLES = True
