"""Checkpoint self-check: does a precision mode hold the token-mismatch bound on THESE weights?

Every parity figure of the engine's precision modes (``bert.PREC_*``) was measured on synthetic weight families against recorded runs of the
reference.  ``check_checkpoint`` measures the same figure on the checkpoint a model actually holds, with the engine's own fp32 reference mode
(``PREC_F32``: fp32 weights and workspace, every GEMM an ascending-k fmaf chain on the f32-input MFMA) in the reference's place:

  1. the run's noise is drawn once with the reference's protocol (``parity_replay.reference_noise``: per step one ``exponential_`` [B n m, C], then
     one Gumbel [B, n, m], CPU default generator seeded with ``seed``);
  2. a run is RECORDED at precision 5 by a host-driven loop of ``forward_cfg`` / ``forward`` + ``mb_sample_step``, each step fed the previous step's
     output tokens -- kept in the dict layout ``parity_replay.load_run`` returns;
  3. every precision asked for is TEACHER-FORCED against the record (``parity_replay.teacher_forced``): each step restarts from the record's masked
     state, mismatches are counted over the positions sampled at that step;
  4. the model's ``precision`` is put back.

What it proves: how often this checkpoint's fp16 / e2m1 arithmetic flips a sampled token against an fp32 evaluation of the same network on the
same noise.  What it does not: the record is this engine's fp32 mode, not the reference's code -- its own fp32 rounding differs from the
reference's fp32 rounding, a difference two orders of magnitude below the modes' (tests/test_hip_f32_reference.py) -- and one run of ``num_samples``
samples bounds the rate only as far as its position count allows (the report carries a one-sided 95 % Poisson upper limit for that reason).
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, parity_replay
from .bert import PREC_ALO, PREC_ALO_ALL, PREC_AUTO, PREC_F32, PREC_WCORR, LFQBert, mini_capable, pair_capable

# the sampler settings of a default check: configs[2]'s (the 64-step guided run the parity figures are quoted for)
DEFAULT_SAMPLER = dict(num_steps=64, guidance_scale=7.1, guidance_annealing="cosine", scale_pow=3.0, randomize_temperature=8.2,
                       mask_schedule_strategy="arccos")


def poisson_upper_limit(k: int, confidence: float = 0.95) -> float:
    """One-sided upper limit on the mean of a Poisson variable observed as ``k``: the mu with P(X <= k | mu) = 1 - confidence, by bisection on the
    tail summed in log space.  k = 0: -ln(0.05) = 2.996."""
    if k < 0:
        raise ValueError("k must be >= 0")
    alpha = 1.0 - confidence
    i = torch.arange(k + 1, dtype=torch.float64)
    lg = torch.lgamma(i + 1.0)

    def cdf(mu: float) -> float:
        return float(torch.exp(torch.logsumexp(i * math.log(mu) - mu - lg, 0)))

    lo, hi = max(float(k), 1e-12), float(k) + 10.0 * math.sqrt(k + 1.0) + 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if cdf(mid) > alpha:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-12 * hi:
            break
    return 0.5 * (lo + hi)


@dataclass
class PrecisionResult:
    precision: int
    mismatches: int
    positions: int
    per_step: List[int] = field(default_factory=list)
    remask: int = 0
    saturation: int = 0
    seconds: float = 0.0

    @property
    def rate(self) -> float:
        return self.mismatches / max(self.positions, 1)

    @property
    def upper_limit(self) -> float:
        """One-sided 95 % Poisson upper limit on the mismatch rate."""
        return poisson_upper_limit(self.mismatches) / max(self.positions, 1)


@dataclass
class CheckpointReport:
    results: Dict[int, PrecisionResult]
    auto_precision: int
    bound: float = 1e-3
    weight_statistics: Optional[dict] = None
    record_seconds: float = 0.0
    record: Optional[dict] = None          # the precision-5 run (parity_replay.load_run layout)

    @classmethod
    def from_counts(cls, counts: Dict[int, Tuple[int, int]], auto_precision: int, bound: float = 1e-3, **kw) -> "CheckpointReport":
        """A report from {precision: (mismatches, positions)} alone."""
        return cls({p: PrecisionResult(p, int(k), int(n)) for p, (k, n) in counts.items()}, auto_precision, bound, **kw)

    @property
    def holds(self) -> Dict[int, bool]:
        return {p: r.upper_limit <= self.bound for p, r in self.results.items()}

    @property
    def recommended(self) -> Optional[int]:
        """The lowest precision whose upper limit holds the bound; None if none does."""
        ok = [p for p, h in sorted(self.holds.items()) if h]
        return ok[0] if ok else None

    @property
    def default_ok(self) -> Optional[bool]:
        """Whether the precision the auto rule resolves to holds the bound (None: it was not among the precisions checked)."""
        return self.holds.get(self.auto_precision)

    def __str__(self) -> str:
        lines = []
        if self.weight_statistics:
            s = self.weight_statistics
            lines.append(f"weights: kurtosis {s['kurtosis']:.2f}, channel ratio {s['channel_ratio']:.2f}, heavy-tailed {s['heavy_tailed']}")
        lines.append(f"auto precision {self.auto_precision}; bound {self.bound:.1e}; reference: precision {PREC_F32} (fp32), recorded in {self.record_seconds:.1f} s")
        lines.append(f"{'prec':>4} {'mismatch':>9} {'positions':>10} {'rate':>9} {'95% upper':>10} {'holds':>6} {'sat':>5} {'s':>7}")
        holds = self.holds
        for p in sorted(self.results):
            r = self.results[p]
            lines.append(f"{p:>4} {r.mismatches:>9} {r.positions:>10} {r.rate:>9.2e} {r.upper_limit:>10.2e} {str(holds[p]):>6} {r.saturation:>5} {r.seconds:>7.2f}"
                         + ("  <- auto" if p == self.auto_precision else ""))
        lines.append(f"recommended precision: {self.recommended}; default ok: {self.default_ok}")
        return "\n".join(lines)


def record_dict(steps: torch.Tensor, masks: torch.Tensor, labels: torch.Tensor, kw: Dict[str, object], seed: int, bits: int, C: int) -> dict:
    """A run in the layout ``parity_replay.load_run`` returns: steps int64 [S, B, n, m] = the tokens predicted per step, masks bool [S, B, n, m] =
    the positions that were masked in the step's INPUT, kw = the sampler settings as strings."""
    return {"name": "self-recorded", "steps": steps, "masks": masks, "labels": labels, "kw": {str(k): str(v) for k, v in kw.items()},
            "seed": int(seed), "bits": int(bits), "C": int(C), "n": int(steps.shape[2])}


@torch.no_grad()
def record_run(model: LFQBert, labels: torch.Tensor, seed: int = 0, **sample_kwargs) -> Tuple[dict, Tuple[torch.Tensor, torch.Tensor]]:
    """The model's run at its CURRENT precision on the reference-protocol noise of ``seed``, driven from the host step by step (what ``mb_sample`` runs
    on the device, bit for bit).  -> (record, (exp_noise, conf_noise))."""
    lib = _lib.load()
    dev = model._require_cuda("record_run")
    kw = dict(DEFAULT_SAMPLER, **sample_kwargs)
    S, B, n, m, C_ = int(kw["num_steps"]), int(labels.numel()), model.seq_len, model.splits, model.effective_codebook_size
    labels = labels.reshape(B).to(torch.int64).cpu()
    g = record_dict(torch.zeros((S, B, n, m), dtype=torch.int64), torch.zeros((S, B, n, m), dtype=torch.bool), labels, kw, seed, model.bits, C_)
    noise = parity_replay.reference_noise(g, dev)
    scale, temp, mask_len = parity_replay.plan_of(g)
    guided = float(kw["guidance_scale"]) != 0.0
    y = labels.to(dev)
    tin = torch.full((B, n, m), C_, dtype=torch.int64, device=dev)
    nodrop = torch.zeros(B, dtype=torch.bool, device=dev)
    for i in range(S):
        if guided and scale[i] != 0.0:
            lg = model.forward_cfg(tin, y)
            lc, lu = lg[:B].contiguous(), lg[B:].contiguous()
        else:                                                       # (as mb_sample: a zero-scale step is the conditional forward alone)
            lc, lu = model(tin, y, nodrop), None
        tout, pred = torch.empty_like(tin), torch.empty_like(tin)
        _lib.check(lib.mb_sample_step(lc.data_ptr(), lu.data_ptr() if lu is not None else None, scale[i], temp[i], noise[0][i].data_ptr(),
                                      noise[1][i].data_ptr(), mask_len[i], tin.data_ptr(), tout.data_ptr(), pred.data_ptr(), B, n, m, C_,
                                      torch.cuda.current_stream().cuda_stream), "mb_sample_step")
        g["steps"][i] = pred.cpu()
        g["masks"][i] = (tin == C_).cpu()
        tin = tout
    return g, noise


def default_precisions(model: LFQBert) -> List[int]:
    """The auto-resolved precision plus 2, 3, 4 where the shape serves them."""
    keep = model.precision
    try:
        model.precision = PREC_AUTO
        ps = {model.resolved_precision()}
    finally:
        model.precision = keep
    if pair_capable(model.seq_len, model.hidden_dim, model.mlp_dim, model.use_prenorm) and mini_capable(model.seq_len, model.hidden_dim, model.mlp_dim, model.heads):
        ps |= {PREC_WCORR, PREC_ALO, PREC_ALO_ALL}
    return sorted(ps)


@torch.no_grad()
def check_checkpoint(model: LFQBert, *, num_samples: int = 8, labels: Optional[torch.Tensor] = None, seed: int = 0,
                     precisions: Optional[Sequence[int]] = None, bound: float = 1e-3, **sample_kwargs) -> CheckpointReport:
    """Measure the token-mismatch rate of ``precisions`` (default: ``default_precisions``) on the model's own weights against a run recorded in the
    fp32 reference mode.  ``labels``: ``num_samples`` class ids (default: drawn from ``seed``); ``sample_kwargs``: num_steps, guidance_scale,
    guidance_annealing, scale_pow, randomize_temperature, mask_schedule_strategy (default ``DEFAULT_SAMPLER``).  The model's ``precision`` is restored."""
    if not isinstance(model, LFQBert):
        raise TypeError(f"check_checkpoint() needs a maskbit_amd LFQBert / Bert generator, got {type(model).__name__}")
    unknown = set(sample_kwargs) - set(DEFAULT_SAMPLER)
    if unknown:
        raise TypeError(f"check_checkpoint() got unexpected sampler arguments {sorted(unknown)}")
    if labels is None:
        labels = torch.randint(0, model.nclass, (num_samples,), generator=torch.Generator().manual_seed(seed))
    if labels.numel() != num_samples:
        raise ValueError(f"{labels.numel()} labels for num_samples={num_samples}")
    model._check_labels(labels.cpu())
    keep = model.precision
    try:
        model.precision = PREC_AUTO
        auto = model.resolved_precision()
        stats = dict(model.weight_statistics())
        todo = sorted(set(int(p) for p in precisions)) if precisions is not None else default_precisions(model)
        if any(p < 0 or p >= PREC_F32 for p in todo):
            raise ValueError(f"precisions must lie in 0 .. {PREC_F32 - 1}, got {todo}")
        model.precision = PREC_F32
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        record, noise = record_run(model, labels, seed, **sample_kwargs)
        torch.cuda.synchronize()
        t_rec = time.perf_counter() - t0
        results = {}
        for p in todo:
            model.precision = p
            model.engine(1)                                          # (the rebuild and repack is not part of the replay's time)
            model.saturation_count(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mism, total, per_step, remask = parity_replay.teacher_forced(model, g=record, noise=noise)
            torch.cuda.synchronize()
            results[p] = PrecisionResult(p, mism, total, per_step, remask, model.saturation_count(), time.perf_counter() - t0)
    finally:
        model.precision = keep
    return CheckpointReport(results, auto, bound, stats, t_rec, record)
