"""Restatement of the two reference functions behind masked-token validation, in this project's words: the yardstick of tests/test_mlm_cpu.py
and tests/test_hip_mlm.py for inputs that have no golden.

``mask_tokens_ref``: modeling/modules/masking.py:7-38.  The draws and the float32 threshold are part of the contract (they decide which
slots are masked), so they are made exactly as the reference makes them; only the select is restated.
``mlm_loss64``: modeling/modules/losses.py:319-337 in float64: label-smoothed cross entropy and argmax accuracy over all rows and over the
masked rows."""
import functools
import math

import numpy as np
import torch

from conftest import load_golden
from maskbit_amd.synth import make_mlm_case, make_mlm_tokens

KEYS = ("mlm_loss", "correct_tokens", "masked_token_loss", "masked_correct_tokens")
CONFIGS = ((0.1, False), (0.0, True), (0.1, True))            # (label_smoothing, sum_splits) of every golden loss case


@functools.lru_cache(maxsize=None)
def mlm_golden():
    return load_golden("mlm.npz")


def unpack_mask(packed, shape) -> torch.Tensor:
    count = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(packed)[:count].astype(bool)).reshape(tuple(int(v) for v in shape))


def loss_case(name):
    """-> (logits fp32 [b, n, m, C], targets int64 [b, n, m], mask bool [b, n, m]) of a golden loss case: inputs regenerated from the recorded
    seed, the mask as the reference drew it."""
    z = mlm_golden()
    b, n, m, C, seed = (int(v) for v in z[name + ".params"][:5])
    logits, targets = make_mlm_case(b, n, m, C, seed)
    return logits, targets, unpack_mask(z[name + ".mask"], (b, n, m))


def mask_case(name):
    """-> (tokens, mask_token, mode, min_masking_ratio, seed) of a golden mask case."""
    z = mlm_golden()
    b, n, m, C, tok_seed, seed = (int(v) for v in z[name + ".params"])
    return make_mlm_tokens(b, n, m, C, tok_seed), C, str(z[name + ".mode"]), float(z[name + ".min_masking_ratio"]), seed


def mask_tokens_ref(tokens: torch.Tensor, mask_token: int, mode: str = "arccos", min_masking_ratio: float = 0.0, generator=None):
    """-> (masked_tokens, mask, val_to_mask): one uniform per sample through the schedule gives the sample's threshold, one uniform per slot
    below it masks the slot."""
    r = torch.rand(tokens.shape[0], generator=generator) * (1 - min_masking_ratio)
    schedule = {"linear": lambda: 1 - r, "square": lambda: 1 - r ** 2, "cosine": lambda: torch.cos(r * math.pi * 0.5),
                "arccos": lambda: torch.acos(r) / (math.pi * 0.5)}
    if mode not in schedule:
        raise ValueError(f"unknown mode {mode!r}")
    val = schedule[mode]()
    mask = torch.rand(tokens.shape, generator=generator) < val.reshape([-1] + [1] * (tokens.dim() - 1))
    return torch.where(mask, torch.full_like(tokens, mask_token), tokens), mask, val


def row_losses64(logits: torch.Tensor, targets: torch.Tensor, label_smoothing: float):
    """float64 per-row loss [rows] and whether the row's first maximum is its target [rows]."""
    x = logits.double().reshape(-1, logits.shape[-1])
    t = targets.reshape(-1)
    lse = torch.logsumexp(x, dim=-1)
    nll = lse - x.gather(1, t.unsqueeze(1)).squeeze(1)
    loss = nll
    if label_smoothing > 0:
        loss = (1.0 - label_smoothing) * nll + label_smoothing * (lse - x.mean(dim=-1))
    return loss, x.argmax(dim=-1) == t


def mlm_loss64(logits, targets, masks, label_smoothing: float = 0.1, sum_splits: bool = False) -> dict:
    """The four figures as Python floats (float64), and the integer counts ``rows``, ``masked``, ``correct``, ``masked_correct``."""
    m = logits.shape[2]
    loss, hit = row_losses64(logits, targets, label_smoothing)
    mk = masks.reshape(-1).bool()
    scale = float(m) if sum_splits else 1.0
    rows, masked = loss.numel(), int(mk.sum())
    correct, masked_correct = int(hit.sum()), int(hit[mk].sum())
    nan = float("nan")
    return {"mlm_loss": float(loss.sum() / rows) * scale, "correct_tokens": (correct / rows) ** m,
            "masked_token_loss": float(loss[mk].sum() / masked) * scale if masked else nan,
            "masked_correct_tokens": (masked_correct / masked) ** m if masked else nan,
            "rows": rows, "masked": masked, "correct": correct, "masked_correct": masked_correct}


def loss_bound() -> float:
    """The relative bound of the two losses against ref64: 4 x the largest E_rel of the golden, E_rel = |ref32 - ref64| / |ref64| = the
    reference's own float32 evaluation error."""
    z = mlm_golden()
    return 4.0 * max(float(z[str(n) + ".E_rel"].max()) for n in z["loss_cases"])
