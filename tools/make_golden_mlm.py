"""Golden fixture of masked-token validation: the reference's ``get_mask_tokens`` (modeling/modules/masking.py:7-38) and ``MLMLoss``
(modeling/modules/losses.py:289-339) run on the CPU on seeded inputs.  Needs the reference checkout (MASKBIT_REFERENCE, as
oracle/make_golden.py); writes results only (a few KB) to tests/golden/mlm.npz -- the tests regenerate the inputs from the recorded seeds
(maskbit_amd.synth.make_mlm_case / make_mlm_tokens).

Per loss case (b, n, m, C), with the mask the reference draws under ``torch.manual_seed(mask_seed)`` (bit-packed), and for each
(label_smoothing, sum_splits) of CONFIGS, the four figures [mlm_loss, correct_tokens, masked_token_loss, masked_correct_tokens] of
  ref32  the reference as it runs,
  ref64  the same module on ``.double()`` logits,
the integer counts [rows, masked, correct, masked_correct], and E_rel = |ref32 - ref64| / |ref64| of the two losses: the reference's own fp32
evaluation error, the unit of the tests' loss bound.  Asserted on the inputs: no row has two equal largest logits; every case has a masked and
an unmasked row.  Per mask case the reference's ``val_to_mask`` (recomputed from the same draw: the function does not return it) and its mask.

    python tools/make_golden_mlm.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from maskbit_amd.synth import make_mlm_case, make_mlm_tokens  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mlm.npz")

# name -> (b, n, m, C, input seed, mask seed)
LOSS_CASES = {
    "b3n16m2c64": (3, 16, 2, 64, 3000, 3100),
    "b2n256m2c128": (2, 256, 2, 128, 3001, 3101),
    "b2n16m1c1024": (2, 16, 1, 1024, 3002, 3102),
    "b3n7m3c16": (3, 7, 3, 16, 3003, 3103),                 # 21 rows per sample: not a multiple of the rows per wave
    "b2n16m2c512": (2, 16, 2, 512, 3004, 3104),
    "b3n16m1c10": (3, 16, 1, 10, 3005, 3105),               # scalar path
    "b2n8m1c4100": (2, 8, 1, 4100, 3006, 3106),             # several passes over the row, with a tail
}
CONFIGS = ((0.1, False), (0.0, True), (0.1, True))          # (label_smoothing, sum_splits)
KEYS = ("mlm_loss", "correct_tokens", "masked_token_loss", "masked_correct_tokens")

# name -> (b, n, m, C, token seed, mask seed, mode, min_masking_ratio)
MASK_CASES = {}
for _s, (_b, _n, _m) in enumerate(((5, 16, 2), (3, 256, 3))):
    for _k, (_mode, _min) in enumerate((("linear", 0.0), ("square", 0.0), ("cosine", 0.0), ("arccos", 0.0), ("arccos", 0.5))):
        MASK_CASES[f"{_mode}{'_min50' if _min else ''}_{_b}x{_n}x{_m}"] = (_b, _n, _m, 64, 3200 + _s, 3300 + 10 * _s + _k, _mode, _min)


def val_to_mask_of(batch, mode, min_masking_ratio):
    """masking.py:22-30 on the draw the reference is about to make (call under the same seed)."""
    r = torch.rand(batch) * (1 - min_masking_ratio)
    return {"linear": lambda: 1 - r, "square": lambda: 1 - (r ** 2), "cosine": lambda: torch.cos(r * math.pi * 0.5),
            "arccos": lambda: torch.acos(r) / (math.pi * 0.5)}[mode]()


def main():
    MG._import_reference()
    from modeling.modules import MLMLoss, get_mask_tokens
    import modeling
    assert os.path.realpath(modeling.__file__).startswith(os.path.realpath(MG.REF))
    torch.set_grad_enabled(False)
    out = dict(loss_cases=np.array(list(LOSS_CASES)), mask_cases=np.array(list(MASK_CASES)),
               configs=np.array([[ls, float(ss)] for ls, ss in CONFIGS], dtype=np.float64))
    for name, (b, n, m, C, seed, mask_seed) in LOSS_CASES.items():
        logits, targets = make_mlm_case(b, n, m, C, seed)
        top2 = logits.topk(2, dim=-1).values
        assert bool((top2[..., 0] > top2[..., 1]).all()), f"{name}: a row with two equal largest logits"
        torch.manual_seed(mask_seed)
        masked, mask = get_mask_tokens(targets, C, mode="arccos")
        assert bool(mask.any()) and not bool(mask.all()), f"{name}: needs a masked and an unmasked row"
        assert bool((masked[mask] == C).all()) and bool((masked[~mask] == targets[~mask]).all())
        hit = logits.argmax(-1) == targets
        out[name + ".params"] = np.array([b, n, m, C, seed, mask_seed], dtype=np.int64)
        out[name + ".mask"] = np.packbits(mask.numpy().reshape(-1))
        out[name + ".counts"] = np.array([hit.numel(), int(mask.sum()), int(hit.sum()), int(hit[mask].sum())], dtype=np.int64)
        ref = {}
        for tag, dbl in (("ref32", False), ("ref64", True)):
            rows = []
            for ls, ss in CONFIGS:
                _, d = MLMLoss(label_smoothing=ls, sum_splits=ss)(logits.double() if dbl else logits.clone(), targets, mask)
                assert tuple(d) == KEYS
                rows.append([float(d[k]) for k in KEYS])
            ref[tag] = out[f"{name}.{tag}"] = np.array(rows, dtype=np.float64)
        e_rel = np.abs(ref["ref32"][:, [0, 2]] - ref["ref64"][:, [0, 2]]) / np.abs(ref["ref64"][:, [0, 2]])
        out[name + ".E_rel"] = e_rel
        print(f"{name:14s} loss {ref['ref64'][0, 0]:.6f} masked {ref['ref64'][0, 2]:.6f} acc {ref['ref64'][0, 1]:.4f} / {ref['ref64'][0, 3]:.4f} "
              f"masked rows {int(mask.sum())} / {mask.numel()} E_rel max {e_rel.max():.3g}")
    for name, (b, n, m, C, tok_seed, seed, mode, min_ratio) in MASK_CASES.items():
        tokens = make_mlm_tokens(b, n, m, C, tok_seed)
        torch.manual_seed(seed)
        val = val_to_mask_of(b, mode, min_ratio)
        torch.manual_seed(seed)
        masked, mask = get_mask_tokens(tokens, C, mode=mode, min_masking_ratio=min_ratio)
        assert bool((masked == torch.where(mask, torch.full_like(tokens, C), tokens)).all())
        out[name + ".params"] = np.array([b, n, m, C, tok_seed, seed], dtype=np.int64)
        out[name + ".mode"] = np.array(mode)
        out[name + ".min_masking_ratio"] = np.float64(min_ratio)
        out[name + ".val_to_mask"] = val.numpy()
        out[name + ".mask"] = np.packbits(mask.numpy().reshape(-1))
        print(f"{name:24s} val_to_mask {val.numpy().round(4)} masked {int(mask.sum())} / {mask.numel()}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "E_rel max over all cases", max(float(out[n + ".E_rel"].max()) for n in LOSS_CASES))


if __name__ == "__main__":
    main()
