"""Times ``MaskedTokenEvaluator.update`` (mb_mlm_loss: one kernel over the logits + a one-workgroup finalize) against the same four figures as
a torch chain on the same device -- ``CrossEntropyLoss(label_smoothing)`` on all rows and on ``inputs[masks]`` plus the two argmax means, what the
reference's MLMLoss runs -- with device events, at the logit shapes of BASELINE configs[2] (64 x 256 x 2 x 64) and of the 14-bit model
(64 x 256 x 2 x 128).  Reports the achieved bytes/s of the update against its one-read traffic: the logits + 9 bytes per row (target, mask).

    python tools/mlm_bench.py [--iters 200] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskbit_amd import MaskedTokenEvaluator  # noqa: E402
from maskbit_amd.synth import make_mlm_case  # noqa: E402

SHAPES = {"configs[2] 12-bit": (64, 256, 2, 64), "14-bit": (64, 256, 2, 128)}


def timed(fn, iters: int, warmup: int = 20) -> float:
    """Mean milliseconds per call between two device events (the work of `iters` calls enqueued back to back)."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_chain(logits, targets, masks, criterion, m):
    C = logits.shape[-1]
    loss = criterion(logits.reshape(-1, C), targets.view(-1))
    correct = (torch.argmax(logits, dim=-1) == targets).float().mean() ** m
    masked_input = logits[masks, :]
    masked_loss = criterion(masked_input, targets[masks])
    masked_correct = (torch.argmax(masked_input, dim=-1) == targets[masks]).float().mean() ** m
    return loss, correct, masked_loss, masked_correct


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlm_bench needs a GPU: timings are taken with device events")
    rows = []
    for name, (b, n, m, C) in SHAPES.items():
        logits, targets = make_mlm_case(b, n, m, C, 7)
        masks = torch.rand(b, n, m, generator=torch.Generator().manual_seed(8)) < 0.55
        logits, targets, masks = logits.cuda(), targets.cuda(), masks.cuda()
        ev = MaskedTokenEvaluator()
        criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
        ev.update(logits, targets, masks)
        ours = ev.result()
        ref = torch_chain(logits, targets, masks, criterion, m)
        agree = max(abs(float(ours[k]) - float(v)) / abs(float(v)) for k, v in zip(("mlm_loss", "correct_tokens", "masked_token_loss", "masked_correct_tokens"), ref))
        pairs = []
        for _ in range(3):                                    # alternate the two, so that a drifting clock shows in both
            pairs.append((timed(lambda: ev.update(logits, targets, masks), args.iters),
                          timed(lambda: torch_chain(logits, targets, masks, criterion, m), max(10, args.iters // 4))))
        hip_ms, torch_ms = min(p[0] for p in pairs), min(p[1] for p in pairs)
        traffic = b * n * m * (4 * C + 9)
        row = dict(shape=name, b=b, n=n, m=m, C=C, update_ms=hip_ms, torch_chain_ms=torch_ms, speedup=torch_ms / hip_ms, one_read_bytes=traffic,
                   update_bytes_per_s=traffic / (hip_ms * 1e-3), all_update_ms=[p[0] for p in pairs], all_torch_ms=[p[1] for p in pairs],
                   max_rel_diff_to_torch_fp32=agree)
        rows.append(row)
        print(f"{name:18s} {b} x {n} x {m} x {C}: update {hip_ms * 1e3:8.1f} us ({traffic / (hip_ms * 1e-3) / 1e9:7.1f} GB/s of {traffic / 1e6:.2f} MB), "
              f"torch chain {torch_ms * 1e3:8.1f} us, x{torch_ms / hip_ms:.1f}; figures agree to {agree:.1e}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
