"""Timing of ``maskbit_amd.GeneratorEvaluator.update_features`` against the reference's own update loop written with torch operations on the
same device (evaluator/evaluator.py:553-569: softmax, log, two column sums, and per image ``total += f; sigma += torch.outer(f, f)``), at
B = 64, D = 2048, C = 1008 in float64.  One process; the arms are timed in alternating rounds with HIP events (warm-up, then ``--reps`` updates per
round), and every GPU step runs under a time limit of its own.  Results are compared first: a faster update that computes something else is not
faster.  Reports the median and the minimum over the rounds, the ratio, and the bytes/s of the FID update against what it has to move: the upper
64 x 64 blocks of the D x D float64 state read and written once, plus the features.

    python tools/generator_evaluator_bench.py [--reps 20] [--rounds 5] [--batch 64]

Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskbit_amd import GeneratorEvaluator  # noqa: E402
from maskbit_amd.synth import make_eval_features  # noqa: E402

STEP_LIMIT_S = 120


class TorchLoop:
    """GeneratorEvaluator.update of the reference after the network, operation for operation in torch."""

    def __init__(self, device, D, C):
        self.total = torch.zeros(D, dtype=torch.float64, device=device)
        self.sigma = torch.zeros((D, D), dtype=torch.float64, device=device)
        self.prob_total = torch.zeros(C, dtype=torch.float64, device=device)
        self.kl_total = torch.zeros(C, dtype=torch.float64, device=device)

    def update_is(self, logits):
        p = F.softmax(logits, dim=-1)
        self.prob_total += torch.sum(p, 0, dtype=torch.float64)
        self.kl_total += torch.sum(p * torch.log(p + 1e-16), 0, dtype=torch.float64)

    def update_fid(self, pool):
        for f in pool:
            self.total += f
            self.sigma += torch.outer(f, f)


def limited(fn, what):
    """One GPU step under its own time limit."""
    def on_alarm(signum, frame):
        raise TimeoutError(f"{what}: no result within {STEP_LIMIT_S} s")
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(STEP_LIMIT_S)
    try:
        return fn()
    finally:
        signal.alarm(0)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generator_evaluator_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    B, D, C = args.batch, 2048, 1008
    pool, logits = (t.to(dev) for t in make_eval_features(D, C, B, 0))
    hip = GeneratorEvaluator(dev, enable_fid=True, enable_inception_score=True)
    hip_fid = GeneratorEvaluator(dev, enable_fid=True)
    hip_is = GeneratorEvaluator(dev, enable_inception_score=True)
    ref = TorchLoop(dev, D, C)

    def compare():
        hip.update_features(pool, logits)
        ref.update_fid(pool)
        ref.update_is(logits)
        _, total, sigma = hip.fid_statistics()
        _, prob, kl = hip.is_statistics()
        diff = dict(total=float((total - ref.total).abs().max() / ref.total.abs().max()), sigma=float((sigma - ref.sigma).abs().max() / ref.sigma.abs().max()),
                    prob=float((prob - ref.prob_total).abs().max()), kl=float((kl - ref.kl_total).abs().max() / ref.kl_total.abs().max()))
        hip.reset_metrics()
        return diff
    diff = limited(compare, "comparison")
    print(json.dumps(dict(what="update_features vs torch loop (fp64), largest difference relative to the largest element", **{k: float(f"{v:.3g}") for k, v in diff.items()})))
    assert max(diff.values()) < 1e-12

    arms = {
        "hip_update_features": lambda: hip.update_features(pool, logits),
        "torch_loop": lambda: (ref.update_fid(pool), ref.update_is(logits)),
        "hip_fid_only": lambda: hip_fid.update_features(pool, None),
        "torch_loop_fid_only": lambda: ref.update_fid(pool),
        "hip_is_only": lambda: hip_is.update_features(None, logits),
        "torch_loop_is_only": lambda: ref.update_is(logits),
    }
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):                          # alternating rounds: both see the same clocks and neighbours
        for name, fn in arms.items():
            ms[name].append(limited(lambda: timed(fn, args.reps), name))
    for name, v in ms.items():
        print(json.dumps(dict(what=name, batch=B, D=D, C=C, reps=args.reps, rounds=args.rounds, median_ms=round(statistics.median(v), 4),
                              min_ms=round(min(v), 4), max_ms=round(max(v), 4))))
    med = {k: statistics.median(v) for k, v in ms.items()}
    nb = D // 64
    moved = 2 * (nb * (nb + 1) // 2) * 64 * 64 * 8 + B * D * 8
    print(json.dumps(dict(what="summary", fid_state_and_features_mb=round(moved / 1e6, 1),
                          ratio_update=round(med["torch_loop"] / med["hip_update_features"], 1),
                          ratio_fid=round(med["torch_loop_fid_only"] / med["hip_fid_only"], 1),
                          ratio_is=round(med["torch_loop_is_only"] / med["hip_is_only"], 1),
                          hip_fid_gb_per_s=round(moved / med["hip_fid_only"] / 1e6, 1),
                          note="update time including its launches; bytes/s = the upper blocks of sigma read + written once, plus the features, over that time")))


if __name__ == "__main__":
    main()
