"""Timing of ``maskbit_amd.TokenizerEvaluator.update`` against the reference's formulation of the same update written with torch operations on
the same device (evaluator/evaluator.py:282-375: what a user of the reference runs today), at B = 64, 3 x 256 x 256 with 64 x 256 codebook
indices.  One process; the two are timed in alternating rounds with HIP events (warm-up, then ``--reps`` updates per round), and every GPU step
runs under a time limit of its own.  Reports the median and the minimum over the rounds, the ratio, and the bytes/s the fused update achieves
against the 100.7 MB of input it has to read once.  Results are compared first: a faster update that computes something else is not faster.

    python tools/eval_tokenizer_bench.py [--reps 20] [--rounds 5] [--batch 64]

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

from maskbit_amd import TokenizerEvaluator  # noqa: E402

STEP_LIMIT_S = 120


class TorchChain:
    """TokenizerEvaluator.update / result of the reference for the six closed-form metrics, operation for operation in torch."""

    def __init__(self, device, K):
        k = torch.linspace(-5.0, 5.0, steps=11)
        g = torch.exp(-0.5 * (k / 1.5).pow(2))
        g = g / g.sum()
        self.window = torch.outer(g, g).to(device).expand(3, 1, -1, -1)
        self.device, self.K = device, K
        self.reset()

    def reset(self):
        self.n = 0
        self.sums = [torch.tensor(0.0, dtype=torch.float64, device=self.device) for _ in range(4)]
        self.seen = set()
        self.freq = torch.zeros(self.K, dtype=torch.float64, device=self.device)

    def update(self, real, fake, indices=None, images=True):
        B = real.shape[0]
        dim = (1, 2, 3)
        self.n += B
        if images:
            self.sums[0] += torch.abs(fake - real.view_as(fake)).mean(dim=dim).sum()
            self.sums[1] += torch.pow(fake - real.view_as(fake), 2).mean(dim=dim).sum()
            mse = torch.pow(fake.double() - real.view_as(fake).double(), 2).mean(dim=dim)
            self.sums[2] += torch.sum(10.0 * torch.log10(1.0 / (mse + 1e-10)))
            x = F.pad(torch.clone(fake), [5, 5, 5, 5], mode="reflect")
            y = F.pad(torch.clone(real), [5, 5, 5, 5], mode="reflect")
            out = F.conv2d(torch.cat([x, y, torch.pow(x, 2), torch.pow(y, 2), x * y]), self.window, groups=3)
            mx, my, xx, yy, xy = (out[i * B:(i + 1) * B] for i in range(5))
            mxx, myy, mxy = mx.pow(2), my.pow(2), mx * my
            sxx, syy, sxy = xx - mxx, yy - myy, xy - mxy
            c1, c2 = 0.01 ** 2, 0.03 ** 2
            idx = ((2 * mxy + c1) * (2 * sxy + c2)) / ((mxx + myy + c1) * (sxx + syy + c2))
            self.sums[3] += torch.mean(idx, dim, dtype=torch.float64).sum()
        if indices is not None:
            self.seen |= set(torch.unique(indices, sorted=False).tolist())
            entries, counts = torch.unique(indices, sorted=False, return_counts=True)
            self.freq.index_add_(0, entries.int(), counts.double())

    def result(self):
        r = {k: s.item() / self.n for k, s in zip(("MAE", "MSE", "PSNR", "SSIM"), self.sums)}
        p = self.freq / self.freq.sum()
        r["CodebookUsage"] = len(self.seen) / self.K
        r["CodebookEntropy"] = float((-torch.log2(p + 1e-8) * p).sum())
        return r


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
        raise SystemExit("eval_tokenizer_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    B, K = args.batch, 4096
    g = torch.Generator(device=dev).manual_seed(0)
    real = torch.rand(B, 3, 256, 256, device=dev, generator=g)
    fake = (real + 0.05 * torch.randn(B, 3, 256, 256, device=dev, generator=g)).clamp(0.0, 1.0)
    idx = torch.randint(0, K, (B, 16, 16), device=dev, generator=g)
    nbytes = 2 * real.numel() * 4
    flags = dict(enable_psnr_score=True, enable_ssim_score=True, enable_mse_error=True, enable_mae_error=True)
    hip_all = TokenizerEvaluator(dev, enable_codebook_usage_measure=True, enable_codebook_entropy_measure=True, num_codebook_entries=K, **flags)
    hip_img = TokenizerEvaluator(dev, **flags)
    ref = TorchChain(dev, K)

    def compare():
        hip_all.update(real, fake, idx)
        ref.update(real, fake, idx)
        a, b = hip_all.result(), ref.result()
        diff = {k: abs(float(a[k]) - b[k]) for k in b}
        hip_all.reset_metrics()
        ref.reset()
        return diff
    diff = limited(compare, "comparison")
    print(json.dumps(dict(what="fused update vs torch chain (fp32), absolute difference of the results", **{k: float(f"{v:.3g}") for k, v in diff.items()})))
    assert diff["MAE"] < 1e-6 and diff["MSE"] < 1e-6 and diff["PSNR"] < 1e-3 and diff["SSIM"] < 1e-5 and diff["CodebookUsage"] == 0

    arms = {
        "hip_update_all_six": lambda: hip_all.update(real, fake, idx),
        "torch_chain_all_six": lambda: ref.update(real, fake, idx),
        "hip_update_images": lambda: hip_img.update(real, fake),
        "torch_chain_images": lambda: ref.update(real, fake),
        "torch_chain_codebook": lambda: ref.update(real, fake, idx, images=False),
    }
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):                          # alternating rounds: both see the same clocks and neighbours
        for name, fn in arms.items():
            ms[name].append(limited(lambda: timed(fn, args.reps), name))
    for name, v in ms.items():
        print(json.dumps(dict(what=name, batch=B, shape=[3, 256, 256], reps=args.reps, rounds=args.rounds, median_ms=round(statistics.median(v), 4),
                              min_ms=round(min(v), 4), max_ms=round(max(v), 4))))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(what="summary", input_mb=round(nbytes / 1e6, 1),
                          ratio_all_six=round(med["torch_chain_all_six"] / med["hip_update_all_six"], 2),
                          ratio_images=round(med["torch_chain_images"] / med["hip_update_images"], 2),
                          hip_images_gb_per_s=round(nbytes / med["hip_update_images"] / 1e6, 1),
                          note="update() time including its launches; bytes/s = input bytes over that time")))


if __name__ == "__main__":
    main()
