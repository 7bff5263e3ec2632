"""Timing of the precision / recall kernels (csrc/manifold.hip through ``maskbit_amd.manifold``) against the same quantities by chunked
``torch.matmul`` in float64 plus ``topk`` / a comparison on the same GPU -- the way the numpy blocks of ADM's evaluator (``manifold_radii``,
``evaluate_pr``) would port -- at the sizes of an ImageNet evaluation: D = 2048, a reference batch of 10 000 rows, 50 000 samples, fp32 features.

    python tools/manifold_bench.py [--reps 3] [--rounds 3] [--ref 10000] [--samples 50000] [--chunk 4096]

One process; results are compared first (a faster kernel that computes something else is not faster); the arms are timed in alternating rounds
with HIP events after a warm-up, every GPU step under a time limit of its own, the shader clock sampled while the HIP arms run.  Achieved
FLOP/s = 2 N_rows N_cols D, the multiply-adds of the Gram matrix alone, over the call's time (its two or three launches included).  Prints one
JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskbit_amd import knn_radii, manifold_coverage, precision_recall  # noqa: E402
from maskbit_amd.telemetry import ClockSampler  # noqa: E402

STEP_LIMIT_S = 180
D = 2048
K = 3


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
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_radii(x64, norms, k, chunk):
    out = torch.empty(x64.shape[0], dtype=torch.float64, device=x64.device)
    for i0 in range(0, x64.shape[0], chunk):
        d2 = (norms[i0:i0 + chunk, None] + norms[None, :]).addmm_(x64[i0:i0 + chunk], x64.T, alpha=-2.0).clamp_min_(0.0)
        rows = torch.arange(i0, min(i0 + chunk, x64.shape[0]), device=x64.device)
        d2[rows - i0, rows] = 0.0
        out[i0:i0 + chunk] = torch.topk(d2, k + 1, dim=1, largest=False).values[:, k]
    return out


def torch_cover(q64, q_norms, b64, b_norms, radii2, chunk):
    out = torch.empty(q64.shape[0], dtype=torch.bool, device=q64.device)
    for i0 in range(0, q64.shape[0], chunk):
        d2 = (q_norms[i0:i0 + chunk, None] + b_norms[None, :]).addmm_(q64[i0:i0 + chunk], b64.T, alpha=-2.0).clamp_min_(0.0)
        out[i0:i0 + chunk] = (d2 <= radii2[None, :]).any(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref", type=int, default=10000)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--chunk", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("manifold_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    # pooled ReLU-like features: non-negative, the samples scaled and shifted against the reference
    ref = torch.relu(torch.randn(args.ref, D, generator=g, device=dev) + 0.5)
    smp = torch.relu(torch.randn(args.samples, D, generator=g, device=dev) * 0.95 + 0.55)
    ref64, smp64 = ref.double(), smp.double()
    ref_n, smp_n = (ref64 * ref64).sum(1), (smp64 * smp64).sum(1)

    def compare():
        r_hip, r_torch = knn_radii(ref, K), torch_radii(ref64, ref_n, K, args.chunk)
        s_hip, s_torch = knn_radii(smp, K), torch_radii(smp64, smp_n, K, args.chunk)
        in_hip, in_torch = manifold_coverage(smp, ref, r_hip), torch_cover(smp64, smp_n, ref64, ref_n, r_hip, args.chunk)
        p, r = precision_recall(ref, smp, K)
        return dict(radii_ref_rel=float(((r_hip - r_torch).abs() / r_torch).max()), radii_samples_rel=float(((s_hip - s_torch).abs() / s_torch).max()),
                    cover_flags_differing=int((in_hip != in_torch).sum()), precision=p, recall=r)
    diff = limited(compare, "comparison")
    print(json.dumps(dict(what="hip vs torch float64 chain", **diff)))
    assert diff["radii_ref_rel"] < 1e-10 and diff["radii_samples_rel"] < 1e-10

    hip_arms = {
        "hip_knn_radii_ref": (lambda: knn_radii(ref, K), 2.0 * args.ref * args.ref * D),
        "hip_knn_radii_samples": (lambda: knn_radii(smp, K), 2.0 * args.samples * args.samples * D),
        "hip_cover_samples_in_ref": (lambda: manifold_coverage(smp, ref, radii_ref), 2.0 * args.samples * args.ref * D),
        "hip_precision_recall": (lambda: precision_recall(ref, smp, K), 2.0 * (args.ref ** 2 + args.samples ** 2 + 2 * args.ref * args.samples) * D),
    }
    torch_arms = {
        "torch_knn_radii_ref": (lambda: torch_radii(ref64, ref_n, K, args.chunk), 2.0 * args.ref * args.ref * D),
        "torch_knn_radii_samples": (lambda: torch_radii(smp64, smp_n, K, args.chunk), 2.0 * args.samples * args.samples * D),
        "torch_cover_samples_in_ref": (lambda: torch_cover(smp64, smp_n, ref64, ref_n, radii_ref, args.chunk), 2.0 * args.samples * args.ref * D),
    }
    radii_ref = knn_radii(ref, K)
    ms = {k: [] for k in list(hip_arms) + list(torch_arms)}
    clocks = []
    for _ in range(args.rounds):                          # alternating rounds: both see the same clocks and neighbours
        with ClockSampler(0) as cs:
            for name, (fn, _) in hip_arms.items():
                ms[name].append(limited(lambda: timed(fn, args.reps), name))
        clocks.append(cs.summary())
        for name, (fn, _) in torch_arms.items():
            ms[name].append(limited(lambda: timed(fn, args.reps), name))
    flop = {k: v[1] for k, v in {**hip_arms, **torch_arms}.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name, v in ms.items():
        print(json.dumps(dict(what=name, ref=args.ref, samples=args.samples, D=D, k=K, reps=args.reps, rounds=args.rounds, median_ms=round(med[name], 2),
                              min_ms=round(min(v), 2), max_ms=round(max(v), 2), fp64_tflops=round(flop[name] / med[name] / 1e9, 2))))
    mhz = [c["effective_clock_mhz"] for c in clocks if "effective_clock_mhz" in c]
    print(json.dumps(dict(what="summary", shader_clock_mhz_during_hip_arms=(statistics.median(mhz) if mhz else "not measured"),
                          clock_source=clocks[0].get("source"),
                          ratio_knn_ref=round(med["torch_knn_radii_ref"] / med["hip_knn_radii_ref"], 2),
                          ratio_knn_samples=round(med["torch_knn_radii_samples"] / med["hip_knn_radii_samples"], 2),
                          ratio_cover=round(med["torch_cover_samples_in_ref"] / med["hip_cover_samples_in_ref"], 2),
                          note="call time including its launches; FLOP = 2 rows cols D of the Gram matrix only")))


if __name__ == "__main__":
    main()
