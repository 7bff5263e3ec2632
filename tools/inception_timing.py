"""Time of one ``InceptionV3`` forward on the HIP path against the torch restatement of the same network on the same device, and what fp16
activation storage costs in the metrics' own units (profiles/inception.md).

* 64 images of 256 x 256 (``--images``, ``--side``), seeded "tf" weights: device events around ``--iters`` forwards after a warm-up, three
  repetitions.  The float64 torch restatement (tests/inception_reference.py, the only runnable stand-in for the reference's float64
  ``torch_fidelity`` network) and the same in float32 run in chunks of ``--torch-chunk`` images with the vendor convolution library switched off
  (torch's own im2col + GEMM path: float64 has no other, and float32 is timed on the same path so that the two differ in the arithmetic alone).
* One profiled forward (HIP events per launch, which add their own gaps) for the split by layer group, and the achieved share of the arithmetic
  counted from the layer table.
* FID and Inception Score between the HIP features and the float64 features of the same ``--metric-images`` synthetic images.

The weights are seeded, not the checkpoint: nothing here says how the real network's features behave.  Prints one JSON line.

    python tools/inception_timing.py [--images 64] [--side 256] [--iters 5] [--metric-images 512]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inception_reference as R  # noqa: E402
from maskbit_amd import InceptionV3, _lib, frechet_distance, get_covariance  # noqa: E402
from maskbit_amd.synth import inception_convs, make_eval_images, make_inception_weights  # noqa: E402


def output_side(name: str) -> int:
    """the side of a layer's output map (DESIGN.md "Inception-v3")"""
    stem = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71}
    if name in stem:
        return stem[name]
    if name.startswith("Mixed_5"):
        return 35
    if name.startswith("Mixed_6a"):
        return 17 if name.endswith(("branch3x3", "branch3x3dbl_3")) else 35
    if name.startswith("Mixed_6"):
        return 17
    if name.startswith("Mixed_7a"):
        return 8 if name.endswith(("branch3x3_2", "branch7x7x3_4")) else 17
    return 8


def macs_by_group():
    out = {}
    for name, cin, cout, (kh, kw), _s, _p in inception_convs():
        g = "stem" if name.startswith("Conv2d") else name[:7]
        out[g] = out.get(g, 0) + output_side(name) ** 2 * cout * cin * kh * kw
    out["head"] = 2048 * 1008
    return out


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def score(logits):
    p = torch.softmax(logits.double(), 1)
    return float(torch.exp((p * (torch.log(p + 1e-16) - torch.log(p.mean(0, keepdim=True) + 1e-16))).sum(1).mean()))


def fid(a, b):
    a, b = a.double(), b.double()
    return frechet_distance(a.mean(0), get_covariance(a.T @ a, a.sum(0), a.shape[0]), b.mean(0), get_covariance(b.T @ b, b.sum(0), b.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=16)
    ap.add_argument("--metric-images", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.enabled = False
    N, S = args.images, args.side
    sd = make_inception_weights(R.WEIGHT_SEED, "tf")
    sd_d = {k: v.to(dev) for k, v in sd.items()}
    net = InceptionV3()
    net.load_weights(sd)
    net = net.to(dev)
    net.max_images_per_call = N

    def images(n, seed):
        return (make_eval_images("noise", 0.05, n, S, S, seed)[0] * 255.0).to(torch.uint8).to(dev)

    x = images(N, 1)

    def run_hip():
        return net(x)

    def run_torch(dtype, batch=None):
        batch = x if batch is None else batch
        with torch.no_grad():
            parts = [R.inception64(batch[i:i + args.torch_chunk], sd_d, dtype=dtype) for i in range(0, batch.shape[0], args.torch_chunk)]
        return {k: torch.cat([p[k] for p in parts]) for k in ("2048", "logits_unbiased")}

    for _ in range(3):
        run_hip()
    run_torch(torch.float32)
    ref = run_torch(torch.float64)
    torch.cuda.synchronize()
    got = run_hip()
    agree = {k: float((got[k].double() - ref[k]).abs().max()) for k in ref}
    hip_ms = [timed(run_hip, args.iters) for _ in range(3)]
    f32_ms = [timed(lambda: run_torch(torch.float32), 1) for _ in range(2)]
    f64_ms = [timed(lambda: run_torch(torch.float64), 1) for _ in range(2)]

    _lib.prof_enable(True)
    run_hip()
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in _lib.prof_read().items() if k.startswith("inception")}
    _lib.prof_enable(False)
    macs = macs_by_group()
    total_macs = sum(macs.values())
    groups = {}
    for g in ("stem", "Mixed_5", "Mixed_6", "Mixed_7"):
        ms = prof.get("inception_conv." + g, 0.0)
        groups[g] = dict(conv_ms=ms, pool_ms=prof.get("inception_pool." + g, 0.0), gmac_per_image=macs[g] / 1e9,
                         conv_tflops=2.0 * macs[g] * N / (ms * 1e9) if ms else None)

    M = args.metric_images
    feats_hip, feats_64 = {"2048": [], "logits_unbiased": []}, {"2048": [], "logits_unbiased": []}
    for i in range(0, M, N):
        batch = images(min(N, M - i), 100 + i)
        h, r = net(batch), run_torch(torch.float64, batch)
        for k in feats_hip:
            feats_hip[k].append(h[k].double())
            feats_64[k].append(r[k])
    feats_hip = {k: torch.cat(v) for k, v in feats_hip.items()}
    feats_64 = {k: torch.cat(v) for k, v in feats_64.items()}
    half = M // 2
    out = dict(images=N, side=S, hip_ms=hip_ms, torch_fp32_ms=f32_ms, torch_fp64_ms=f64_ms, speedup_vs_fp64=min(f64_ms) / min(hip_ms),
               speedup_vs_fp32=min(f32_ms) / min(hip_ms), max_abs_diff_vs_fp64=agree, gmac_per_image=total_macs / 1e9,
               tflops_whole_forward=2.0 * total_macs * N / (min(hip_ms) * 1e9), profile_ms=prof, groups=groups,
               metric_images=M, fid_hip_vs_fp64=fid(feats_hip["2048"], feats_64["2048"]),
               fid_fp64_halves=fid(feats_64["2048"][:half], feats_64["2048"][half:]), fid_hip_halves=fid(feats_hip["2048"][:half], feats_hip["2048"][half:]),
               inception_score_hip=score(feats_hip["logits_unbiased"]), inception_score_fp64=score(feats_64["logits_unbiased"]),
               feature_rms=float(feats_64["2048"].pow(2).mean().sqrt()),
               feature_max_abs_diff=float((feats_hip["2048"] - feats_64["2048"]).abs().max()), saturated=net.saturation_count())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
