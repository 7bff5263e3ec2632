"""Time of one ``TokenizerEvaluator.update`` with LPIPS attached against the same chain in torch fp32 on the same device (profiles/lpips.md).

64 pairs of 256 x 256 (``--pairs``, ``--side``), seeded "grown" VGG16 weights, device events around ``--iters`` calls, three alternating
repetitions (HIP, torch, HIP, torch, ...).  Then one profiled pass (HIP events per launch group) for the split into input / convolutions / pools /
distance, from which the convolution stack's TFLOP/s (real arithmetic, conv1_1 counted with its 3 input channels) and the distance kernel's
bytes/s against its one-read traffic follow.  Prints one JSON line.

    python tools/lpips_bench.py [--pairs 64] [--side 256] [--iters 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskbit_amd import LPIPS, TokenizerEvaluator, _lib  # noqa: E402
from maskbit_amd.synth import VGG16_CONVS, make_eval_images, make_vgg16_weights  # noqa: E402

POOL_BEFORE, TAP_AFTER = (5, 10, 17, 24), (2, 7, 14, 21, 28)


def torch_lpips(real, fake, vgg, lins, shift, scale):
    """lpips.py:39-52 with torch fp32 operators on the device, both images in one batch as the engine runs them"""
    x = (torch.cat([real, fake]).clamp(0.0, 1.0) * 2.0 - 1.0 - shift) / scale
    B = real.shape[0]
    val = 0.0
    k = 0
    for idx, _cin, _cout in VGG16_CONVS:
        if idx in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, vgg[f"{idx}.weight"], vgg[f"{idx}.bias"], padding=1))
        if idx in TAP_AFTER:
            n = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            d = (n[:B] - n[B:]).pow(2)
            val = val + (d * lins[k].view(1, -1, 1, 1)).sum(1, keepdim=True).mean((2, 3), keepdim=True)
            k += 1
    return val


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=16, help="pairs per torch call (fp32 activations of 2 x 16 images of 256^2 take 2 GiB at conv1)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P, S = args.pairs, args.side
    real, fake = (t.to(dev) for t in make_eval_images("noise", 0.05, P, S, S, 1))
    vgg = make_vgg16_weights(4100, "grown")
    g = torch.Generator().manual_seed(2)
    lins = [torch.rand(c, generator=g) for c in (64, 128, 256, 512, 512)]
    m = LPIPS()
    m.load_vgg16(vgg)
    m.load_linear({f"lin{k}.model.1.weight": v.view(1, -1, 1, 1) for k, v in enumerate(lins)})
    m = m.to(dev)
    ev = TokenizerEvaluator(dev)
    ev.use_lpips(m)
    vgg_d = {k: v.to(dev) for k, v in vgg.items()}
    lins_d = [v.to(dev) for v in lins]
    shift, scale = m.scaling_layer.shift.to(dev), m.scaling_layer.scale.to(dev)

    def run_hip():
        ev.update(real, fake, clamp=True)

    def run_torch():
        with torch.no_grad():
            return torch.cat([torch_lpips(real[i:i + args.torch_chunk], fake[i:i + args.torch_chunk], vgg_d, lins_d, shift, scale)
                              for i in range(0, P, args.torch_chunk)])

    run_hip()
    ref = run_torch().reshape(-1).double()
    torch.cuda.synchronize()
    agree = float(((ev.last_lpips - ref).abs() / ref).max())
    hip_ms, torch_ms = [], []
    for _ in range(3):
        hip_ms.append(timed(run_hip, args.iters))
        torch_ms.append(timed(run_torch, args.iters))
    _lib.prof_enable(True)
    run_hip()
    torch.cuda.synchronize()
    prof = {k: v for k, v in _lib.prof_read().items() if k.startswith("lpips")}
    _lib.prof_enable(False)
    flops = 0.0
    bytes_dist = 0.0
    side = S
    for idx, cin, cout in VGG16_CONVS:
        if idx in POOL_BEFORE:
            side //= 2
        flops += 2.0 * side * side * cout * cin * 9
        if idx in TAP_AFTER:
            bytes_dist += 2.0 * side * side * cout * 2
    flops *= 2 * P
    bytes_dist *= P
    conv_ms, dist_ms = prof.get("lpips_conv", (0, 0.0))[1], prof.get("lpips_distance", (0, 0.0))[1]
    out = dict(pairs=P, side=S, hip_ms=hip_ms, torch_fp32_ms=torch_ms, speedup=min(torch_ms) / min(hip_ms), max_rel_diff_vs_torch=agree,
               profile_ms={k: v[1] for k, v in prof.items()}, conv_tflops=flops / (conv_ms * 1e9) if conv_ms else None,
               distance_gbytes_per_s=bytes_dist / (dist_ms * 1e6) if dist_ms else None, distance_mbytes=bytes_dist / 1e6,
               saturated=m.saturation_count())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
