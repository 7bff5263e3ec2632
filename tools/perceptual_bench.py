"""Time of ``PerceptualLoss.per_image`` against the same network as torch fp32 operators on the same device, and the loss's noise floor
(profiles/perceptual.md).

Two shapes a tokenizer evaluation runs: 64 pairs of 256 x 256 and 16 pairs of 512 x 512.  Seeded weights (``make_resnet50_weights``), device events
around ``--iters`` calls after a warm-up of both, three alternating repetitions (HIP, torch, HIP, torch, ...).  Then one profiled pass (HIP events
per launch group, profiler off during the timed windows) for the split into input / stem / pool / the four layers / head / distance, from which the
convolutions' TFLOP/s follow (4.09 GMAC per image at 224 x 224, conv1 counted with its 147 real products).  The torch side is the written-out
network with ``F.interpolate(antialias=True)``, ``F.conv2d``, ``F.batch_norm`` and ``F.mse_loss`` in fp32 -- what a user would run otherwise.

Noise floor: fp16 activation storage against the float64 restatement (tests/resnet_reference.py) for one 256 x 256 pair at three distances
(noise sigma 0.005, 0.02, 0.1), both ``on_logits`` settings.

    python tools/perceptual_bench.py [--iters 10] [--out profiles/perceptual.md]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resnet_reference as R  # noqa: E402
from maskbit_amd import PerceptualLoss, _lib  # noqa: E402
from maskbit_amd.synth import make_eval_images  # noqa: E402

SHAPES = ((64, 256), (16, 512))
GMAC_PER_IMAGE = 4.087136256


def torch_network(x, sd):
    """torchvision's resnet50 forward in fp32 functional form -> (layer4, logits)"""
    def cb(t, conv, bn, stride=1, padding=0):
        t = F.conv2d(t, sd[conv + ".weight"], None, stride, padding)
        return F.batch_norm(t, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, 1e-5)

    x = F.max_pool2d(F.relu(cb(x, "conv1", "bn1", 2, 3)), 3, 2, 1)
    for li, blocks in enumerate(R.BLOCKS):
        for b in range(blocks):
            p, stride = f"layer{li + 1}.{b}", 2 if (b == 0 and li > 0) else 1
            t = F.relu(cb(x, p + ".conv1", p + ".bn1"))
            t = F.relu(cb(t, p + ".conv2", p + ".bn2", stride, 1))
            idn = cb(x, p + ".downsample.0", p + ".downsample.1", stride) if b == 0 else x
            x = F.relu(cb(t, p + ".conv3", p + ".bn3") + idn)
    return x, F.linear(x.mean((2, 3)), sd["fc.weight"], sd["fc.bias"])


def torch_loss(real, fake, sd, mean, std, on_logits=True):
    """perceptual_loss.py:49-63 per pair, both images in one batch"""
    x = torch.cat([real, fake])
    x = (F.interpolate(x, size=224, mode="bilinear", antialias=True, align_corners=False) - mean) / std
    feat, logits = torch_network(x, sd)
    B = real.shape[0]
    v = (logits[:B] - logits[B:]).pow(2).mean(1)
    if not on_logits:
        v = v + (feat[:B] - feat[B:]).pow(2).mean((1, 2, 3))
    return v


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-chunk", type=int, default=16, help="pairs per torch call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    sd = R.weights()
    m = PerceptualLoss()
    m.load_resnet50(sd)
    m = m.to(dev)
    sd_d = {k: v.to(dev) for k, v in sd.items() if v.is_floating_point()}
    mean, std = m.mean.to(dev), m.std.to(dev)
    rows, raw = [], []
    for P, S in SHAPES:
        real, fake = (t.to(dev) for t in make_eval_images("noise", 0.05, P, S, S, 1))

        def run_hip():
            return m.per_image(real, fake)

        def run_torch():
            with torch.no_grad():
                return torch.cat([torch_loss(real[i:i + args.torch_chunk], fake[i:i + args.torch_chunk], sd_d, mean, std)
                                  for i in range(0, P, args.torch_chunk)])

        got, ref = run_hip(), run_torch().double()               # the warm-up of every shape both use
        run_hip(), run_torch()
        torch.cuda.synchronize()
        agree = float(((got - ref).abs() / ref).max())
        hip_ms, torch_ms = [], []
        for _ in range(3):
            hip_ms.append(timed(run_hip, args.iters))
            torch_ms.append(timed(run_torch, args.iters))
        _lib.prof_enable(True)
        run_hip()
        torch.cuda.synchronize()
        prof = {k: v[1] for k, v in _lib.prof_read().items() if k.startswith("resnet")}
        _lib.prof_enable(False)
        conv_ms = sum(v for k, v in prof.items() if k.startswith("resnet_conv") or k == "resnet_stem")
        tflops = 2.0 * GMAC_PER_IMAGE * 2 * P / conv_ms if conv_ms else None
        raw.append(dict(pairs=P, side=S, hip_ms=hip_ms, torch_fp32_ms=torch_ms, max_rel_diff_vs_torch=agree, profile_ms=prof, conv_tflops=tflops,
                        saturated=m.saturation_count()))
        rows.append((P, S, hip_ms, torch_ms, agree, prof, tflops))

    # the noise floor: one 256 x 256 pair at three distances against float64
    floor = []
    base, _ = R.pair_images("256")
    g = torch.Generator().manual_seed(5290)
    noise = torch.randn(base.shape, generator=g)
    models = {True: m, False: None}
    f = PerceptualLoss(compute_perceptual_loss_on_logits=False)
    f.load_resnet50(sd)
    models[False] = f.to(dev)
    for sigma in (0.005, 0.02, 0.1):
        other = (base + sigma * noise).clamp(0.0, 1.0)
        with torch.no_grad():
            exact = R.trunk64(R.input64(torch.cat([base, other])), sd, False)
        for on_logits in (True, False):
            want = float(R.loss64(exact, 1, on_logits))
            got = float(models[on_logits].per_image(base.to(dev), other.to(dev)).cpu())
            floor.append((sigma, on_logits, want, got, abs(got - want), abs(got - want) / want))

    lines = ["# ResNet-50 perceptual loss: times and noise floor", "",
             "Written by `tools/perceptual_bench.py` on one MI355X: seeded weights (`make_resnet50_weights`), device events around "
             f"{args.iters} calls after a warm-up of both sides, three alternating repetitions, the profiler off during the timed windows.  "
             "`torch fp32` is the written-out network as `F.interpolate(antialias=True)` / `F.conv2d` / `F.batch_norm` / `F.linear` on the same device "
             f"({args.torch_chunk} pairs per call).  There is no speed gate: the two times are stated as they came out.", "",
             "| pairs | side | HIP ms (3 repetitions) | torch fp32 ms (3 repetitions) | torch / HIP (best of each) | max rel. difference of a pair's value |",
             "|---|---|---|---|---|---|"]
    for P, S, hip_ms, torch_ms, agree, prof, tflops in rows:
        lines.append(f"| {P} | {S} | {', '.join(f'{v:.2f}' for v in hip_ms)} | {', '.join(f'{v:.2f}' for v in torch_ms)} | "
                     f"{min(torch_ms) / min(hip_ms):.2f} | {agree:.1e} |")
    lines += ["", "Per launch group (`mb_prof_*`, HIP events, one profiled pass of its own; ms per call of the whole batch):", ""]
    keys = sorted({k for r in rows for k in r[5]})
    lines += ["| group | " + " | ".join(f"{P} x {S}^2" for P, S, *_ in rows) + " |", "|---|" + "---|" * len(rows)]
    for k in keys:
        lines.append(f"| `{k}` | " + " | ".join(f"{r[5].get(k, 0.0):.3f}" for r in rows) + " |")
    lines.append("| convolutions, TFLOP/s (4.09 GMAC per image) | " + " | ".join(f"{r[6]:.0f}" if r[6] else "-" for r in rows) + " |")
    lines += ["", "`resnet` is the whole call; `resnet_stem` is the im2col kernel plus conv1 as a 1x1; a `resnet_conv.layerL` scope spans the three or four "
              "convolutions of every bottleneck of that layer.", "",
              "## Noise floor", "",
              "fp16 activation storage (fp32 accumulation, fp16 weights) against the float64 restatement, one 256 x 256 pair: a base image and the base "
              "plus Gaussian noise of the given sigma.", "",
              "| sigma | on_logits | float64 | HIP | abs. difference | relative |", "|---|---|---|---|---|---|"]
    for sigma, on_logits, want, got, d, rel in floor:
        lines.append(f"| {sigma} | {on_logits} | {want:.6e} | {got:.6e} | {d:.2e} | {rel:.1e} |")
    lines += ["", "Weights are seeded, not the ImageNet checkpoint; the network was not compared with torchvision's or with the reference module.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(dict(shapes=raw, noise_floor=[dict(sigma=s, on_logits=o, exact=w, hip=g_, abs=d, rel=r) for s, o, w, g_, d, r in floor])))


if __name__ == "__main__":
    main()
