"""Time of the VQGAN+ discriminator's held-out pass against the same graph as torch fp32 operators on the same device (profiles/discriminator.md).

The shape a tokenizer evaluation runs: 64 images of 256 x 256 at hidden 128, 3 stages, blur 4 -- forward plus the five logit sums, of the real
and of the fake batch (128 images a call).  Seeded weights (``make_discriminator_weights``), device events around ``--iters`` calls after a warm-up
of both, three alternating repetitions (HIP, torch, HIP, torch, ...).  Then one profiled pass (HIP events per launch group, profiler off during
the timed windows) for the split into block_in / stage convolutions / downsample / GroupNorm / head, from which the convolutions' TFLOP/s follow
(40.0 GFLOP per image: block_in counted with its 75 real products).  The torch side is ``F.conv2d`` / ``F.leaky_relu`` / a depthwise blur
``F.conv2d`` / ``F.group_norm`` / ``F.adaptive_max_pool2d`` in fp32 and the five sums in float64 -- what a user would run otherwise.

    python tools/discriminator_bench.py [--iters 5] [--out profiles/discriminator_times.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/discriminator_bench.py --trace-only       # the per-kernel split: three plain passes
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

from maskbit_amd import NLayerDiscriminatorv2, _lib  # noqa: E402
from maskbit_amd.discriminator import blur_kernel, stats_from_logits  # noqa: E402
from maskbit_amd.synth import make_discriminator_weights, make_eval_images  # noqa: E402

IMAGES, SIDE, HIDDEN, STAGES, BLUR = 64, 256, 128, 3, 4
PEAK_TFLOPS = 2500.0                     # fp16 MFMA, dense


def gflop_per_image(side=SIDE, hidden=HIDDEN, stages=STAGES):
    px, total, cin = side * side, 0.0, hidden
    total += 2.0 * px * hidden * 75
    for i in range(stages):
        cout = hidden << i
        total += 2.0 * px * cout * cin * 9
        px, cin = px // 4, cout
    return (total + 2.0 * 256 * cin * cin) / 1e9


def torch_logits(x, sd, stages=STAGES, blur=BLUR):
    k = blur_kernel(blur).to(x.device)
    pad = max((SIDE // 2 - 1) * 2 + blur - SIDE, 0)        # the same at every even size
    x = F.leaky_relu(F.conv2d(x, sd["block_in.0.weight"], sd["block_in.0.bias"], padding=2), 0.1)
    for i in range(stages):
        x = F.conv2d(x, sd[f"blocks.{i}.0.weight"], sd[f"blocks.{i}.0.bias"], padding=1)
        x = F.conv2d(F.pad(x, [pad // 2, pad - pad // 2, pad // 2, pad - pad // 2]), k.expand(x.shape[1], -1, -1, -1), stride=2, groups=x.shape[1])
        x = F.leaky_relu(F.group_norm(x, 32, sd[f"blocks.{i}.2.weight"], sd[f"blocks.{i}.2.bias"], 1e-5), 0.1)
    x = F.adaptive_max_pool2d(x, 16)
    x = F.leaky_relu(F.conv2d(x, sd["to_logits.0.weight"], sd["to_logits.0.bias"]), 0.1)
    return F.conv2d(x, sd["to_logits.2.weight"], sd["to_logits.2.bias"], padding=2)


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=16, help="images per torch call")
    ap.add_argument("--trace-only", action="store_true", help="three plain passes and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discriminator_times.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("discriminator_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    sd = make_discriminator_weights(900, HIDDEN, STAGES, BLUR)
    m = NLayerDiscriminatorv2(hidden_channels=HIDDEN, num_stages=STAGES, blur_resample=True, blur_kernel_size=BLUR)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    sd_d = {k: v.to(dev) for k, v in sd.items()}
    real, fake = (t.to(dev) for t in make_eval_images("noise", 0.05, IMAGES, SIDE, SIDE, 1))

    def run_hip():
        return m.logit_stats(real), m.logit_stats(fake)

    def run_torch():
        with torch.no_grad():
            return tuple(torch.cat([stats_from_logits(torch_logits(t[i:i + args.torch_chunk], sd_d)) for i in range(0, IMAGES, args.torch_chunk)])
                         for t in (real, fake))

    if args.trace_only:
        for _ in range(3):
            run_hip()
        torch.cuda.synchronize()
        return
    got, ref = run_hip(), run_torch()
    run_hip(), run_torch()
    torch.cuda.synchronize()
    agree = max(float((g - r).abs().max()) / 256 for g, r in zip(got, ref))          # per logit
    hip_ms, torch_ms = [], []
    for _ in range(3):
        hip_ms.append(timed(run_hip, args.iters))
        torch_ms.append(timed(run_torch, args.iters))
    _lib.prof_enable(True)
    run_hip()
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in _lib.prof_read().items() if k.startswith("disc")}
    _lib.prof_enable(False)
    conv_ms = prof.get("disc_conv", 0.0)
    stage_gflop = gflop_per_image() - 2.0 * SIDE * SIDE * HIDDEN * 75 / 1e9 - 2.0 * 256 * (HIDDEN << (STAGES - 1)) ** 2 / 1e9
    tflops = stage_gflop * 2 * IMAGES / conv_ms if conv_ms else None
    whole = gflop_per_image() * 2 * IMAGES / min(hip_ms)
    out = dict(images=2 * IMAGES, side=SIDE, hidden=HIDDEN, gflop_per_image=gflop_per_image(), hip_ms=hip_ms, torch_fp32_ms=torch_ms,
               max_mean_logit_diff_vs_torch=agree, profile_ms=prof, stage_conv_tflops=tflops, whole_call_tflops=whole, saturated=m.saturation_count())
    lines = ["# VQGAN+ discriminator: times", "",
             f"Written by `tools/discriminator_bench.py` on one MI355X: {IMAGES} real and {IMAGES} fake images of {SIDE} x {SIDE}, hidden {HIDDEN}, {STAGES} "
             f"stages, blur {BLUR}, seeded weights; `logit_stats` of both batches a call.  Device events around {args.iters} calls after a warm-up of both "
             f"sides, three alternating repetitions, the profiler off during the timed windows.  `torch fp32` is the same graph as torch operators on the "
             f"same device ({args.torch_chunk} images per call).  There is no speed gate: the two times are stated as they came out.", "",
             "| images | HIP ms (3 repetitions) | torch fp32 ms (3 repetitions) | torch / HIP (best of each) | largest difference of an image's mean logit |",
             "|---|---|---|---|---|",
             f"| {2 * IMAGES} | {', '.join(f'{v:.2f}' for v in hip_ms)} | {', '.join(f'{v:.2f}' for v in torch_ms)} | {min(torch_ms) / min(hip_ms):.2f} | {agree:.1e} |",
             "", "Per launch group (`mb_prof_*`, HIP events, one profiled pass of its own; ms per call of both batches):", "",
             "| group | ms | share of `disc` |", "|---|---|---|"]
    for k in sorted(prof):
        lines.append(f"| `{k}` | {prof[k]:.3f} | {100 * prof[k] / prof.get('disc', 1.0):.1f} % |")
    lines += ["", f"{gflop_per_image():.1f} GFLOP per image, {gflop_per_image() * 2 * IMAGES / 1e3:.2f} TFLOP per call.  The three stage convolutions (`disc_conv`, "
              f"{stage_gflop:.1f} GFLOP per image) run at {tflops:.0f} TFLOP/s = {100 * tflops / PEAK_TFLOPS:.1f} % of the {PEAK_TFLOPS / 1000:.1f} PFLOP/s fp16 MFMA "
              f"peak; the whole call, everything included, at {whole:.0f} TFLOP/s = {100 * whole / PEAK_TFLOPS:.1f} %.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
