"""Times of the fp32 reference mode (precision 5; profiles/f32_reference.md), on the GPU box from the repo root:

    python tools/f32_reference_bench.py [forward] [check] [tool]

  forward  the precision-5 plain forward of the full-size 12-bit generator at 8 and 128 sequences: median of 5 after a warm-up, the shader clock sampled
           during the timed forwards, and the resulting TF/s of the GEMMs + attention against the 155 TF f32-MFMA peak.
  check    the wall time of a default check_checkpoint (8 samples, 64 steps, guided) on the same weights, and its report.
  tool     tools/check_checkpoint.py on a synthetic .bin written from synth.make_generator_weights (in a child process)."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maskbit_amd import LFQBert, check_checkpoint, synth                       # noqa: E402
from maskbit_amd.bert import PREC_F32                                          # noqa: E402
from maskbit_amd.telemetry import ClockSampler                                 # noqa: E402

dev = torch.device("cuda")


def generator():
    gen = LFQBert(img_size=256, hidden_dim=1024, codebook_size=4096, codebook_splits=2, depth=24, heads=16, mlp_dim=4096, dropout=0.1, nclass=1000,
                  input_stride=16)
    gen.load_state_dict(synth.make_generator_weights(synth.GenCfg(bits=12, splits=2), seed=100, head_gain=12.0), strict=True)
    return gen.eval().requires_grad_(False).to(dev)


def forward_flops(nb, N=257, d=1024, f=4096, depth=24, out=128):
    """GEMMs (QKV, out-proj, FFN-up, FFN-down per layer; the two head GEMMs) and attention (Q K^T and P V), 2 FLOP per multiply-add."""
    M = nb * N
    gemm = depth * 2 * M * (3 * d * d + d * d + 2 * d * f) + 2 * M * d * d + 2 * M * d * out
    attn = depth * 4 * nb * N * N * d
    return gemm + attn


def forward():
    gen = generator()
    gen.precision = PREC_F32
    g = torch.Generator().manual_seed(1)
    for nb in (8, 128):
        tok = torch.randint(0, 65, (nb, 256, 2), generator=g).to(dev)
        y = torch.randint(0, 1000, (nb,), generator=g).to(dev)
        gen(tok, y)
        torch.cuda.synchronize()
        ts = []
        with ClockSampler(0, period_s=0.02) as cs:
            for _ in range(5):
                t0 = time.perf_counter()
                gen(tok, y)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        print(f"precision 5 forward, {nb:3d} sequences: median {t * 1e3:8.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) = "
              f"{forward_flops(nb) / t / 1e12:6.1f} TF/s of 155; clocks {cs.summary()}", flush=True)


def check():
    gen = generator()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = check_checkpoint(gen)
    torch.cuda.synchronize()
    print(f"default check_checkpoint: {time.perf_counter() - t0:.1f} s wall")
    print(rep, flush=True)


def tool():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "generator.bin")
        torch.save(synth.make_generator_weights(synth.GenCfg(bits=12, splits=2), seed=100, head_gain=12.0), path)
        t0 = time.perf_counter()
        rc = subprocess.call([sys.executable, os.path.join(ROOT, "tools", "check_checkpoint.py"), path, "--bits", "12", "--splits", "2", "--samples", "4",
                              "--steps", "16"])
        print(f"tools/check_checkpoint.py: exit status {rc}, {time.perf_counter() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    modes = sys.argv[1:] or ["forward", "check", "tool"]
    for m in modes:
        {"forward": forward, "check": check, "tool": tool}[m]()
