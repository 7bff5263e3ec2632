"""Checkpoint self-check from the command line (maskbit_amd.check_checkpoint): which precision mode holds the token-mismatch bound on THIS generator file.

    python tools/check_checkpoint.py <generator.bin> --bits 12 --splits 2 [--prenorm] [--seq 256] [--hidden 1024 --depth 24 --heads 16 --mlp 4096]
                                     [--steps 64 --guidance-scale 7.1 --guidance-annealing cosine --scale-pow 3.0 --randomize-temperature 8.2
                                      --mask-schedule arccos] [--samples 8] [--seed 0] [--precisions 2,3,4] [--bound 1e-3]

The file is loaded as the reference's checkpoints are (``load_pretrained(rename_keys={"token_emb": "input_proj"})``).  A run is recorded in the engine's
fp32 reference mode (precision 5), every precision is teacher-forced against it, and the report is printed.  Exit status 1 when the precision the auto
rule resolves to does not hold the bound (upper 95 % limit of its mismatch rate above --bound)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maskbit_amd import LFQBert, check_checkpoint                              # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("--bits", type=int, required=True)
    ap.add_argument("--splits", type=int, required=True)
    ap.add_argument("--prenorm", action="store_true")
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--mlp", type=int, default=4096)
    ap.add_argument("--nclass", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--guidance-scale", type=float, default=7.1)
    ap.add_argument("--guidance-annealing", default="cosine")
    ap.add_argument("--scale-pow", type=float, default=3.0)
    ap.add_argument("--randomize-temperature", type=float, default=8.2)
    ap.add_argument("--mask-schedule", default="arccos")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precisions", default=None, help="comma-separated; default: the auto-resolved one plus 2, 3, 4 where the shape serves them")
    ap.add_argument("--bound", type=float, default=1e-3)
    a = ap.parse_args(argv)
    side = int(round(a.seq ** 0.5))
    if side * side != a.seq:
        ap.error(f"--seq {a.seq} is not a square token grid")
    gen = LFQBert(img_size=16 * side, hidden_dim=a.hidden, codebook_size=2 ** a.bits, codebook_splits=a.splits, depth=a.depth, heads=a.heads,
                  mlp_dim=a.mlp, dropout=0.1, nclass=a.nclass, input_stride=16, use_prenorm=a.prenorm)
    gen.load_pretrained(a.checkpoint, rename_keys={"token_emb": "input_proj"})
    gen = gen.eval().requires_grad_(False).to("cuda")
    precisions = [int(p) for p in a.precisions.split(",")] if a.precisions else None
    report = check_checkpoint(gen, num_samples=a.samples, seed=a.seed, precisions=precisions, bound=a.bound, num_steps=a.steps,
                              guidance_scale=a.guidance_scale, guidance_annealing=a.guidance_annealing, scale_pow=a.scale_pow,
                              randomize_temperature=a.randomize_temperature, mask_schedule_strategy=a.mask_schedule)
    print(report)
    return 0 if report.default_ok else 1


if __name__ == "__main__":
    sys.exit(main())
