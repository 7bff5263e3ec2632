"""Timing of ``maskbit_amd.ImageTransform`` (csrc/image.hip), the upload included, against the same transform with Pillow on 16 host threads of the
same machine: 64 synthetic sources of the common ImageNet shape (375 x 500), and a seeded mixed-size batch of 64 (sides 120 .. 900 and four
photographs of 2000 .. 3000 pixels).

    python tools/image_transform_bench.py [--reps 20] [--rounds 3] [--threads 16] [--resolution 256]

One process.  Results are compared first where Pillow is installed (every byte; a faster transform that computes something else is not faster).
The arms are timed in alternating rounds after a warm-up: the device arm by a host clock around the call and a device synchronise (staging copy,
upload, launches and kernels), the Pillow arm by a host clock around a thread pool producing the same float32 tensors.  Per-kernel times come from
the library's HIP-event hooks in a separate pass; the bytes are what the algorithm has to move (the source rows the windows read, the uint8
intermediate written and read once, the outputs).  Prints one JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskbit_amd import ImageTransform, _lib  # noqa: E402
from maskbit_amd.telemetry import ClockSampler  # noqa: E402

try:
    from PIL import Image
except ImportError:                                            # the device arm still runs; the host arm is reported as not measured
    Image = None


def batches(seed=0):
    rng = np.random.default_rng(seed)
    common = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(64)]
    sizes = [(int(rng.integers(120, 900)), int(rng.integers(120, 900))) for _ in range(60)] + [(2000, 3000), (3000, 2000), (2448, 3264), (1536, 2048)]
    mixed = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    return {"imagenet_375x500_x64": common, "mixed_sizes_x64": mixed}


def pillow_one(img, R, recipe, resample):
    pil = Image.fromarray(img)
    if recipe == "adm":
        while min(*pil.size) >= 2 * R:
            pil = pil.resize(tuple(x // 2 for x in pil.size), resample=Image.BOX)
        scale = R / min(*pil.size)
        pil = pil.resize(tuple(round(x * scale) for x in pil.size), resample=Image.BICUBIC)
        arr = np.asarray(pil)
        cy, cx = (arr.shape[0] - R) // 2, (arr.shape[1] - R) // 2
        arr = arr[cy:cy + R, cx:cx + R]
    else:
        w, h = pil.size
        ow, oh = (R, int(R * h / w)) if w <= h else (int(R * w / h), R)
        if (w, h) != (ow, oh):
            pil = pil.resize((ow, oh), resample)
        top, left = int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))
        arr = np.asarray(pil.crop((left, top, left + R, top + R)))
    # ToTensor(): uint8 -> float32, / 255 (the same IEEE division); in numpy, so that 16 worker threads do not each start a torch thread team
    return np.ascontiguousarray((arr.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def algorithm_bytes(transform, images):
    """Source bytes of the rows read, the intermediate once out and once in, the float32 output."""
    R, total = transform.resolution, 0
    for p in transform.plan([im.shape[:2] for im in images]):
        for j in p["jobs"]:
            (sh, sw), (rh, rw), (wy, wx, wh, ww) = j["src_size"], j["res_size"], j["window"]
            rows = min(sh, int(np.ceil(wh * max(sh / rh, 1.0))) + 4)
            total += rows * sw * 3 + 2 * rows * ww * 3 + wh * ww * 3 * (4 if p["final"] else 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--resolution", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_transform_bench needs a GPU: a timing taken anywhere else says nothing")
    R = args.resolution
    arms = [("reference", "bilinear"), ("reference", "bicubic"), ("adm", "bicubic")]
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC} if Image else {}
    pool = ThreadPoolExecutor(args.threads)
    for name, images in batches().items():
        for recipe, interp in arms:
            t = ImageTransform(R, interp, recipe, device="cuda:0")
            out = t(images)
            torch.cuda.synchronize()
            if Image:
                want = torch.from_numpy(np.stack(list(pool.map(lambda im: pillow_one(im, R, recipe, resample[interp]), images))))
                differing = int((out.cpu().view(torch.int32) != want.view(torch.int32)).sum())
                print(json.dumps(dict(what="device vs Pillow", batch=name, recipe=recipe, interpolation=interp, differing_floats=differing)))
                assert differing == 0

            def device_arm():
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    t(images)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / args.reps

            def pillow_arm():
                t0 = time.perf_counter()
                for _ in range(max(1, args.reps // 4)):
                    torch.from_numpy(np.stack(list(pool.map(lambda im: pillow_one(im, R, recipe, resample[interp]), images))))
                return (time.perf_counter() - t0) * 1e3 / max(1, args.reps // 4)

            device_arm()
            dev_ms, pil_ms, clocks = [], [], []
            for _ in range(args.rounds):
                with ClockSampler(0) as cs:
                    dev_ms.append(device_arm())
                clocks.append(cs.summary())
                if Image:
                    pil_ms.append(pillow_arm())
            # per-kernel device times, in a pass of their own
            _lib.prof_enable(True)
            _lib.prof_read()
            for _ in range(args.reps):
                t(images)
            torch.cuda.synchronize()
            prof = _lib.prof_read()
            _lib.prof_enable(False)
            kernels = {k: round(v[1] / args.reps, 4) for k, v in prof.items() if k.startswith("image_")}
            nbytes = algorithm_bytes(t, images)
            kernel_ms = sum(v for k, v in kernels.items() if k != "image_resample")
            mhz = [c["effective_clock_mhz"] for c in clocks if "effective_clock_mhz" in c]
            med = statistics.median(dev_ms)
            print(json.dumps(dict(
                what="timing", batch=name, images=len(images), recipe=recipe, interpolation=interp, resolution=R, reps=args.reps, rounds=args.rounds,
                device_call_ms=round(med, 3), device_call_ms_min_max=[round(min(dev_ms), 3), round(max(dev_ms), 3)], device_ms_per_image=round(med / len(images), 4),
                pillow_threads=args.threads, pillow_ms=(round(statistics.median(pil_ms), 2) if pil_ms else "not measured"),
                pillow_ms_min_max=([round(min(pil_ms), 2), round(max(pil_ms), 2)] if pil_ms else None),
                ratio_pillow_over_device=(round(statistics.median(pil_ms) / med, 2) if pil_ms else None),
                kernel_ms_per_call=kernels, raw_upload_bytes=int(sum(im.size for im in images)), algorithm_bytes=int(nbytes),
                kernels_gb_per_s=(round(nbytes / kernel_ms / 1e6, 1) if kernel_ms > 0 else None),
                shader_clock_mhz=(statistics.median(mhz) if mhz else "not measured"), clock_source=clocks[0].get("source"))))


if __name__ == "__main__":
    main()
