"""The data loader's image transform on the device, bit for bit what Pillow computes (``csrc/image.hip``).

``recipe="reference"`` is the reference's ``eval_transform`` (data/webdataset_reader.py:79-85): torchvision ``Resize(resolution, interpolation)``
-> ``CenterCrop(resolution)`` -> ``ToTensor()`` on a PIL image, bilinear for the tokenizer configs and bicubic for the generator configs.
``recipe="adm"`` is guided-diffusion's ``center_crop_arr``, which made the ADM reference batches: BOX halvings while the short side is at least
``2 R``, one BICUBIC resize of the short side to ``R``, a centre crop.  Both are host arithmetic on sizes (``plan``) around passes of one
device entry (``mb_image_resample``: Pillow's fixed-point antialiased resize, horizontal pass first through a uint8 intermediate).  Decoding
(JPEG, PNG) stays on the host: the inputs are decoded uint8 ``[H, W, 3]`` arrays of any size.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2}
MAX_SIDE = 16384
MAX_IMAGES = 4096


def _reference_sizes(H: int, W: int, R: int):
    """torchvision Resize(R) (the short side becomes R, the long one int(R * long / short)) and CenterCrop(R) (origin by Python's round)."""
    if W <= H:
        res_h, res_w = int(R * H / W), R
    else:
        res_h, res_w = R, int(R * W / H)
    return (res_h, res_w), (int(round((res_h - R) / 2.0)), int(round((res_w - R) / 2.0)))


def _adm_sizes(H: int, W: int, R: int):
    """guided-diffusion center_crop_arr: the BOX halvings, the BICUBIC size, the crop origin."""
    halvings = []
    while min(H, W) >= 2 * R:
        H, W = H // 2, W // 2
        halvings.append((H, W))
    scale = R / min(H, W)
    res_h, res_w = round(H * scale), round(W * scale)
    return halvings, (res_h, res_w), ((res_h - R) // 2, (res_w - R) // 2)


class ImageTransform:
    """``ImageTransform(resolution, interpolation, recipe)(images)`` -> float32 ``[B, 3, R, R]`` on the device, exactly
    ``torch.stack([eval_transform(PIL image) ...])``; ``.uint8(images)`` -> uint8 NHWC ``[B, R, R, 3]`` (``to_evaluator_uint8`` of it is what
    ``GeneratorEvaluator.update_uint8`` and the Inception network take).  ``images``: a sequence of uint8 ``[H, W, 3]`` numpy arrays or CPU tensors
    of differing sizes.  The raw bytes and a 72-byte record per image and pass go up in one asynchronous copy from a reusable pinned buffer;
    everything else runs on the current stream without host synchronisation (the one wait is for the upload of the call before the previous
    one, whose pinned buffer is reused)."""

    def __init__(self, resolution: int = 256, interpolation: str = "bilinear", recipe: str = "reference", device=None):
        if recipe not in ("reference", "adm"):
            raise ValueError(f"recipe is 'reference' or 'adm', got {recipe!r}")
        if not isinstance(interpolation, str) or interpolation not in ("bilinear", "bicubic"):
            raise ValueError(f"interpolation {interpolation!r} is not taken: 'bilinear' or 'bicubic' (the shipped configs; Pillow's 'nearest' "
                             "takes another code path and 'lanczos' is not built)")
        if int(resolution) < 1 or int(resolution) > MAX_SIDE:
            raise ValueError(f"resolution must lie in [1, {MAX_SIDE}], got {resolution}")
        self.resolution = int(resolution)
        self.recipe = recipe
        self.interpolation = "bicubic" if recipe == "adm" else interpolation          # "adm" fixes its own filters
        self.device = torch.device(device) if device is not None else None
        self._pinned = [None, None]        # two staging buffers in turn, each with the event of its last upload
        self._uploaded = [None, None]
        self._turn = 0
        self._dev = None                   # device bytes: records, sources, halved images
        self._work = None                  # the passes' workspace

    # ---- host arithmetic on sizes ------------------------------------------------------------------------------------------------------
    def plan(self, sizes: Iterable[Tuple[int, int]]) -> List[Dict]:
        """[(H, W), ...] -> the list of passes.  A pass = {"filter": name, "final": bool, "jobs": [{"image": index, "src_size": (h, w),
        "res_size": (h, w), "window": (y, x, h, w)}, ...]}; a non-final pass ("adm" halvings) writes whole uint8 images that a later pass reads,
        the final pass writes the R x R crops.  Images that need fewer halvings are absent from the later halving passes.  Host only."""
        R = self.resolution
        sizes = [(int(h), int(w)) for h, w in sizes]
        for h, w in sizes:
            if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                raise ValueError(f"image sides must lie in [1, {MAX_SIDE}], got {(h, w)}")
        passes: List[Dict] = []
        final = {"filter": self.interpolation, "final": True, "jobs": []}
        for i, (H, W) in enumerate(sizes):
            if self.recipe == "reference":
                res, (top, left) = _reference_sizes(H, W, R)
                src = (H, W)
            else:
                halvings, res, (top, left) = _adm_sizes(H, W, R)
                src = (H, W)
                for level, (h, w) in enumerate(halvings):
                    while len(passes) <= level:
                        passes.append({"filter": "box", "final": False, "jobs": []})
                    passes[level]["jobs"].append({"image": i, "src_size": src, "res_size": (h, w), "window": (0, 0, h, w)})
                    src = (h, w)
            if max(res) > MAX_SIDE:
                raise ValueError(f"image {i} of size {(H, W)} would be resized to {res}: beyond {MAX_SIDE}")
            final["jobs"].append({"image": i, "src_size": src, "res_size": res, "window": (top, left, R, R)})
        return passes + [final]

    # ---- device ------------------------------------------------------------------------------------------------------------------------
    def __call__(self, images: Sequence) -> torch.Tensor:
        return self._run(images, want_u8=False, want_f32=True)[1]

    def uint8(self, images: Sequence) -> torch.Tensor:
        return self._run(images, want_u8=True, want_f32=False)[0]

    @staticmethod
    def _as_arrays(images) -> List[np.ndarray]:
        if isinstance(images, (np.ndarray, torch.Tensor)) or not hasattr(images, "__len__") or len(images) == 0:
            raise ValueError("images must be a non-empty sequence of uint8 [H, W, 3] arrays (one per image: sizes differ)")
        if len(images) > MAX_IMAGES:
            raise ValueError(f"at most {MAX_IMAGES} images per call, got {len(images)}")
        out = []
        for i, im in enumerate(images):
            if isinstance(im, torch.Tensor):
                if im.device.type != "cpu":
                    raise ValueError(f"image {i} is a tensor on {im.device}: raw images are CPU tensors or numpy arrays")
                im = im.detach().numpy()
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                what = (im.dtype, im.shape) if isinstance(im, np.ndarray) else type(im).__name__
                raise ValueError(f"image {i} must be a uint8 [H, W, 3] array (RGB), got {what}")
            if max(im.shape[:2]) > MAX_SIDE:
                raise ValueError(f"image sides must lie in [1, {MAX_SIDE}], got {im.shape[:2]}")
            out.append(im)
        return out

    def _run(self, images, want_u8: bool, want_f32: bool):
        arrays = self._as_arrays(images)
        passes = self.plan([a.shape[:2] for a in arrays])
        dev = self.device if self.device is not None else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        if dev.type != "cuda":
            raise RuntimeError(f"ImageTransform: the image kernels run only on an AMD GPU through libmaskbit_hip.so (device is {dev}); "
                               "maskbit_amd has no CPU path.")
        lib = _lib.load()
        B, R = len(arrays), self.resolution
        rec = C.sizeof(_lib.ImageJob)
        # layout of the device bytes: [records of every pass | sources, as given | the halved images of every non-final pass]
        table_at, at = [], 0
        for p in passes:
            table_at.append(at)
            at += rec * len(p["jobs"])
        at = sources_at = (at + 15) // 16 * 16
        where = {}                                             # image -> (byte offset, row stride) of its current source
        for i, a in enumerate(arrays):
            where[i] = (at, 3 * a.shape[1])
            at += a.shape[0] * a.shape[1] * 3
        upload = at
        at = (at + 15) // 16 * 16
        tables, work_need, region = [], 0, []
        for p in passes:
            jobs = (_lib.ImageJob * len(p["jobs"]))()
            start, pixels = at, 0
            for j, job in zip(jobs, p["jobs"]):
                i = job["image"]
                j.src_offset, j.src_stride = where[i]
                (j.src_h, j.src_w), (j.res_h, j.res_w) = job["src_size"], job["res_size"]
                j.win_y, j.win_x, j.win_h, j.win_w = job["window"]
                if p["final"]:
                    j.dst_offset = i * R * R
                else:
                    j.dst_offset = pixels
                    where[i] = (start + 3 * pixels, 3 * j.res_w)
                    pixels += j.res_h * j.res_w
            need = int(lib.mb_image_workspace_bytes(jobs, len(jobs), FILTERS[p["filter"]]))
            if need == 0:
                raise ValueError("the image kernels do not take these sizes")
            work_need = max(work_need, need)
            tables.append(jobs)
            region.append((start, pixels))
            at = (start + 3 * pixels + 15) // 16 * 16
        total = at
        with torch.cuda.device(dev):
            turn = self._turn
            self._turn ^= 1
            if self._uploaded[turn] is not None:
                self._uploaded[turn].synchronize()             # the copy out of this pinned buffer two calls ago: long done
            if self._pinned[turn] is None or self._pinned[turn].numel() < upload:
                self._pinned[turn] = torch.empty(max(upload, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
            host = self._pinned[turn].numpy()
            for off, jobs in zip(table_at, tables):
                host[off:off + C.sizeof(jobs)] = np.frombuffer(jobs, dtype=np.uint8)
            off = sources_at
            for a in arrays:
                n = a.shape[0] * a.shape[1] * 3
                host[off:off + n].reshape(a.shape)[...] = a
                off += n
            if self._dev is None or self._dev.numel() < total or self._dev.device != dev:
                self._dev = torch.empty(total * 5 // 4 + 64, dtype=torch.uint8, device=dev)
            if self._work is None or self._work.numel() < work_need or self._work.device != dev:
                self._work = torch.empty(work_need * 5 // 4 + 64, dtype=torch.uint8, device=dev)
            self._dev[:upload].copy_(self._pinned[turn][:upload], non_blocking=True)
            self._uploaded[turn] = torch.cuda.Event()
            self._uploaded[turn].record()
            out_u8 = torch.empty((B, R, R, 3), dtype=torch.uint8, device=dev) if want_u8 else None
            out_f32 = torch.empty((B, 3, R, R), dtype=torch.float32, device=dev) if want_f32 else None
            stream = torch.cuda.current_stream().cuda_stream
            base = self._dev.data_ptr()
            for p, jobs, off, (start, pixels) in zip(passes, tables, table_at, region):
                if p["final"]:
                    u8_ptr, f32_ptr, cap = (out_u8.data_ptr() if want_u8 else None), (out_f32.data_ptr() if want_f32 else None), B * R * R
                else:
                    u8_ptr, f32_ptr, cap = base + start, None, pixels
                _lib.check(lib.mb_image_resample(jobs, base + off, len(jobs), FILTERS[p["filter"]], base, self._dev.numel(), u8_ptr, f32_ptr, cap,
                                                 self._work.data_ptr(), self._work.numel(), stream), "mb_image_resample")
        return out_u8, out_f32


def transformed(loader, transform: ImageTransform, key: str = "image"):
    """A generator over ``loader`` whose batches (dicts) carry a list of raw uint8 ``[H, W, 3]`` arrays under ``key``: yields the same dicts with
    ``transform(batch[key])`` (float32 ``[B, 3, R, R]`` on the device) in its place, so that ``eval_reconstruction`` and ``eval_masked_prediction``
    take a raw-image loader as they are."""
    for batch in loader:
        out = dict(batch)
        out[key] = transform(batch[key])
        yield out
