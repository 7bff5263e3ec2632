"""Improved precision / recall (Kynkaanniemi et al., 2019) as ADM's evaluator computes it -- ``manifold_radii``, ``evaluate_pr`` and
``compute_prec_recall`` on pool features with k = 3 -- behind the gfx950 kernels of ``csrc/manifold.hip``.

A set's manifold is the union of the balls around its rows whose radius is the distance to the row's k-th nearest neighbour.  ``precision`` is the
share of sample rows inside the reference manifold, ``recall`` the share of reference rows inside the sample manifold.  All pairwise squared
distances are formed in float64 on the matrix cores and reduced per row on the fly (include/maskbit_hip.h states the definition); nothing of size
N x N is ever stored.  The calls enqueue on the current stream; only ``precision_recall`` reads a result back.  There is no CPU path.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib

MAX_K = 8


def _device_rows(x, what: str):
    """[N, D] on the device -> (fp32 or fp64 tensor with unit column stride, dtype code, row stride in elements); a row stride above D is kept"""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point() or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} must be a non-empty floating-point [N, D] tensor, got "
                         f"{(x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.device.type != "cuda":
        raise RuntimeError(f"{what}: the manifold kernels run only on an AMD GPU through libmaskbit_hip.so (tensor is on {x.device}); "
                           "maskbit_amd has no CPU path.")
    x = x.detach()
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    N, D = x.shape
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x, (1 if x.dtype == torch.float64 else 0), (x.stride(0) if N > 1 else D)


def _workspace(lib, rows: int, D: int, device) -> torch.Tensor:
    need = int(lib.mb_manifold_workspace_bytes(rows, D))
    if need == 0:
        raise ValueError(f"{rows} rows of width {D} are outside what the manifold kernels take")
    return torch.empty(need // 8, dtype=torch.float64, device=device)


def knn_radii(features: torch.Tensor, k: int = 3) -> torch.Tensor:
    """features [N, D] (fp32 or fp64, device, rows of any stride) -> float64 [N]: the SQUARED distance of every row to its k-th nearest
    neighbour other than itself (duplicates count: a row with k copies has radius 0).  1 <= k <= 8, k + 1 <= N."""
    x, code, stride = _device_rows(features, "features")
    N, D = (int(v) for v in x.shape)
    k = int(k)
    if k < 1 or k > MAX_K or k + 1 > N:
        raise ValueError(f"knn_radii: 1 <= k <= {MAX_K} and k + 1 <= N are required, got k = {k}, N = {N}")
    lib = _lib.load()
    with torch.cuda.device(x.device):
        radii2 = torch.empty(N, dtype=torch.float64, device=x.device)
        work = _workspace(lib, N, D, x.device)
        _lib.check(lib.mb_knn_radii(x.data_ptr(), code, N, D, stride, k, radii2.data_ptr(), work.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "mb_knn_radii")
    return radii2


def manifold_coverage(queries: torch.Tensor, base: torch.Tensor, radii2: torch.Tensor) -> torch.Tensor:
    """queries [Nq, D], base [Nb, D], radii2 [Nb] (``knn_radii(base)``) -> bool [Nq]: whether the query lies within the radius of at least one
    base row (squared distance <= radii2, as ADM's ``evaluate_pr`` compares).  The two sets may differ in dtype and stride."""
    q, q_code, q_stride = _device_rows(queries, "queries")
    b, b_code, b_stride = _device_rows(base, "base")
    if b.device != q.device:
        raise ValueError(f"queries are on {q.device}, base on {b.device}")
    Nq, D = (int(v) for v in q.shape)
    Nb = int(b.shape[0])
    if int(b.shape[1]) != D:
        raise ValueError(f"queries have {D} columns, base {int(b.shape[1])}")
    if not isinstance(radii2, torch.Tensor) or tuple(radii2.shape) != (Nb,):
        raise ValueError(f"radii2 must be a tensor of {Nb} values, one per base row")
    r2 = radii2.detach().to(q.device, torch.float64).contiguous()
    lib = _lib.load()
    with torch.cuda.device(q.device):
        inside = torch.empty(Nq, dtype=torch.uint8, device=q.device)
        work = _workspace(lib, Nq + Nb, D, q.device)
        _lib.check(lib.mb_manifold_cover(q.data_ptr(), q_code, Nq, q_stride, b.data_ptr(), b_code, Nb, b_stride, D, r2.data_ptr(),
                                         inside.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream), "mb_manifold_cover")
    return inside.view(torch.bool)


def precision_recall(reference_features: torch.Tensor, sample_features: torch.Tensor, k: int = 3) -> Tuple[float, float]:
    """ADM's ``compute_prec_recall``: (share of sample rows inside the reference manifold, share of reference rows inside the sample manifold).
    One device-to-host copy of the two counts."""
    ref_radii2 = knn_radii(reference_features, k)
    sample_radii2 = knn_radii(sample_features, k)
    in_ref = manifold_coverage(sample_features, reference_features, ref_radii2)
    in_sample = manifold_coverage(reference_features, sample_features, sample_radii2)
    counts = torch.stack([in_ref.sum(), in_sample.sum()]).cpu()
    return int(counts[0]) / int(sample_features.shape[0]), int(counts[1]) / int(reference_features.shape[0])
