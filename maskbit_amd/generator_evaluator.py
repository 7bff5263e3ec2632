"""Generator evaluation on the device: the reference's ``GeneratorEvaluator`` (evaluator/evaluator.py:469-641) behind the gfx950 kernels of
``csrc/fid.hip`` and the codebook histogram of ``csrc/evaluator.hip``.

Same constructor keywords, ``reset_metrics()``, ``update(generated_images, codebook_indices=None)`` and ``result()`` with the keys
``InceptionScore``, ``FID``, ``CodebookUsage``, ``CodebookEntropy``.  The Inception network and the ImageNet statistics file are the caller's:
``use_inception(extractor, real_statistics)`` attaches any callable with the contract of the reference's ``get_inception_model()`` -- uint8
``[B, 3, H, W]`` in, ``{"2048": [B, D], "logits_unbiased": [B, C]}`` out.  Everything after the network runs here.  Per batch the reference
builds B ``torch.outer`` temporaries of D x D float64 and adds each to its state (evaluator.py:567-569); ``mb_fid_accumulate`` is one fp64 MFMA
rank-B update that reads and writes the upper half of that state once, and ``mb_is_accumulate`` is the softmax / log / column-sum chain of
evaluator.py:553-564 in float64.  The state -- ``total`` [D], ``sigma`` [D, D], ``prob_total`` / ``kl_total`` [C], the index histogram -- stays on
the device; updates enqueue on the current stream and never synchronise; ``result()`` makes one device-to-host copy.  There is no CPU path for
the evaluator; ``frechet_distance``, ``inception_score`` and ``get_covariance`` are plain torch and take CPU tensors.

Beyond the reference, the rest of ADM's table: ``use_precision_recall(reference_features)`` collects the pool features on the device and ``result()``
adds ``Precision`` / ``Recall`` (``maskbit_amd.manifold``, ``csrc/manifold.hip``); ``use_spatial_statistics((mu_s, sigma_s))`` accumulates a second
state over the extractor's ``"spatial"`` features and ``result()`` adds ``sFID``.  Both are methods, not constructor keywords, and without them
``result()`` is what it was.
"""
from __future__ import annotations

import os
from typing import Callable, Mapping, Optional, Text, Tuple, Union

import numpy as np
import torch

from . import _lib
from .manifold import MAX_K, precision_recall

_IS_EPS = 1e-16                          # evaluator.py:509
_HOW_TO_ATTACH = ("attach a feature extractor first: evaluator.use_inception(extractor, real_statistics), where extractor(uint8 [B,3,H,W]) returns "
                  "{'2048': [B,D], 'logits_unbiased': [B,C]} (the reference's metrics.inception.get_inception_model() is one) and real_statistics "
                  "is (mu, sigma) or the path of an .npz with 'mu' / 'sigma'")


# ---- the closed forms (torch only, any device) -----------------------------------------------------------------------------------------------
def get_covariance(sigma: torch.Tensor, total: torch.Tensor, num_examples: int) -> torch.Tensor:
    """The covariance from the sum of outer products and the sum of the features (evaluator.py:86-101)."""
    if num_examples == 0:
        return torch.zeros_like(sigma)
    sub_matrix = torch.outer(total, total) / num_examples
    return (sigma - sub_matrix) / (num_examples - 1)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2) in float64 (evaluator.py:605-626).  S1 S2 is similar to the symmetric positive
    semi-definite S1^(1/2) S2 S1^(1/2), so tr sqrt(S1 S2) is the sum of the square roots of that matrix's eigenvalues: two ``eigh`` calls with the
    eigenvalues clamped at 0, in place of the reference's ``scipy.linalg.sqrtm`` of the non-symmetric product."""
    mu1, mu2 = torch.as_tensor(mu1).double().flatten(), torch.as_tensor(mu2).double().flatten()
    s1, s2 = torch.as_tensor(sigma1).double(), torch.as_tensor(sigma2).double()
    D = mu1.numel()
    if mu2.numel() != D or tuple(s1.shape) != (D, D) or tuple(s2.shape) != (D, D):
        raise ValueError(f"frechet_distance: mu of {mu1.numel()} / {mu2.numel()} and sigma of {tuple(s1.shape)} / {tuple(s2.shape)} do not agree")
    mu2, s1, s2 = mu2.to(mu1.device), s1.to(mu1.device), s2.to(mu1.device)
    s1, s2 = (s1 + s1.T) / 2, (s2 + s2.T) / 2
    w, v = torch.linalg.eigh(s1)
    root = (v * w.clamp_min(0.0).sqrt()) @ v.T
    m = root @ s2 @ root
    tr_covmean = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0.0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2 * tr_covmean)


def inception_score(prob_total: torch.Tensor, kl_total: torch.Tensor, num_examples: int) -> float:
    """exp of the mean KL divergence between p(y|x) and p(y) from the two running sums (evaluator.py:586-593) in float64."""
    prob_total, kl_total = prob_total.double(), kl_total.double()
    mean_probs = prob_total / num_examples
    log_mean_probs = torch.log(mean_probs + _IS_EPS)
    excess_entropy = prob_total * log_mean_probs
    avg_kl_d = torch.sum(kl_total - excess_entropy) / num_examples
    return torch.exp(avg_kl_d).item()


def load_statistics(real_statistics) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mu, sigma)``, or the path of an ``.npz`` with ``mu`` / ``sigma`` (what the reference's ``read_imagenet_train_stats`` reads,
    evaluator.py:104-142) -> float64 CPU tensors [D], [D, D]."""
    if isinstance(real_statistics, (str, os.PathLike)):
        if not os.path.isfile(real_statistics):
            raise ValueError(f"statistics file does not exist at {real_statistics}")
        with np.load(real_statistics) as z:
            for key in ("mu", "sigma"):
                if key not in z:
                    raise ValueError(f'statistics file must contain a "{key}" key')
            real_statistics = (z["mu"], z["sigma"])
    mu, sigma = real_statistics
    mu = torch.as_tensor(mu).detach().to("cpu", torch.float64).flatten()
    sigma = torch.as_tensor(sigma).detach().to("cpu", torch.float64)
    if tuple(sigma.shape) != (mu.numel(), mu.numel()):
        raise ValueError(f"statistics: mu of {mu.numel()} values needs a sigma of that size squared, got {tuple(sigma.shape)}")
    return mu, sigma


# ---- the device state ---------------------------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor, device: torch.device) -> Tuple[torch.Tensor, int, int]:
    """[B, N] of any float dtype -> (fp32 or fp64 tensor on ``device`` with unit column stride, dtype code, row stride in elements)."""
    x = x.detach().to(device)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    B, N = x.shape
    if x.stride(1) != 1 or (B > 1 and x.stride(0) < N):
        x = x.contiguous()
    return x, (1 if x.dtype == torch.float64 else 0), (x.stride(0) if B > 1 else N)


def _check_rows(x, what: str, width: Optional[int]) -> Tuple[int, int]:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"{what} must be a floating-point [B, N] tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    B, N = (int(v) for v in x.shape)
    if B < 1 or N < 1:
        raise ValueError(f"{what}: empty batch {tuple(x.shape)}")
    if width is not None and N != width:
        raise ValueError(f"{what} has {N} columns; this pass was started with {width} (reset_metrics() starts a new one)")
    return B, N


class FeatureStatistics:
    """``total`` [D] and ``sigma`` [D, D] of one feature stream in float64 on the device (evaluator.py:523-529), fed by ``mb_fid_accumulate``.
    D is fixed by the first batch of a pass.  The kernel keeps only the blocks on and above the diagonal; ``full_sigma()`` is the symmetric matrix."""

    def __init__(self, device: torch.device):
        self.device = device
        self.width: Optional[int] = None
        self.total: Optional[torch.Tensor] = None
        self.sigma: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.width = self.total = self.sigma = None

    def add(self, feats: torch.Tensor) -> None:
        B, D = _check_rows(feats, "features", self.width)
        lib = _lib.load()
        if self.width is None:
            self.width = D
            self.total = torch.zeros(D, dtype=torch.float64, device=self.device)
            self.sigma = torch.zeros((D, D), dtype=torch.float64, device=self.device)
        x, code, stride = _rows(feats, self.device)
        _lib.check(lib.mb_fid_accumulate(x.data_ptr(), code, B, D, stride, self.total.data_ptr(), self.sigma.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "mb_fid_accumulate")

    def full_sigma(self) -> torch.Tensor:
        upper = torch.triu(self.sigma)
        return upper + torch.triu(self.sigma, 1).T


class ScoreStatistics:
    """``prob_total`` and ``kl_total`` [C] in float64 on the device (evaluator.py:517-522), fed by ``mb_is_accumulate``."""

    def __init__(self, device: torch.device):
        self.device = device
        self.width: Optional[int] = None
        self.sums: Optional[torch.Tensor] = None           # [2, C]: prob_total, kl_total
        self._workspace: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.width = self.sums = None

    def add(self, logits: torch.Tensor) -> None:
        B, C = _check_rows(logits, "logits", self.width)
        lib = _lib.load()
        need = int(lib.mb_is_workspace_bytes(B, C))
        if need == 0:
            raise ValueError(f"logits of {tuple(logits.shape)} are outside what mb_is_accumulate takes")
        if self.width is None:
            self.width = C
            self.sums = torch.zeros((2, C), dtype=torch.float64, device=self.device)
        if self._workspace is None or self._workspace.numel() * 8 < need:
            self._workspace = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        x, code, stride = _rows(logits, self.device)
        _lib.check(lib.mb_is_accumulate(x.data_ptr(), code, B, C, stride, self.sums[0].data_ptr(), self.sums[1].data_ptr(),
                                        self._workspace.data_ptr(), torch.cuda.current_stream().cuda_stream), "mb_is_accumulate")


def extract_all(extractor: Callable, u8_nchw: torch.Tensor, want_pool: bool, want_logits: bool, want_spatial: bool):
    """Runs the attached network on uint8 [B, 3, H, W] -> (pool or None, logits or None, spatial or None), checking the contract of
    ``get_inception_model()``; ``spatial`` is the key of sFID (``InceptionV3(features_list=[..., "spatial"])``)."""
    out = extractor(u8_nchw)
    for key, want in (("2048", want_pool), ("logits_unbiased", want_logits), ("spatial", want_spatial)):
        if want and (not isinstance(out, Mapping) or key not in out):
            raise ValueError(f"the feature extractor must return a mapping with the key {key!r} (metrics/inception.py)" if key != "spatial" else
                             "use_spatial_statistics() is attached: the feature extractor must also return the key 'spatial' "
                             "(InceptionV3(features_list=['2048', 'logits_unbiased', 'spatial']))")
    return (out["2048"] if want_pool else None), (out["logits_unbiased"] if want_logits else None), (out["spatial"] if want_spatial else None)


def extract(extractor: Callable, u8_nchw: torch.Tensor, want_pool: bool, want_logits: bool):
    """``extract_all`` without the spatial features -> (pool or None, logits or None)."""
    return extract_all(extractor, u8_nchw, want_pool, want_logits, False)[:2]


def to_uint8(images: torch.Tensor) -> torch.Tensor:
    """``(images * 255).to(torch.uint8)`` (evaluator.py:550)."""
    return (images * 255).to(torch.uint8)


class GeneratorEvaluator:
    def __init__(
        self,
        device,
        enable_fid: bool = False,
        enable_inception_score: bool = False,
        enable_codebook_usage_measure: bool = False,
        enable_codebook_entropy_measure: bool = False,
        test_resolution: int = 256,
        num_codebook_entries: int = 1024,
    ):
        """Nothing is allocated and the device is not touched before the first update.  ``test_resolution`` selects the reference's statistics
        file (evaluator.py:508); here the statistics come through ``use_inception`` and the value is only checked (256 or 512)."""
        self._device = torch.device(device)
        if self._device.type != "cuda":
            raise RuntimeError(f"GeneratorEvaluator runs only on an AMD GPU through libmaskbit_hip.so (device is {self._device}); "
                               "maskbit_amd has no CPU path.")
        if test_resolution not in (256, 512):
            raise ValueError(f"Resolution {test_resolution} is not supported. Please choose 256 or 512.")
        self._enable_fid = bool(enable_fid)
        self._enable_inception_score = bool(enable_inception_score)
        self._enable_codebook_usage_measure = bool(enable_codebook_usage_measure)
        self._enable_codebook_entropy_measure = bool(enable_codebook_entropy_measure)
        self._test_resolution = int(test_resolution)
        self._num_codebook_entries = int(num_codebook_entries)
        if self._num_codebook_entries < 1:
            raise ValueError(f"num_codebook_entries={num_codebook_entries}: at least one entry")
        self._codebook = self._enable_codebook_usage_measure or self._enable_codebook_entropy_measure
        self._network = self._enable_fid or self._enable_inception_score
        self._inception_model: Optional[Callable] = None
        self._fid_real_mu: Optional[torch.Tensor] = None
        self._fid_real_sigma: Optional[torch.Tensor] = None
        self._fid: Optional[FeatureStatistics] = None
        self._is: Optional[ScoreStatistics] = None
        self._hist: Optional[torch.Tensor] = None
        self._out_of_range: Optional[torch.Tensor] = None
        self._pr_reference: Optional[torch.Tensor] = None  # use_precision_recall: [Nr, D] as given, moved to the device by result()
        self._pr_k = 3
        self._pr_capacity = 0                              # rows the buffer is allocated with at the first update
        self._pr_rows: Optional[torch.Tensor] = None       # fp32 [capacity, D] on the device; the first _pr_count rows are the pass's pool features
        self._pr_count = 0
        self._sfid_real_mu: Optional[torch.Tensor] = None  # use_spatial_statistics
        self._sfid_real_sigma: Optional[torch.Tensor] = None
        self._sfid: Optional[FeatureStatistics] = None
        self.reset_metrics()

    def _bind_device(self) -> torch.device:
        """The device with its index resolved, and the state objects: at the first update, so that construction does no device work."""
        if self._fid is None:
            if self._device.index is None:
                self._device = torch.device("cuda", torch.cuda.current_device())
            self._fid, self._is = FeatureStatistics(self._device), ScoreStatistics(self._device)
        return self._device

    def reset_metrics(self):
        """Resets all metrics; the feature widths D and C are taken again from the next update."""
        self._num_examples = 0
        self._num_updates = 0
        if self._fid is not None:
            self._fid.reset()
            self._is.reset()
        if self._hist is not None:
            self._hist.zero_()
            self._out_of_range.zero_()
        self._pr_count = 0
        if self._sfid is not None:
            self._sfid.reset()

    def use_inception(self, extractor: Optional[Callable], real_statistics=None) -> None:
        """Attaches the feature extractor (``None`` detaches) and, if given, the real statistics FID is measured against: ``(mu, sigma)`` or the
        path of an ``.npz`` with ``mu`` / ``sigma`` keys.  Takes the place of ``get_inception_model()`` and ``read_imagenet_train_stats()`` in the
        reference's constructor (evaluator.py:506-508), neither of which can be fetched here."""
        if extractor is not None and not callable(extractor):
            raise TypeError(f"use_inception() takes a callable, got {type(extractor).__name__}")
        if real_statistics is not None:
            self._fid_real_mu, self._fid_real_sigma = load_statistics(real_statistics)
        self._inception_model = extractor

    def use_precision_recall(self, reference_features: Optional[torch.Tensor], k: int = 3, max_samples: Optional[int] = None) -> None:
        """Attaches the reference set of the improved precision / recall (``manifold.precision_recall``, ADM's ``compute_prec_recall``):
        ``reference_features`` [Nr, D], the pool features of the reference images, on any device; ``None`` detaches.  From then on every update
        also appends its pool features to an fp32 device buffer -- allocated with ``max_samples`` rows if given (50 000 x 2048 is 410 MB), doubled
        whenever it is full -- without synchronising, and ``result()`` reports ``Precision`` and ``Recall`` after its other keys.  Rows collected
        so far are kept; ``reset_metrics()`` empties the buffer."""
        if reference_features is None:
            self._pr_reference = self._pr_rows = None
            self._pr_count = self._pr_capacity = 0
            return
        if not self._enable_fid:
            raise ValueError("use_precision_recall needs the pool features: construct the evaluator with enable_fid=True")
        r = reference_features
        if not isinstance(r, torch.Tensor) or r.dim() != 2 or not r.is_floating_point():
            raise ValueError(f"reference_features must be a floating-point [Nr, D] tensor, got {tuple(r.shape) if isinstance(r, torch.Tensor) else type(r).__name__}")
        k = int(k)
        if k < 1 or k > MAX_K:
            raise ValueError(f"k = {k}: 1 <= k <= {MAX_K}")
        if int(r.shape[0]) < k + 1 or int(r.shape[1]) < 1:
            raise ValueError(f"reference_features of {tuple(r.shape)}: at least k + 1 = {k + 1} rows are needed")
        if max_samples is not None and int(max_samples) < 1:
            raise ValueError(f"max_samples = {max_samples}: at least one row, or None")
        if self._fid is not None and self._fid.width is not None and int(r.shape[1]) != self._fid.width:
            raise ValueError(f"reference_features have {int(r.shape[1])} columns; this pass was started with {self._fid.width}")
        self._pr_reference, self._pr_k = r.detach(), k
        self._pr_capacity = int(max_samples) if max_samples is not None else 0

    def use_spatial_statistics(self, real_statistics_s) -> None:
        """Attaches the real statistics of sFID: ``(mu_s, sigma_s)`` or the path of an ``.npz`` with those two keys (the names in ADM's reference
        batches), of the width of the extractor's ``"spatial"`` features (2023 for ``InceptionV3``); ``None`` detaches.  From then on the attached
        extractor must return ``"spatial"`` (``update_features_spatial`` takes the features directly), a second running state of that width is
        accumulated by ``mb_fid_accumulate``, and ``result()`` reports ``sFID`` after its other keys.  What the spatial features are, and why no parity
        with published sFID values is claimed, is stated in DESIGN.md "sFID"."""
        if real_statistics_s is None:
            self._sfid_real_mu = self._sfid_real_sigma = self._sfid = None
            return
        if self._num_examples:
            raise ValueError("use_spatial_statistics: a pass is in progress; attach before the first update or after reset_metrics()")
        if isinstance(real_statistics_s, (str, os.PathLike)):
            if not os.path.isfile(real_statistics_s):
                raise ValueError(f"statistics file does not exist at {real_statistics_s}")
            with np.load(real_statistics_s) as z:
                for key in ("mu_s", "sigma_s"):
                    if key not in z:
                        raise ValueError(f'spatial statistics file must contain a "{key}" key')
                real_statistics_s = (z["mu_s"], z["sigma_s"])
        self._sfid_real_mu, self._sfid_real_sigma = load_statistics(real_statistics_s)
        self._sfid = None                                  # bound to the device at the next update

    def _collect(self, pool: torch.Tensor, dev: torch.device) -> None:
        """Appends a batch's pool features to the buffer of use_precision_recall.  Enqueued on the current stream, no synchronisation."""
        B, D = (int(v) for v in pool.shape)
        need = self._pr_count + B
        if self._pr_rows is None or self._pr_rows.shape[1] != D or need > self._pr_rows.shape[0]:
            have = 0 if self._pr_rows is None or self._pr_rows.shape[1] != D else int(self._pr_rows.shape[0])
            rows = max(need, 2 * have, self._pr_capacity, 1024)
            grown = torch.empty((rows, D), dtype=torch.float32, device=dev)
            if self._pr_count:
                grown[:self._pr_count].copy_(self._pr_rows[:self._pr_count])
            self._pr_rows = grown
        self._pr_rows[self._pr_count:need].copy_(pool.detach())
        self._pr_count = need

    # -- the three ways in -----------------------------------------------------------------------------------------------------------------
    def update(self, generated_images: torch.Tensor, codebook_indices: Optional[torch.Tensor] = None):
        """Adds a batch of float images [B, 3, H, W] in [0, 1] (evaluator.py:533-576)."""
        if generated_images.dim() != 4:
            raise ValueError(f"update expects [B, C, H, W] images, got {tuple(generated_images.shape)}")
        if not self._network:
            return self._update(int(generated_images.shape[0]), None, None, codebook_indices)
        self._require_extractor()
        self.update_uint8(to_uint8(generated_images), codebook_indices)

    def update_uint8(self, u8_nchw: torch.Tensor, codebook_indices: Optional[torch.Tensor] = None):
        """Adds a batch given as the uint8 [B, 3, H, W] bytes the network reads (``harness.to_evaluator_uint8`` of the decoder's output)."""
        if u8_nchw.dim() != 4 or u8_nchw.dtype != torch.uint8:
            raise ValueError(f"update_uint8 expects uint8 [B, C, H, W], got {u8_nchw.dtype} {tuple(u8_nchw.shape)}")
        if not self._network:
            return self._update(int(u8_nchw.shape[0]), None, None, codebook_indices)
        self._require_extractor()
        self._check_indices(codebook_indices)
        pool, logits, spatial = extract_all(self._inception_model, u8_nchw, self._enable_fid, self._enable_inception_score,
                                            self._sfid_real_mu is not None)
        self._update(int(u8_nchw.shape[0]), pool, logits, codebook_indices, spatial)

    def update_features(self, pool: Optional[torch.Tensor], logits: Optional[torch.Tensor], codebook_indices: Optional[torch.Tensor] = None):
        """Adds a batch whose features are already at hand: ``pool`` [B, D] (needed when FID is enabled) and ``logits`` [B, C] (needed when the
        Inception score is), fp32 or fp64, rows of any stride."""
        given = pool if pool is not None else logits
        if given is None or not isinstance(given, torch.Tensor) or given.dim() != 2:
            raise ValueError("update_features needs pool [B, D] or logits [B, C]")
        self._update(int(given.shape[0]), pool, logits, codebook_indices)

    def update_features_spatial(self, pool: Optional[torch.Tensor], logits: Optional[torch.Tensor], spatial: torch.Tensor,
                                codebook_indices: Optional[torch.Tensor] = None):
        """``update_features`` with the batch's spatial features [B, S] for sFID (``use_spatial_statistics`` must be attached)."""
        if self._sfid_real_mu is None:
            raise ValueError("update_features_spatial: no spatial statistics are attached (use_spatial_statistics)")
        if not isinstance(spatial, torch.Tensor) or spatial.dim() != 2:
            raise ValueError("update_features_spatial needs spatial [B, S]")
        self._update(int(spatial.shape[0]), pool, logits, codebook_indices, spatial)

    def _require_extractor(self) -> None:
        if self._inception_model is None:
            raise RuntimeError("FID / Inception score are enabled but no feature extractor is attached: " + _HOW_TO_ATTACH)

    def _check_indices(self, codebook_indices) -> None:
        if not self._codebook:
            return
        if codebook_indices is None:
            raise ValueError("codebook_indices is required when a codebook metric is enabled")
        if codebook_indices.is_floating_point() or codebook_indices.is_complex():
            raise ValueError(f"codebook_indices must be an integer tensor, got {codebook_indices.dtype}")

    def _update(self, B: int, pool, logits, codebook_indices, spatial=None) -> None:
        """Every check first, then the device work."""
        if B < 1:
            raise ValueError("empty batch")
        if self._enable_fid and pool is None:
            raise ValueError("FID is enabled: pool features [B, D] are required")
        if self._enable_inception_score and logits is None:
            raise ValueError("the Inception score is enabled: logits [B, C] are required")
        for x, on, width, what in ((pool, self._enable_fid, self._fid.width if self._fid else None, "features"),
                                   (logits, self._enable_inception_score, self._is.width if self._is else None, "logits")):
            if on and _check_rows(x, what, width)[0] != B:
                raise ValueError(f"{what} of {tuple(x.shape)} for a batch of {B}")
        if self._enable_fid and self._fid_real_mu is not None and int(pool.shape[1]) != self._fid_real_mu.numel():
            raise ValueError(f"features have {int(pool.shape[1])} columns, the real statistics {self._fid_real_mu.numel()}")
        if self._pr_reference is not None and int(pool.shape[1]) != int(self._pr_reference.shape[1]):
            raise ValueError(f"features have {int(pool.shape[1])} columns, the reference features of use_precision_recall {int(self._pr_reference.shape[1])}")
        if self._sfid_real_mu is not None:
            if spatial is None:
                raise ValueError("use_spatial_statistics() is attached: spatial features [B, S] are required (update_features_spatial, or an "
                                 "extractor that returns 'spatial')")
            if _check_rows(spatial, "spatial features", self._sfid.width if self._sfid else None)[0] != B:
                raise ValueError(f"spatial features of {tuple(spatial.shape)} for a batch of {B}")
            if int(spatial.shape[1]) != self._sfid_real_mu.numel():
                raise ValueError(f"spatial features have {int(spatial.shape[1])} columns, the real spatial statistics {self._sfid_real_mu.numel()}")
        self._check_indices(codebook_indices)
        dev = self._bind_device()
        if self._sfid_real_mu is not None and self._sfid is None:
            self._sfid = FeatureStatistics(dev)
        self._num_examples += B
        self._num_updates += 1
        with torch.cuda.device(dev):
            if self._enable_fid:
                self._fid.add(pool)
                if self._pr_reference is not None:
                    self._collect(pool, dev)
            if self._sfid is not None:
                self._sfid.add(spatial)
            if self._enable_inception_score:
                self._is.add(logits)
            if self._codebook:
                lib = _lib.load()
                if self._hist is None:
                    self._hist = torch.zeros(self._num_codebook_entries, dtype=torch.int64, device=dev)
                    self._out_of_range = torch.zeros(1, dtype=torch.int32, device=dev)
                idx = codebook_indices.to(device=dev, dtype=torch.int64).contiguous()
                _lib.check(lib.mb_eval_codebook(idx.data_ptr(), idx.numel(), self._num_codebook_entries, self._hist.data_ptr(),
                                                self._out_of_range.data_ptr(), torch.cuda.current_stream().cuda_stream), "mb_eval_codebook")

    # -- reading the state ------------------------------------------------------------------------------------------------------------------
    def fid_statistics(self) -> Tuple[int, torch.Tensor, torch.Tensor]:
        """``(n, total [D], sigma [D, D])``: the number of examples and float64 device tensors, sigma as the full symmetric matrix -- what a run
        saves, and what ranks add up before ``get_covariance`` / ``frechet_distance``.  No synchronisation."""
        if not self._enable_fid or self._fid is None or self._fid.width is None:
            raise ValueError("no FID statistics: enable_fid and at least one update are needed")
        return self._num_examples, self._fid.total.clone(), self._fid.full_sigma()

    def spatial_statistics(self) -> Tuple[int, torch.Tensor, torch.Tensor]:
        """``fid_statistics()`` of the spatial features behind sFID: ``(n, total [S], sigma [S, S])``."""
        if self._sfid is None or self._sfid.width is None:
            raise ValueError("no spatial statistics: use_spatial_statistics() and at least one update are needed")
        return self._num_examples, self._sfid.total.clone(), self._sfid.full_sigma()

    def is_statistics(self) -> Tuple[int, torch.Tensor, torch.Tensor]:
        """``(n, prob_total [C], kl_total [C])`` as float64 device tensors."""
        if not self._enable_inception_score or self._is is None or self._is.width is None:
            raise ValueError("no Inception score statistics: enable_inception_score and at least one update are needed")
        return self._num_examples, self._is.sums[0].clone(), self._is.sums[1].clone()

    def result(self) -> Mapping[Text, Union[float, torch.Tensor]]:
        """Keys, order and types of evaluator.py:579-641: Python floats, except ``CodebookEntropy``, a 0-d float64 tensor on the evaluator's
        device.  One device-to-host copy of the state.  ``RuntimeError`` for FID without real statistics -- ``result()`` of an evaluator without
        ``enable_fid`` reports the rest; ``IndexError`` if an index fell outside [0, num_codebook_entries).  After them, when attached: ``sFID``
        (``use_spatial_statistics``; a second copy of its S x S state), ``Precision`` and ``Recall`` (``use_precision_recall``; two counts)."""
        if self._num_examples < 1:
            raise ValueError("No examples to evaluate.")
        if self._enable_fid and self._fid_real_mu is None:
            raise RuntimeError("FID needs the real statistics: use_inception(extractor, real_statistics=(mu, sigma) or an .npz path). "
                               "fid_statistics(), the Inception score and the codebook figures do not (construct without enable_fid).")
        if self._pr_reference is not None and self._pr_count < self._pr_k + 1:
            raise ValueError(f"Precision / Recall with k = {self._pr_k} need at least {self._pr_k + 1} samples, {self._pr_count} were collected "
                             "(rows are collected from use_precision_recall() on)")
        n = self._num_examples
        parts, entropy = [], None
        if self._enable_fid:
            D = self._fid.width
            parts += [self._fid.total, self._fid.full_sigma().reshape(-1)]
        if self._enable_inception_score:
            C = self._is.width
            parts.append(self._is.sums.reshape(-1))
        if self._codebook:
            counts = self._hist.double()
            probs = counts / counts.sum()
            entropy = (-torch.log2(probs + 1e-8) * probs).sum()                                # evaluator.py:637-638
            parts += [(self._hist != 0).sum().double().reshape(1), (self._out_of_range.long() & 0xFFFFFFFF).double()]
        host = torch.cat(parts).cpu() if parts else torch.zeros(0, dtype=torch.float64)        # the one copy
        if self._codebook and host[-1] != 0:
            raise IndexError(f"{int(host[-1])} codebook indices outside [0, {self._num_codebook_entries})")
        eval_score = {}
        at = 0
        if self._enable_fid:
            total, sigma = host[:D], host[D:D + D * D].reshape(D, D)
            at = D + D * D
        if self._enable_inception_score:
            eval_score["InceptionScore"] = inception_score(host[at:at + C], host[at + C:at + 2 * C], n)
        if self._enable_fid:
            eval_score["FID"] = frechet_distance(self._fid_real_mu, self._fid_real_sigma, total / n, get_covariance(sigma, total, n))
        if self._enable_codebook_usage_measure:
            eval_score["CodebookUsage"] = float(int(host[-2])) / self._num_codebook_entries
        if self._enable_codebook_entropy_measure:
            eval_score["CodebookEntropy"] = entropy
        if self._sfid is not None:                         # its own copy: 2023^2 doubles, kept out of the state above so that its layout stands
            total_s, sigma_s = self._sfid.total.cpu(), self._sfid.full_sigma().cpu()
            eval_score["sFID"] = frechet_distance(self._sfid_real_mu, self._sfid_real_sigma, total_s / n, get_covariance(sigma_s, total_s, n))
        if self._pr_reference is not None:
            with torch.cuda.device(self._device):
                self._pr_reference = self._pr_reference.to(self._device)
                eval_score["Precision"], eval_score["Recall"] = precision_recall(self._pr_reference, self._pr_rows[:self._pr_count], self._pr_k)
        return eval_score
