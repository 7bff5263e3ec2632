"""Tokenizer evaluation on the device: the reference's ``TokenizerEvaluator`` (evaluator/evaluator.py:145-466) behind the gfx950 kernels of
``csrc/evaluator.hip``.

Same constructor keywords, ``reset_metrics()``, ``update(real_images, fake_images, codebook_indices=None)`` and ``result()``.  In scope are
the six closed-form metrics -- MAE, MSE, PSNR, SSIM (11 x 11 Gaussian window, sigma 1.5, reflect padding, k1 / k2 = 0.01 / 0.03, data range 1),
CodebookUsage and CodebookEntropy.  ``update()`` is two kernels for the images (``mb_eval_images``: one read of both images for all four image
metrics, then a small deterministic finalize) and one for the indices (``mb_eval_codebook``: a histogram, in place of two ``torch.unique``
calls and a ``.tolist()`` into a Python set); it enqueues on the current stream and never synchronises.  The running state -- four float64
sums, an int64 histogram, an out-of-range counter -- stays on the device; ``result()`` makes one device-to-host copy.

``enable_rfid``, ``enable_inception_score`` and ``enable_lpips_score`` raise at construction: those flags mean "fetch the network and its
weights", which cannot be honoured here.  LPIPS itself is built (``maskbit_amd.LPIPS``, csrc/lpips.hip): attach a model that
holds the user's weights with ``use_lpips(model)`` and ``update()`` also enqueues ``mb_lpips_forward`` on the same images into a float64 device
sum; ``result()`` reports ``"LPIPS"`` where the reference does.  rFID and the Inception score work the same way: ``use_inception(extractor)``
attaches the caller's Inception network, and everything after it -- the statistics of real and fake features (csrc/fid.hip) and the two closed
forms -- runs here (``generator_evaluator.py``, which also holds ``GeneratorEvaluator``).  There is no CPU path.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Mapping, Optional, Text

import torch

from . import _lib
from .generator_evaluator import (FeatureStatistics, GeneratorEvaluator, ScoreStatistics, extract, frechet_distance,  # noqa: F401
                                  get_covariance, inception_score, to_uint8)

_ABS, _SQ, _SSIM = 1, 2, 4          # metrics bits of mb_eval_images


class TokenizerEvaluator:
    def __init__(
        self,
        device,
        enable_rfid: bool = False,
        enable_inception_score: bool = False,
        enable_psnr_score: bool = False,
        enable_ssim_score: bool = False,
        enable_lpips_score: bool = False,
        enable_mse_error: bool = False,
        enable_mae_error: bool = False,
        enable_codebook_usage_measure: bool = False,
        enable_codebook_entropy_measure: bool = False,
        num_codebook_entries: int = 1024
    ):
        for flag, name in ((enable_rfid, "enable_rfid"), (enable_inception_score, "enable_inception_score"), (enable_lpips_score, "enable_lpips_score")):
            if flag:
                raise NotImplementedError(
                    f"{name}: rFID, Inception score and LPIPS need the Inception / LPIPS networks and their weights, which are out of scope here "
                    "(SURVEY.md section 2). Run them with the reference's own evaluator beside this one (evaluator.TokenizerEvaluator with only "
                    "those flags set; both take the same update() arguments)."
                    + (" LPIPS itself runs here with your own weights: build a maskbit_amd.LPIPS, load it (load_vgg16, load_linear) and attach it "
                       "with TokenizerEvaluator.use_lpips(model)." if name == "enable_lpips_score" else ""))
        self._device = torch.device(device)
        if self._device.type != "cuda":
            raise RuntimeError(f"TokenizerEvaluator runs only on an AMD GPU through libmaskbit_hip.so (device is {self._device}); "
                               "maskbit_amd has no CPU path.")
        self._enable_psnr_score = bool(enable_psnr_score)
        self._enable_ssim_score = bool(enable_ssim_score)
        self._enable_mse_error = bool(enable_mse_error)
        self._enable_mae_error = bool(enable_mae_error)
        self._enable_codebook_usage_measure = bool(enable_codebook_usage_measure)
        self._enable_codebook_entropy_measure = bool(enable_codebook_entropy_measure)
        self._num_codebook_entries = int(num_codebook_entries)
        if self._num_codebook_entries < 1:
            raise ValueError(f"num_codebook_entries={num_codebook_entries}: at least one entry")
        self._metrics = ((_ABS if self._enable_mae_error else 0) | (_SQ if self._enable_mse_error or self._enable_psnr_score else 0)
                         | (_SSIM if self._enable_ssim_score else 0))
        self._codebook = self._enable_codebook_usage_measure or self._enable_codebook_entropy_measure
        self._workspace: Optional[torch.Tensor] = None
        self._sums: Optional[torch.Tensor] = None
        self._hist: Optional[torch.Tensor] = None
        self._out_of_range: Optional[torch.Tensor] = None
        self.last_per_image: Optional[torch.Tensor] = None
        # the attached pair losses in the order of result(): the result key, the model (None: detached), the float64 device sum, the last batch's [B] values
        self._pair_losses = [SimpleNamespace(key=key, model=None, sum=None, last=None) for key in ("LPIPS", "PerceptualLoss")]
        self._disc = None                                                                     # use_discriminator(): the model, its loss kind, float64 [2, 5] sums
        self._disc_loss = "hinge"
        self._disc_sums: Optional[torch.Tensor] = None
        self._inception = None                                                                # use_inception(): the extractor and its three states
        self._rfid = self._inception_score = False
        self._is_stats = self._rfid_real = self._rfid_fake = None
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        self.reset_metrics()

    def reset_metrics(self):
        """Resets all metrics (the device state is zeroed by enqueued fills; no synchronisation)."""
        self._num_examples = 0
        self._num_updates = 0
        if self._sums is None:
            _lib.load()
            self._sums = torch.zeros(4, dtype=torch.float64, device=self._device)                 # MAE, MSE, PSNR, SSIM sums of per-image terms
            self._hist = torch.zeros(self._num_codebook_entries if self._codebook else 1, dtype=torch.int64, device=self._device)
            self._out_of_range = torch.zeros(1, dtype=torch.int32, device=self._device)
        else:
            self._sums.zero_()
            self._hist.zero_()
            self._out_of_range.zero_()
        self.last_per_image = None
        for row in self._pair_losses:
            row.last = None
            if row.sum is not None:
                row.sum.zero_()
        for stats in (self._is_stats, self._rfid_real, self._rfid_fake):
            if stats is not None:
                stats.reset()
        if self._disc_sums is not None:
            self._disc_sums.zero_()

    def use_inception(self, extractor, rfid: bool = True, inception_score: bool = True) -> None:
        """Attaches a feature extractor with the contract of the reference's ``get_inception_model()`` -- uint8 [B, 3, H, W] in,
        ``{"2048": [B, D], "logits_unbiased": [B, C]}`` out -- (``None`` detaches): ``update()`` then runs it on ``(images * 255).to(uint8)`` of the
        fake images, and for rFID of the real ones, and accumulates the statistics with ``mb_is_accumulate`` / ``mb_fid_accumulate``
        (evaluator.py:336-364); ``result()`` reports ``"InceptionScore"`` and ``"rFID"`` where the reference does (evaluator.py:406-451).  Takes
        the place of ``enable_rfid`` / ``enable_inception_score``, whose network cannot be fetched here.  Attach before the first ``update()`` of a
        pass, or call ``reset_metrics()``."""
        if extractor is None:
            self._inception, self._rfid, self._inception_score = None, False, False
            return
        if not callable(extractor):
            raise TypeError(f"use_inception() takes a callable, got {type(extractor).__name__}")
        if not (rfid or inception_score):
            raise ValueError("use_inception(): rfid or inception_score must be asked for")
        self._inception, self._rfid, self._inception_score = extractor, bool(rfid), bool(inception_score)
        if self._is_stats is None:
            self._is_stats, self._rfid_real, self._rfid_fake = (ScoreStatistics(self._device), FeatureStatistics(self._device),
                                                                FeatureStatistics(self._device))

    def use_lpips(self, model) -> None:
        """Attaches a loaded ``maskbit_amd.LPIPS`` on the evaluator's device (``None`` detaches): ``update()`` then also adds the batch's LPIPS
        values to a float64 device sum (``last_lpips`` holds the batch's [B] values) and ``result()`` reports ``"LPIPS"``.  Takes the place of
        the reference's ``enable_lpips_score`` (evaluator.py:223-226,366-368,453-455), whose weights cannot be fetched here.  Attach before the
        first ``update()`` of a pass, or call ``reset_metrics()``: the mean is over all examples counted."""
        from .lpips import LPIPS
        self._use_pair_loss(self._pair_losses[0], model, LPIPS, "use_lpips")

    def use_perceptual(self, model) -> None:
        """Attaches a loaded ``maskbit_amd.PerceptualLoss`` on the evaluator's device (``None`` detaches): ``update()`` then also adds the batch's
        per-pair ResNet-50 perceptual distances to a float64 device sum (``last_perceptual`` holds the batch's [B] values) and ``result()`` reports
        ``"PerceptualLoss"``, their mean -- what the reference's ``PerceptualLoss.forward`` gives over the same pairs.  The reference's evaluator
        has no such entry; the key is there only while a model is attached.  Attach before the first ``update()`` of a pass, or call
        ``reset_metrics()``."""
        from .perceptual import PerceptualLoss
        self._use_pair_loss(self._pair_losses[1], model, PerceptualLoss, "use_perceptual")

    def use_discriminator(self, model, loss: str = "hinge") -> None:
        """Attaches a loaded ``maskbit_amd.NLayerDiscriminatorv2`` on the evaluator's device (``None`` detaches): ``update()`` then also adds the
        five logit sums (``NLayerDiscriminatorv2.logit_stats``) of the real and of the fake batch to float64 device sums, without a
        synchronisation, and ``result()`` reports ``"LogitsReal"`` and ``"LogitsFake"`` (the mean logit), ``"DiscriminatorLoss"`` and
        ``"GeneratorLoss"`` of the kind ``loss`` (``"hinge"``, ``"vanilla"``, ``"non-saturating"``: the ``discriminator_loss`` of the training
        config) over all logits counted -- what the training step logs as ``logits_real``, ``logits_fake``, ``discriminator_loss`` (without
        the LeCam term) and ``gan_loss``, on held-out images.  The reference's evaluator has no such entries; the keys are there only while a
        model is attached.  Attach before the first ``update()`` of a pass, or call ``reset_metrics()``."""
        from .discriminator import D_LOSSES, NLayerDiscriminatorv2
        if model is None:
            self._disc = None
            return
        if not isinstance(model, NLayerDiscriminatorv2):
            raise TypeError(f"use_discriminator() takes a maskbit_amd.NLayerDiscriminatorv2, got {type(model).__name__}")
        if loss not in D_LOSSES:
            raise ValueError(f"use_discriminator(): loss {loss!r}: one of {sorted(D_LOSSES)}")
        dev = model._require_cuda("use_discriminator")
        if (dev.index if dev.index is not None else torch.cuda.current_device()) != self._device.index:
            raise ValueError(f"the NLayerDiscriminatorv2 model is on {dev}, the evaluator on {self._device}")
        self._disc, self._disc_loss = model, loss
        if self._disc_sums is None:
            self._disc_sums = torch.zeros((2, 5), dtype=torch.float64, device=self._device)

    def _use_pair_loss(self, row, model, cls, who: str) -> None:
        if model is None:
            row.model = None
            return
        if not isinstance(model, cls):
            raise TypeError(f"{who}() takes a maskbit_amd.{cls.__name__}, got {type(model).__name__}")
        dev = model._require_cuda(who)
        if (dev.index if dev.index is not None else torch.cuda.current_device()) != self._device.index:
            raise ValueError(f"the {cls.__name__} model is on {dev}, the evaluator on {self._device}")
        row.model = model
        if row.sum is None:
            row.sum = torch.zeros(1, dtype=torch.float64, device=self._device)

    last_lpips = property(lambda self: self._pair_losses[0].last)
    last_perceptual = property(lambda self: self._pair_losses[1].last)
    _lpips_sum = property(lambda self: self._pair_losses[0].sum)                                # (read by tests/test_hip_lpips.py)

    def update(self, real_images: torch.Tensor, fake_images: torch.Tensor, codebook_indices: Optional[torch.Tensor] = None, clamp: bool = False):
        """Adds a batch.  ``real_images`` / ``fake_images``: [B, C, H, W] of any float dtype (cast to contiguous fp32 only when needed), equal
        element counts (``real`` is viewed as ``fake``, evaluator.py:283), H, W >= 6, C == 3 when SSIM is enabled.  ``clamp=True`` clamps both
        to [0, 1] inside the kernel (eval_tokenizer.py:146-147).  ``codebook_indices``: integer tensor of any shape, required when a codebook
        metric is enabled.  Violations raise ``ValueError`` before any device work.  After the call ``last_per_image`` is the batch's float64
        [B, 3] device tensor of sum |d|, sum d^2 and sum SSIM per image (zeros for a metric that is not enabled)."""
        if real_images.dim() != 4 or fake_images.dim() != 4:
            raise ValueError(f"update expects [B, C, H, W] images, got {tuple(real_images.shape)} and {tuple(fake_images.shape)}")
        if real_images.numel() != fake_images.numel():
            raise ValueError(f"real and fake images differ in size: {tuple(real_images.shape)} vs {tuple(fake_images.shape)}")
        B, C, H, W = (int(v) for v in fake_images.shape)
        if B < 1 or C < 1:
            raise ValueError(f"empty batch: {tuple(fake_images.shape)}")
        if H < 6 or W < 6:
            raise ValueError(f"images of {H} x {W}: the 11 x 11 window's reflect padding needs H, W >= 6")
        if self._enable_ssim_score and C != 3:
            raise ValueError(f"SSIM takes 3 channels (evaluator.py:298), got {C}")
        if self._codebook and codebook_indices is None:
            raise ValueError("codebook_indices is required when a codebook metric is enabled")
        if self._codebook and (codebook_indices.is_floating_point() or codebook_indices.is_complex()):
            raise ValueError(f"codebook_indices must be an integer tensor, got {codebook_indices.dtype}")
        attached = [row for row in self._pair_losses if row.model is not None]
        for row in attached:
            row.model.check_images(tuple(fake_images.shape), tuple(fake_images.shape))         # sizes the engine does not take: ValueError, no device work
        if self._disc is not None:
            self._disc.check_images(tuple(fake_images.shape))
        lib = _lib.load()
        need = int(lib.mb_eval_workspace_bytes(B, C, H, W)) if self._metrics else 0
        if self._metrics and need == 0:
            raise ValueError(f"batch of {tuple(fake_images.shape)} is outside what mb_eval_images takes (B, C <= 65535)")
        self._num_examples += B
        self._num_updates += 1
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream().cuda_stream
            if self._metrics:
                fake = fake_images.to(device=self._device, dtype=torch.float32).contiguous()
                real = real_images.to(device=self._device, dtype=torch.float32).reshape(fake.shape).contiguous()
                if self._workspace is None or self._workspace.numel() * 8 < need:
                    self._workspace = torch.empty(need // 8, dtype=torch.float64, device=self._device)
                per_image = torch.empty((B, 3), dtype=torch.float64, device=self._device)
                _lib.check(lib.mb_eval_images(real.data_ptr(), fake.data_ptr(), B, C, H, W, self._metrics, 1 if clamp else 0,
                                              self._workspace.data_ptr(), per_image.data_ptr(), self._sums.data_ptr(), stream), "mb_eval_images")
                self.last_per_image = per_image
            if self._inception is not None:                                                      # evaluator.py:336-364
                images = (fake_images, real_images.reshape(fake_images.shape))
                if clamp:
                    images = tuple(v.clamp(0.0, 1.0) for v in images)
                pool_fake, logits_fake = extract(self._inception, to_uint8(images[0]), self._rfid, self._inception_score)
                if self._inception_score:
                    self._is_stats.add(logits_fake)
                if self._rfid:
                    pool_real, _ = extract(self._inception, to_uint8(images[1]), True, False)
                    if tuple(pool_real.shape) != tuple(pool_fake.shape):
                        raise ValueError(f"features of the real images {tuple(pool_real.shape)} and of the fake ones {tuple(pool_fake.shape)} differ")
                    self._rfid_real.add(pool_real)
                    self._rfid_fake.add(pool_fake)
            for row in attached:                                                                # evaluator.py:366-368
                row.last = row.model._run(real_images.reshape(fake_images.shape), fake_images, clamp, row.sum)
            if self._disc is not None:
                self._disc.logit_stats(real_images.reshape(fake_images.shape), clamp, self._disc_sums[0])
                self._disc.logit_stats(fake_images, clamp, self._disc_sums[1])
            if self._codebook:
                idx = codebook_indices.to(device=self._device, dtype=torch.int64).contiguous()
                _lib.check(lib.mb_eval_codebook(idx.data_ptr(), idx.numel(), self._num_codebook_entries, self._hist.data_ptr(),
                                                self._out_of_range.data_ptr(), stream), "mb_eval_codebook")

    def result(self) -> Mapping[Text, torch.Tensor]:
        """The averages over all images given, keys and order of evaluator.py:385-466: Python floats, except ``CodebookEntropy``, a 0-d float64
        tensor on the evaluator's device as in the reference.  One device-to-host copy.  ``IndexError`` if an index fell outside
        [0, num_codebook_entries)."""
        if self._num_examples < 1:
            raise ValueError("No examples to evaluate.")
        entropy = None
        attached = [row for row in self._pair_losses if row.model is not None]
        parts = [self._sums] + [row.sum for row in attached]
        cb = 4 + len(attached)                                                                  # position of the codebook figures
        if self._codebook:
            counts = self._hist.double()
            probs = counts / counts.sum()
            entropy = (-torch.log2(probs + 1e-8) * probs).sum()                                # evaluator.py:462-463
            parts += [(self._hist != 0).sum().double().reshape(1), (self._out_of_range.long() & 0xFFFFFFFF).double()]
        if (self._inception_score and self._is_stats.width is None) or (self._rfid and self._rfid_real.width is None):
            raise ValueError("use_inception() was called after the updates of this pass: attach the extractor first, or reset_metrics()")
        at = sum(int(p.numel()) for p in parts)                                                # where the Inception statistics begin
        if self._inception_score:
            parts.append(self._is_stats.sums.reshape(-1))
        if self._rfid:
            for stats in (self._rfid_real, self._rfid_fake):
                parts += [stats.total, stats.full_sigma().reshape(-1)]
        at_disc = sum(int(p.numel()) for p in parts)                                           # where the discriminator's sums begin
        if self._disc is not None:
            parts.append(self._disc_sums.reshape(-1))
        host = torch.cat(parts).cpu()                                                           # the one copy
        if self._codebook and host[cb + 1] != 0:
            raise IndexError(f"{int(host[cb + 1])} codebook indices outside [0, {self._num_codebook_entries})")
        eval_score = {}
        n = self._num_examples
        if self._enable_mae_error:
            eval_score["MAE"] = host[0].item() / n
        if self._enable_mse_error:
            eval_score["MSE"] = host[1].item() / n
        if self._enable_psnr_score:
            eval_score["PSNR"] = host[2].item() / n
        if self._enable_ssim_score:
            eval_score["SSIM"] = host[3].item() / n
        if self._inception_score:                                                               # evaluator.py:406-415
            C = self._is_stats.width
            eval_score["InceptionScore"] = inception_score(host[at:at + C], host[at + C:at + 2 * C], n)
            at += 2 * C
        if self._rfid:                                                                          # evaluator.py:417-451
            D = self._rfid_real.width
            (t_real, s_real), (t_fake, s_fake) = ((host[o:o + D], host[o + D:o + D + D * D].reshape(D, D)) for o in (at, at + D + D * D))
            eval_score["rFID"] = frechet_distance(t_real / n, get_covariance(s_real, t_real, n), t_fake / n, get_covariance(s_fake, t_fake, n))
        for i, row in enumerate(attached):
            eval_score[row.key] = host[4 + i].item() / n                                        # evaluator.py:453-455
        if self._disc is not None:
            from .discriminator import D_LOSSES, G_LOSSES, logits_mean
            stats = host[at_disc:at_disc + 10].reshape(2, 5) / n                                  # the sums of the average image
            real, fake = stats[0:1], stats[1:2]
            eval_score["LogitsReal"], eval_score["LogitsFake"] = logits_mean(real).item(), logits_mean(fake).item()
            eval_score["DiscriminatorLoss"] = D_LOSSES[self._disc_loss](real, fake).item()
            eval_score["GeneratorLoss"] = G_LOSSES[self._disc_loss](fake).item()
        if self._enable_codebook_usage_measure:
            eval_score["CodebookUsage"] = float(int(host[cb])) / self._num_codebook_entries
        if self._enable_codebook_entropy_measure:
            eval_score["CodebookEntropy"] = entropy
        return eval_score
