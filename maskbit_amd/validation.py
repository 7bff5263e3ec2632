"""Masked-token validation of a generator checkpoint on the device: the forward half of the reference's training step
(scripts/train_maskbit.py:372-381) -- ``get_mask_tokens`` (modeling/modules/masking.py:7-38) and ``MLMLoss``
(modeling/modules/losses.py:289-339) -- behind the gfx950 kernels of ``csrc/mlm.hip``, plus ``MaskedTokenEvaluator``, which pools the same
figures over a whole validation set.

``get_mask_tokens`` draws on the host with the reference's random-number protocol (B schedule values, then one uniform per token slot, from
the CPU generator) and compares / selects in ``mb_mlm_mask``.  ``MLMLoss.forward`` and ``MaskedTokenEvaluator.update`` are ``mb_mlm_loss``:
one read of the logits for the label-smoothed cross entropy and the argmax accuracy over all rows and over the masked rows, fp32 per row,
fp64 sums in a fixed order, no host synchronisation (the reference's ``inputs[masks]`` is one).  Inference only: nothing here records
gradients.  There is no CPU path.
"""
from __future__ import annotations

import math
from typing import Mapping, Optional, Text, Tuple

import torch

from . import _lib

MASK_MODES = ("linear", "square", "cosine", "arccos")
STATE_WORDS = 37            # the pooled state of mb_mlm_loss (include/maskbit_hip.h): 2 sums, 4 counts, 10 x 3 deciles, out-of-range
KEYS = ("mlm_loss", "correct_tokens", "masked_token_loss", "masked_correct_tokens")


def mask_thresholds(batch: int, mode: Text = "arccos", min_masking_ratio: float = 0.0, *, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``val_to_mask`` float32 [batch] of masking.py:22-32: one ``torch.rand(batch)`` from the CPU generator (the global one when ``generator``
    is None) through the reference's float32 expressions."""
    if mode not in MASK_MODES:
        raise ValueError("Invalid mode. Choose between 'linear','square', 'cosine', 'arccos'.")
    r = torch.rand(batch, generator=generator) * (1 - min_masking_ratio)
    if mode == "linear":
        return 1 - r
    if mode == "square":
        return 1 - (r ** 2)
    if mode == "cosine":
        return torch.cos(r * math.pi * 0.5)
    return torch.acos(r) / (math.pi * 0.5)


def _require_device(t: torch.Tensor, what: str) -> torch.device:
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on an AMD GPU through libmaskbit_hip.so (tensor is on {t.device}); maskbit_amd has no CPU path.")
    return t.device


@torch.no_grad()
def get_mask_tokens(tokens: torch.Tensor, mask_token: int, mode: Text = "arccos", min_masking_ratio: float = 0.0, *,
                    generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (masked_tokens int64 like ``tokens``, mask bool like ``tokens``), masking.py:7-38: sample b is masked where a uniform draw lies
    below its ``val_to_mask`` (``mask_thresholds``).  The draws are the reference's -- ``torch.rand(B)`` then ``torch.rand(tokens.size())`` from
    the CPU generator, in that order -- so a seeded run masks the slots the reference masks; the uniforms reach the device through pinned
    memory, the compare and the select run in ``mb_mlm_mask``.  ``tokens`` [B, ...] is not modified."""
    if mode not in MASK_MODES:
        raise ValueError("Invalid mode. Choose between 'linear','square', 'cosine', 'arccos'.")
    dev = _require_device(tokens, "get_mask_tokens")
    if tokens.dim() < 1 or tokens.numel() == 0:
        raise ValueError(f"get_mask_tokens expects [B, ...] tokens, got {tuple(tokens.shape)}")
    lib = _lib.load()
    B = int(tokens.shape[0])
    val = mask_thresholds(B, mode, min_masking_ratio, generator=generator)
    uniforms = torch.rand(tokens.size(), generator=generator, pin_memory=True)
    toks = tokens.detach().to(torch.int64).contiguous()
    masked = torch.empty_like(toks)
    mask = torch.empty(toks.shape, dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        u = uniforms.to(dev, non_blocking=True)
        v = val.pin_memory().to(dev, non_blocking=True)
        _lib.check(lib.mb_mlm_mask(toks.data_ptr(), u.data_ptr(), v.data_ptr(), int(mask_token), masked.data_ptr(), mask.data_ptr(),
                                   B, toks.numel() // B, 1, torch.cuda.current_stream().cuda_stream), "mb_mlm_mask")
    return masked, mask


def _check_update(inputs: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor):
    if inputs.dim() != 4:
        raise ValueError(f"logits must be [b, n, m, codebook_size], got {tuple(inputs.shape)}")
    if tuple(targets.shape) != tuple(inputs.shape[:3]) or tuple(masks.shape) != tuple(inputs.shape[:3]):
        raise ValueError(f"targets and masks must be {tuple(inputs.shape[:3])}, got {tuple(targets.shape)} and {tuple(masks.shape)}")
    if targets.is_floating_point() or targets.is_complex():
        raise ValueError(f"targets must be an integer tensor, got {targets.dtype}")
    b, n, m, C = (int(v) for v in inputs.shape)
    if b < 1 or n < 1 or m < 1 or C < 2:
        raise ValueError(f"logits of {tuple(inputs.shape)}: b, n, m >= 1 and codebook_size >= 2")
    return b, n, m, C


def _run_loss(inputs, targets, masks, label_smoothing: float, state: Optional[torch.Tensor], workspace: Optional[torch.Tensor]):
    """One mb_mlm_loss call -> (sample_sums float64 [b, 2], sample_counts int64 [b, 3], workspace)."""
    b, n, m, C = _check_update(inputs, targets, masks)
    dev = _require_device(inputs, "MLMLoss")
    lib = _lib.load()
    need = int(lib.mb_mlm_workspace_bytes(b, n, m, C))
    if need == 0:
        raise ValueError(f"logits of {tuple(inputs.shape)} are outside what mb_mlm_loss takes (b <= 65535)")
    logits = inputs.detach().to(torch.float32)
    if not logits.is_contiguous():
        logits = logits.contiguous()
    tg = targets.to(device=dev, dtype=torch.int64).contiguous()
    mk = masks.to(device=dev)
    mk = (mk if mk.dtype in (torch.bool, torch.uint8) else mk != 0).contiguous()
    if workspace is None or workspace.numel() * 8 < need or workspace.device != dev:
        workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)
    sums = torch.empty((b, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((b, 3), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mb_mlm_loss(logits.data_ptr(), tg.data_ptr(), mk.data_ptr(), float(label_smoothing), b, n, m, C, workspace.data_ptr(),
                                   sums.data_ptr(), counts.data_ptr(), state.data_ptr() if state is not None else None,
                                   torch.cuda.current_stream().cuda_stream), "mb_mlm_loss")
    return sums, counts, workspace


def _new_state(dev: torch.device) -> torch.Tensor:
    assert int(_lib.load().mb_mlm_state_bytes()) == STATE_WORDS * 8
    return torch.zeros(STATE_WORDS, dtype=torch.int64, device=dev)


def _metrics(state: torch.Tensor, m: int, sum_splits: bool) -> Mapping[Text, torch.Tensor]:
    """The four figures of losses.py:320-337 from a pooled state, on the state's device: float64 quotients, rounded to float32 once.  No masked
    row: 0 / 0 = NaN, the reference's mean of an empty tensor."""
    sums = state[:2].view(torch.float64)
    rows, masked, correct, masked_correct = (state[2 + i].double() for i in range(4))
    scale = float(m) if sum_splits else 1.0
    return {
        "mlm_loss": (sums[0] / rows * scale).float(),
        "correct_tokens": ((correct / rows) ** m).float(),
        "masked_token_loss": (sums[1] / masked * scale).float(),
        "masked_correct_tokens": ((masked_correct / masked) ** m).float(),
    }


class MLMLoss(torch.nn.Module):
    """The reference's ``MLMLoss`` (losses.py:289-339) as one kernel.  INFERENCE ONLY: ``forward`` reads the logits' values and returns
    tensors without a gradient history -- this engine validates checkpoints, it does not train them."""

    def __init__(self, label_smoothing: float = 0.1, sum_splits: bool = False):
        super().__init__()
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing={label_smoothing}: a value in [0, 1] (torch.nn.CrossEntropyLoss)")
        self.label_smoothing = label_smoothing
        self.sum_splits = sum_splits
        self._workspace: Optional[torch.Tensor] = None

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor) -> Tuple[torch.Tensor, Mapping[Text, torch.Tensor]]:
        """``inputs`` [b, n, m, codebook_size] logits, ``targets`` [b, n, m] tokens, ``masks`` [b, n, m] bool -> (loss, loss_dict) with the
        keys ``mlm_loss``, ``correct_tokens`` (= (correct / rows) ** m), ``masked_token_loss``, ``masked_correct_tokens``: 0-d float32 tensors
        on the logits' device, enqueued on the current stream without a host synchronisation.  A target outside [0, codebook_size) leaves its
        row out (``MaskedTokenEvaluator.result`` raises on it; here nothing is read back)."""
        _check_update(inputs, targets, masks)
        state = _new_state(_require_device(inputs, "MLMLoss.forward"))
        _, _, self._workspace = _run_loss(inputs, targets, masks, self.label_smoothing, state, self._workspace)
        loss_dict = _metrics(state, int(inputs.shape[2]), self.sum_splits)
        return loss_dict["mlm_loss"], loss_dict


class MaskedTokenEvaluator:
    """``MLMLoss`` pooled over a validation set: ``update(logits, targets, masks)`` per batch (enqueued, never synchronises), ``result()`` at
    the end (one device-to-host copy).  The running state -- two float64 loss sums, the row counts, a table by mask-fraction decile, an
    out-of-range counter -- lives on the device of the first update; samples enter it in order, so the batching of a data set does not change a
    bit of the result."""

    def __init__(self, label_smoothing: float = 0.1, sum_splits: bool = False):
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing={label_smoothing}: a value in [0, 1] (torch.nn.CrossEntropyLoss)")
        self.label_smoothing = label_smoothing
        self.sum_splits = sum_splits
        self._state: Optional[torch.Tensor] = None
        self._workspace: Optional[torch.Tensor] = None
        self.reset_metrics()

    def reset_metrics(self):
        """Resets all metrics (the device state is zeroed by an enqueued fill; no synchronisation)."""
        self._num_examples = 0
        self._num_updates = 0
        self._splits = None
        if self._state is not None:
            self._state.zero_()
        self.last_sample_sums: Optional[torch.Tensor] = None
        self.last_sample_counts: Optional[torch.Tensor] = None

    @torch.no_grad()
    def update(self, logits: torch.Tensor, targets: torch.Tensor, masks: torch.Tensor):
        """Adds a batch: ``logits`` [b, n, m, codebook_size], ``targets`` / ``masks`` [b, n, m].  Afterwards ``last_sample_sums`` (float64
        [b, 2]: the sum of the row losses over all / over the masked rows of each sample) and ``last_sample_counts`` (int64 [b, 3]: correct
        rows, correct masked rows, masked rows) hold the batch's per-sample figures on the device."""
        b, n, m, C = _check_update(logits, targets, masks)
        dev = _require_device(logits, "MaskedTokenEvaluator.update")
        if self._splits is not None and self._splits != m:
            raise ValueError(f"updates of one evaluation must share the number of token groups: {self._splits} before, {m} now")
        if self._state is None or self._state.device != dev:
            if self._num_updates:
                raise ValueError(f"updates of one evaluation must stay on one device: {self._state.device} before, {dev} now")
            self._state = _new_state(dev)
        self.last_sample_sums, self.last_sample_counts, self._workspace = _run_loss(logits, targets, masks, self.label_smoothing, self._state,
                                                                                    self._workspace)
        self._splits = m
        self._num_examples += b
        self._num_updates += 1

    def result(self) -> Mapping[Text, object]:
        """Pooled over every row seen: the four keys of ``MLMLoss`` (0-d float32 tensors on the evaluator's device, computed exactly as
        ``MLMLoss.forward`` computes them); ``num_tokens`` / ``num_masked`` (int); ``by_mask_fraction`` float64 [10, 3] on the host -- per decile of
        the samples' realised mask fraction (row k: 10 * masked / (n * m) in [k, k + 1), the fully masked samples in row 9) the mean masked loss,
        the masked accuracy (NOT raised to m) and the number of masked rows, NaN where a decile saw none; ``sample_sums`` / ``sample_counts``:
        the per-sample figures of the last update (device tensors).  ``IndexError`` if a target fell outside [0, codebook_size)."""
        if self._num_examples < 1:
            raise ValueError("No examples to evaluate.")
        out = dict(_metrics(self._state, self._splits, self.sum_splits))
        host = self._state.cpu()                                                     # the one copy
        if int(host[36]) != 0:
            raise IndexError(f"{int(host[36])} targets outside [0, codebook_size)")
        out["num_tokens"] = int(host[2])
        out["num_masked"] = int(host[3])
        table = host[6:36].reshape(10, 3)
        loss, correct, rows = table[:, 0].contiguous().view(torch.float64), table[:, 1].double(), table[:, 2].double()
        scale = float(self._splits) if self.sum_splits else 1.0
        out["by_mask_fraction"] = torch.stack([loss / rows * scale, correct / rows, rows], dim=1)
        out["sample_sums"] = self.last_sample_sums
        out["sample_counts"] = self.last_sample_counts
        return out
