"""The generation loop of the reference's evaluation driver, kept on the device.

``scripts/eval_maskbit.py:103-137`` draws ``labels = randperm(1000).repeat(50)``, then per batch calls ``sample()``, clamps to
[0, 1], multiplies by 255, permutes to NHWC, casts to uint8 (truncating) and copies to the host -- one blocking copy of a
float image per batch.  Here the uint8 NHWC image is written by the decoder's last kernel (``mb_sample`` -> ``mb_dec_decode``'s
``img_nhwc_u8`` output), and the device-to-host copy of batch *i* runs on a side stream into pinned memory while batch *i+1*
is being sampled: the host only waits for a copy that has had a whole batch time to finish.

The random-number protocol per batch is that of ``sample()`` (``maskbit_amd/sampling.py``), so for a fixed seed the images equal
what a batch-by-batch ``sample()`` + the reference's post-processing gives (tested, bit for bit).
"""
from __future__ import annotations

import math
from typing import Iterator, Optional, Text

import numpy as np
import torch

from .bert import LFQBert
from .conv_vqgan import ConvVQModel
from .factorization import split_factorized_tokens
from .sampling import build_plan, check_models, check_seeds, check_tokenizer, forced_guidance, run_chunked, seeded_plan
from .validation import MaskedTokenEvaluator, get_mask_tokens


def eval_labels(device, nclass: int = 1000, repeats: int = 50) -> torch.Tensor:
    """``randperm(nclass).repeat(repeats)`` drawn on ``device`` (eval_maskbit.py:107-108): every batch of the run sees a class mix."""
    return torch.randperm(nclass, dtype=torch.int, device=device).repeat(repeats)


def mask_token_for(num_codebook_entries: int, codebook_splits: int) -> int:
    """``int(2 ** (log2(entries) // splits))`` (eval_maskbit.py:77,80)."""
    return int(2 ** (math.log2(num_codebook_entries) // codebook_splits))


def _device_batches(who: Text, model: LFQBert, vqgan_model: ConvVQModel, labels: torch.Tensor, batchsize: int, total_samples: Optional[int],
                    seed: Optional[int], softmax_temperature, randomize_temperature, mask_schedule_strategy, num_steps, guidance_scale,
                    guidance_annealing, use_sampling_annealing, scale_pow):
    """The checks and the plan of a generation run, then an iterator over its batches as DEVICE tensors ``(uint8 [batchsize, H, W, 3], codes int64
    [batchsize, n])``: the sampling loop of eval_maskbit.py:111-135 up to the decoder's uint8 output.  Nothing in it synchronises."""
    check_models(model, vqgan_model, who)
    total = int(labels.numel()) if total_samples is None else int(total_samples)
    nbatch = total // batchsize
    if nbatch * batchsize > labels.numel():
        raise ValueError(f"{labels.numel()} labels do not cover {nbatch} batches of {batchsize}")
    model._check_labels(labels)
    n, m = model.seq_len, model.splits
    run_seeds = None
    if seed is None:
        plan = forced_guidance(build_plan(num_steps, n * m, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing,
                                          mask_schedule_strategy), guidance_scale)
    else:
        check_seeds([seed], 1)
        run_seeds = check_seeds([(seed + j) % (1 << 64) for j in range(nbatch * batchsize)], nbatch * batchsize)
        plan = seeded_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy)
    dev = model._require_cuda(who)
    model.eval()
    vqgan_model.eval()
    if run_seeds is not None:
        run_seeds = run_seeds.to(dev)                   # one copy for the whole run

    def batches():
        for i in range(nbatch):
            y = labels[batchsize * i: batchsize * (i + 1)].long()
            seeds = run_seeds[batchsize * i: batchsize * (i + 1)] if run_seeds is not None else None
            _, u8, _, codes = run_chunked(model, vqgan_model, y, plan, randomize_temperature, seeds=seeds, want_steps=False, want_image=False,
                                          want_u8=True)
            yield u8, codes

    return batches()


@torch.no_grad()
def generate_uint8(model: LFQBert, vqgan_model: ConvVQModel, labels: torch.Tensor, batchsize: int, *,
                   softmax_temperature: float = 1.0, randomize_temperature: float = 4.5, mask_schedule_strategy: Text = "linear",
                   num_steps: int = 12, guidance_scale: float = 3.0, guidance_annealing: Text = "none",
                   use_sampling_annealing: bool = False, scale_pow: float = 4.0,
                   total_samples: Optional[int] = None, return_codes: bool = False, seed: Optional[int] = None) -> Iterator[np.ndarray]:
    """Yield ``total_samples // batchsize`` arrays ``uint8 [batchsize, H, W, 3]`` (host memory), batch *i* generated for
    ``labels[batchsize * i : batchsize * (i + 1)]`` exactly as eval_maskbit.py:111-135 does.  Each yielded array is a fresh copy
    (the reference appends them to a list).  ``return_codes=True`` yields ``(images, codes int64 [batchsize, n])`` -- the combined
    tokens each image was decoded from (what the reference's evaluator takes as ``codebook_indices``, evaluator.py:536).
    ``seed`` (an int in [0, 2**64)): seeded sampling (``sample_seeded``) -- image ``j`` of the run (global index) is generated from the seed
    ``(seed + j) mod 2**64``, so the images do not depend on ``batchsize`` and any one of them can be regenerated alone; torch's generators are not
    consumed."""
    batches = _device_batches("generate_uint8", model, vqgan_model, labels, batchsize, total_samples, seed, softmax_temperature, randomize_temperature,
                              mask_schedule_strategy, num_steps, guidance_scale, guidance_annealing, use_sampling_annealing, scale_pow)
    dev = model._require_cuda("generate_uint8")
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    pinned = [None, None]
    pending = None                                      # (slot, copy-done event) of the batch whose copy is in flight

    def collect(p):
        slot, done, codes = p
        done.synchronize()
        out = pinned[slot].numpy().copy()
        return (out, codes.cpu().numpy()) if return_codes else out

    for i, (u8, codes) in enumerate(batches):
        slot = i & 1
        if pinned[slot] is None or pinned[slot].shape != u8.shape:
            pinned[slot] = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            pinned[slot].copy_(u8, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        u8.record_stream(side)                           # the allocator must not hand the block out before the copy has read it
        if pending is not None:
            yield collect(pending)                       # batch i-1: its copy overlapped the sampling just enqueued
        pending = (slot, done, codes)
    if pending is not None:
        yield collect(pending)


def to_evaluator_uint8(u8_nhwc: torch.Tensor) -> torch.Tensor:
    """NHWC uint8 (the decoder epilogue's output) -> the NCHW uint8 tensor ``GeneratorEvaluator.update`` builds for its Inception
    network, ``(generated_images * 255).to(torch.uint8)`` on the clamped float image (evaluator/evaluator.py:549-551): the same
    bytes without materialising the float image.  A view, no copy."""
    return u8_nhwc.permute(0, 3, 1, 2)


@torch.no_grad()
def eval_generation(model: LFQBert, vqgan_model: ConvVQModel, evaluator, num_samples: int, batchsize: int, labels: Optional[torch.Tensor] = None, *,
                    softmax_temperature: float = 1.0, randomize_temperature: float = 4.5, mask_schedule_strategy: Text = "linear",
                    num_steps: int = 12, guidance_scale: float = 3.0, guidance_annealing: Text = "none",
                    use_sampling_annealing: bool = False, scale_pow: float = 4.0, seed: Optional[int] = None):
    """The generation loop of eval_maskbit.py:107-135 with a ``maskbit_amd.GeneratorEvaluator`` as the consumer: ``num_samples // batchsize``
    batches are sampled and decoded to device uint8 as in ``generate_uint8`` (same arguments, same images for the same ``seed``), and each goes
    straight into ``evaluator.update_uint8(to_evaluator_uint8(u8), codes)`` -- no float image, no copy to the host, nothing in the loop
    synchronises.  ``labels`` default to ``eval_labels`` over the model's classes, repeated to cover ``num_samples``.  The evaluator is reset
    first; returns ``evaluator.result()``."""
    if labels is None:
        dev = model._require_cuda("eval_generation")
        labels = eval_labels(dev, model.nclass, max(1, -(-int(num_samples) // model.nclass)))
    batches = _device_batches("eval_generation", model, vqgan_model, labels, batchsize, num_samples, seed, softmax_temperature, randomize_temperature,
                              mask_schedule_strategy, num_steps, guidance_scale, guidance_annealing, use_sampling_annealing, scale_pow)
    evaluator.reset_metrics()
    for u8, codes in batches:
        evaluator.update_uint8(to_evaluator_uint8(u8), codes)
    return evaluator.result()


@torch.no_grad()
def eval_reconstruction(model: ConvVQModel, loader, evaluator):
    """The reconstruction loop of the reference's tokenizer evaluation (scripts/eval_tokenizer.py:126-167, without the image dump): per batch
    ``model(images)``, then ``evaluator.update(original, reconstruction, min_encoding_indices)`` on both images clamped to [0, 1] -- the clamp
    runs inside the evaluator's kernel (``clamp=True``) instead of as two extra passes -- and ``evaluator.result()`` at the end.  ``loader``
    yields dicts with an ``"image"`` tensor [B, 3, H, W] as the reference's data loader does; ``evaluator`` is a
    ``maskbit_amd.TokenizerEvaluator``.  Nothing in the loop synchronises with the host."""
    dev = model._require_cuda("eval_reconstruction")
    model.eval()
    evaluator.reset_metrics()
    for batch in loader:
        images = batch["image"].to(dev, memory_format=torch.contiguous_format, non_blocking=True)
        reconstructed_images, model_dict = model(images)
        evaluator.update(images, reconstructed_images, model_dict["min_encoding_indices"], clamp=True)
    return evaluator.result()


@torch.no_grad()
def eval_masked_prediction(model: LFQBert, vqgan_model: ConvVQModel, loader, evaluator: Optional[MaskedTokenEvaluator] = None, *,
                           mask_schedule_strategy: Text = "arccos", min_masking_ratio: float = 0.0, class_label_dropout: float = 0.0,
                           generator: Optional[torch.Generator] = None):
    """The forward half of the reference's training step as a validation pass (scripts/train_maskbit.py:356-381, without gradients): per batch
    ``vqgan_model.encode(images)`` -> ``min_encoding_indices`` -> ``split_factorized_tokens`` -> ``get_mask_tokens`` with
    ``mask_token_for(codebook_size, splits)`` -> ``model(masked_tokens, class_ids, drop_label_mask)`` -> ``evaluator.update(logits, tokens,
    masks)``, and ``evaluator.result()`` at the end (the evaluator is reset first; a ``MaskedTokenEvaluator()`` with the reference's defaults when
    none is given).  ``loader`` yields dicts with ``"image"`` [B, 3, H, W] and ``"class_id"`` [B] as the reference's data loader does.  ``model``:
    ``LFQBert`` or ``Bert``; ``vqgan_model``: a lookup-free tokenizer whose codebook the generator was built for.

    Random numbers: the masks are drawn as ``get_mask_tokens`` documents (CPU generator: ``generator``, or the global one).  The label-drop mask
    is drawn only when ``class_label_dropout`` > 0, then as ``torch.rand(B) < class_label_dropout`` from the SAME CPU generator after the
    batch's masks -- the reference draws it with ``rand_like`` on the labels' device (train_maskbit.py:379), a stream this engine does not
    reproduce.  Nothing in the loop synchronises with the host."""
    if not isinstance(model, LFQBert) or not isinstance(vqgan_model, ConvVQModel):
        raise TypeError("eval_masked_prediction() needs a maskbit_amd generator and tokenizer")
    check_tokenizer(model, vqgan_model)
    dev = model._require_cuda("eval_masked_prediction")
    model.eval()
    vqgan_model.eval()
    if evaluator is None:
        evaluator = MaskedTokenEvaluator()
    evaluator.reset_metrics()
    codebook_size, splits = 2 ** model.bits, model.splits
    mask_token = mask_token_for(codebook_size, splits)
    for batch in loader:
        images = batch["image"].to(dev, memory_format=torch.contiguous_format, non_blocking=True)
        class_tokens = batch["class_id"].to(dev, non_blocking=True)
        _, encoder_dict = vqgan_model.encode(images)
        input_tokens = encoder_dict["min_encoding_indices"]
        input_tokens = split_factorized_tokens(input_tokens.reshape(input_tokens.shape[0], -1), codebook_size=codebook_size, splits=splits)
        masked_tokens, masks = get_mask_tokens(input_tokens, mask_token, mode=mask_schedule_strategy, min_masking_ratio=min_masking_ratio,
                                               generator=generator)
        drop_label_mask = None
        if class_label_dropout > 0:
            drop_label_mask = torch.rand(class_tokens.shape[0], generator=generator) < class_label_dropout
        logits = model(masked_tokens, class_tokens, drop_label_mask)
        evaluator.update(logits, input_tokens, masks)
    return evaluator.result()
