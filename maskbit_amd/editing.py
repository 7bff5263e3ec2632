"""Masked-token image editing: keep part of an image, regenerate the rest (inpainting, outpainting, a region under another class label).

The reference's ``sample()`` always starts from the all-masked state (sampling.py:65-71); a MaskGIT-family generator is just as much a model of
"some tokens given, predict the others".  ``sample_from_tokens`` starts the same N-step loop from any token map, ``inpaint`` wraps it for pixels:
encode -> pixel mask to token mask -> grouped tokens with the mask token at the cells to regenerate -> ``mb_sample_edit`` -> decode -> put the kept
pixels back.  Every stage is a kernel of libmaskbit_hip.so on the current stream; nothing synchronises with the host.

Per sample the loop follows the reference's schedule with that sample's own initial masked count ``M_b`` in the place of ``num_maskable`` and its
own current masked count in the clamp (the reference reads sample 0's for the whole batch, sampling.py:109 -- harmless when every sample starts
all-masked).  One deliberate departure: a sample with fewer than two masked slots is not re-masked (DESIGN.md "Editing").  With every slot masked
both functions draw the noise ``sample()`` draws and return what it returns, bit for bit.
"""
from __future__ import annotations

from typing import List, Text, Tuple

import torch

from . import _lib
from .sampling import build_edit_plan, check_models, check_seeds, run_chunked, seeded_plan

__all__ = ["sample_from_tokens", "inpaint", "build_edit_plan"]


def _check_edit_labels(model, labels, B: int) -> None:
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels must be a tensor of {B} class ids, got {type(labels).__name__}")
    if labels.numel() != B:
        raise ValueError(f"{labels.numel()} labels for {B} samples")
    model._check_labels(labels)


@torch.no_grad()
def sample_from_tokens(
    model,
    vqgan_model,
    init_tokens: torch.Tensor,
    labels: torch.Tensor,
    *,
    softmax_temperature: float = 1.0,
    randomize_temperature: float = 4.5,
    mask_schedule_strategy: Text = "linear",
    num_steps: int = 12,
    guidance_scale: float = 3.0,
    guidance_annealing: Text = "none",
    use_sampling_annealing: bool = False,
    scale_pow: float = 4.0,
    seeds=None,
) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """``sample()`` from a partly known token map: ``init_tokens`` int64 [B, n, m] holds ``model.mask_token`` at the slots to regenerate and a token
    in [0, mask_token) everywhere else; known slots come back unchanged in every step's prediction.  Same return value as ``sample()``
    -- ``(image [B,3,H,W] float32 unclamped, [pred tokens per step])`` -- and the same random-number protocol (a full [B*n*m, C] exponential and a
    [B, n, m] Gumbel draw per step, whatever the mask): with every slot masked the call equals ``sample()`` under the same seed.
    Host-resident tokens are range-checked; device-resident ones are clamped to [0, mask_token] on the device, with no host synchronisation.
    ``seeds`` (one per sample, as for ``sample_seeded``): the steps generate their noise from the seeds instead -- nothing is drawn, no generator is
    consumed, and with every slot masked the call equals ``sample_seeded``."""
    check_models(model, vqgan_model, "sample_from_tokens")
    n, m = model.seq_len, model.splits
    if not isinstance(init_tokens, torch.Tensor) or init_tokens.dtype != torch.int64:
        raise TypeError("init_tokens must be an int64 tensor")
    if init_tokens.dim() != 3 or tuple(init_tokens.shape[1:]) != (n, m):
        raise ValueError(f"init_tokens must be [B, {n}, {m}], got {tuple(init_tokens.shape)}")
    B = init_tokens.shape[0]
    if init_tokens.device.type == "cpu" and init_tokens.numel() and (int(init_tokens.min()) < 0 or int(init_tokens.max()) > model.mask_token):
        raise ValueError(f"token outside [0, {model.mask_token}] (mask_token = {model.mask_token} marks a slot to regenerate)")
    _check_edit_labels(model, labels, B)
    if seeds is not None:
        seeds = check_seeds(seeds, B)
    plan = seeded_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy)
    dev = model._require_cuda("sample_from_tokens")
    model.eval()
    vqgan_model.eval()
    tokens = init_tokens.to(dev).contiguous()
    img, _, step_tokens, _ = run_chunked(model, vqgan_model, labels.to(dev), plan, randomize_temperature, seeds=seeds, init_tokens=tokens)
    return img, list(step_tokens.unbind(0))


def _pixel_mask(regenerate, B: int, H: int, W: int) -> torch.Tensor:
    """The regeneration mask as [B, H, W] (a view where possible; bool and uint8 storage are both one byte per pixel)."""
    if not isinstance(regenerate, torch.Tensor) or regenerate.dtype not in (torch.bool, torch.uint8):
        raise TypeError("regenerate must be a bool or uint8 tensor (True / non-zero = regenerate the pixel)")
    if tuple(regenerate.shape) == (B, 1, H, W):
        regenerate = regenerate[:, 0]
    if tuple(regenerate.shape) != (B, H, W):
        raise ValueError(f"regenerate must be [{B}, {H}, {W}] or [{B}, 1, {H}, {W}], got {tuple(regenerate.shape)}")
    return regenerate


@torch.no_grad()
def inpaint(
    model,
    vqgan_model,
    images: torch.Tensor,
    regenerate: torch.Tensor,
    labels: torch.Tensor,
    *,
    keep_known_pixels: bool = True,
    return_uint8: bool = False,
    softmax_temperature: float = 1.0,
    randomize_temperature: float = 4.5,
    mask_schedule_strategy: Text = "linear",
    num_steps: int = 12,
    guidance_scale: float = 3.0,
    guidance_annealing: Text = "none",
    use_sampling_annealing: bool = False,
    scale_pow: float = 4.0,
    seeds=None,
):
    """Regenerate the pixels of ``images`` (float [B, C, H, W] in [0, 1]) where ``regenerate`` (bool or uint8 [B, H, W] or [B, 1, H, W]) is set,
    class-conditionally on ``labels``; the rest of the image is the context.  A token is regenerated when any pixel of its stride x stride block is.
    -> ``(image, codes int64 [B, n], token_mask bool [B, H/stride, W/stride])``; ``image`` is float32 NCHW (unclamped inside the mask, as ``sample()``
    returns it), or uint8 NHWC = trunc(clamp(x, 0, 1) * 255) with ``return_uint8``.  ``keep_known_pixels`` puts the input's own pixels back outside
    the mask (bit for bit); without it the image is the decoder's output for ``codes`` everywhere -- kept tokens reconstruct their region, they do not
    copy it.  ``seeds`` (one per sample, as for ``sample_seeded``): the steps generate their noise from the seeds instead of torch's generators."""
    check_models(model, vqgan_model, "inpaint")
    if vqgan_model.quantizer_type == "lookup" and vqgan_model.codebook_size != 2 ** model.bits:
        raise ValueError(f"the tokenizer's codebook holds {vqgan_model.codebook_size} entries, the generator reads codes of 2**{model.bits}: "
                         "an encoded image could hold codes the generator has no tokens for")
    if not isinstance(images, torch.Tensor) or not images.is_floating_point():
        raise TypeError("images must be a float tensor [B, C, H, W] with values in [0, 1]")
    stride = 1 << (vqgan_model.num_resolutions - 1)
    side = int(round(model.seq_len ** 0.5))
    if images.dim() != 4 or images.shape[1] != vqgan_model.num_channels or tuple(images.shape[2:]) != (side * stride, side * stride) \
            or side * side != model.seq_len:
        raise ValueError(f"images must be [B, {vqgan_model.num_channels}, {side * stride}, {side * stride}] for a generator of {model.seq_len} tokens "
                         f"and a tokenizer of stride {stride}, got {tuple(images.shape)}")
    B, ch, H, W = images.shape
    regenerate = _pixel_mask(regenerate, B, H, W)
    _check_edit_labels(model, labels, B)
    if seeds is not None:
        seeds = check_seeds(seeds, B)
    plan = seeded_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy)
    dev = model._require_cuda("inpaint")
    model.eval()
    vqgan_model.eval()
    n, m, C_ = model.seq_len, model.splits, model.effective_codebook_size
    lib = _lib.load()
    orig = images.to(device=dev, dtype=torch.float32).contiguous()
    pm = regenerate.to(dev).contiguous().view(torch.uint8)
    if orig.data_ptr() % 16:
        orig = orig.clone()                             # (a view into a larger tensor: the kernels read 16 bytes at a time)
    if pm.data_ptr() % 16:
        pm = pm.clone()
    _, idx, _ = vqgan_model._encode(orig)
    token_mask = torch.empty((B, side, side), dtype=torch.uint8, device=dev)
    tokens = torch.empty((B, n, m), dtype=torch.int64, device=dev)
    num_regen = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.mb_edit_token_mask(pm.data_ptr(), token_mask.data_ptr(), B, H, W, stride, stream), "mb_edit_token_mask")
        slot_mask = token_mask.reshape(B, n, 1).expand(B, n, m).contiguous()         # every group of a regenerated cell
        _lib.check(lib.mb_edit_init(idx.data_ptr(), slot_mask.data_ptr(), tokens.data_ptr(), num_regen.data_ptr(), B, n, m, C_, stream), "mb_edit_init")
    direct_u8 = return_uint8 and not keep_known_pixels                                # the decoder's own uint8 epilogue
    gen, u8, _, codes = run_chunked(model, vqgan_model, labels.to(dev), plan, randomize_temperature, seeds=seeds, init_tokens=tokens, want_steps=False,
                                    want_image=not direct_u8, want_u8=direct_u8)
    if keep_known_pixels:
        out = None if return_uint8 else torch.empty_like(gen)
        u8 = torch.empty((B, H, W, ch), dtype=torch.uint8, device=dev) if return_uint8 else None
        with torch.cuda.device(dev):
            _lib.check(lib.mb_edit_composite(gen.data_ptr(), orig.data_ptr(), pm.data_ptr(), out.data_ptr() if out is not None else None,
                                             u8.data_ptr() if u8 is not None else None, B, ch, H, W, torch.cuda.current_stream().cuda_stream),
                       "mb_edit_composite")
        gen = out
    return (u8 if return_uint8 else gen), codes, token_mask.bool()
