"""``sample()``: the MaskBit N-step masked bit-token sampler + decode, on the gfx950 engine.

Drop-in for the reference's ``modeling.modules.sample`` (sampling.py:13-136): same signature,
same return value ``(image [B,3,H,W] float32 unclamped on model.device, [pred tokens per step])``,
same random-number protocol -- per step one ``exponential_`` of shape [B*n*m, C] from the model
device's generator (what ``Categorical.sample`` -> ``torch.multinomial(n=1)`` draws) and one
``Gumbel(0,1).sample([B,n,m])`` from the CPU default generator -- so a fixed seed draws the same
noise the reference would on the same device.  The schedule (guidance scale, temperature, mask
length per step) is evaluated here on the host with the reference's float32 torch-scalar
arithmetic and handed to ``mb_sample`` as a plan; the loop body itself (2B-sequence forward, CFG
combine, softmax, draw, confidence, k-th-smallest re-mask, combine, decode) never leaves the GPU.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence, Text, Tuple

import torch

from . import _lib
from .bert import LFQBert
from .conv_vqgan import ConvVQModel
from .masking import get_masking_ratio
from .taming_vqgan import OriginalVQModel
from .parallel import slice_noise


def _scale_temperature(i: int, num_steps: int, guidance_scale: float, guidance_annealing: str, scale_pow: float, softmax_temperature: float,
                       use_sampling_annealing: bool):
    """Guidance scale and softmax temperature of step ``i`` (sampling.py:82, 90-98, 103-104)."""
    progress = (i + 1) / num_steps
    if guidance_annealing == "none":
        a = guidance_scale * 1.0
    elif guidance_annealing == "linear":
        a = guidance_scale * (i / num_steps)
    elif guidance_annealing == "cosine":
        sp = torch.ones(1) * scale_pow                                      # float32, as in the reference
        a = float(guidance_scale * ((1 - torch.cos(((i / num_steps) ** sp) * torch.pi)) * 1 / 2))
    else:
        raise ValueError(f"guidance_annealing must be 'none', 'linear' or 'cosine', got {guidance_annealing!r}")
    return float(torch.tensor(a, dtype=torch.float32)), (0.5 + 0.8 * (1 - progress) if use_sampling_annealing else softmax_temperature)


class Plan(tuple):
    """The per-step constants of a run: unpacks and indexes as ``(scale, temperature, third)``, three sequences of ``num_steps``.  ``third`` holds the
    integer mask lengths ``mb_sample`` reads, or with ``edit`` the float32 masking ratios of a run that re-masks by the per-sample rule
    (``mb_sample_edit``, ``mb_sample_seeded``).  ``force_guidance``: the CFG forward runs although every annealed scale is 0 (``forced_guidance``).
    ``use_cfg`` and ``arrays`` -- the ctypes arrays the C entries read (+ ``use_cfg``) -- are computed once, here."""

    def __new__(cls, scale, temperature, third, edit: bool = False, force_guidance: bool = False):
        self = super().__new__(cls, (scale, temperature, third))
        self.edit, self.force_guidance = edit, force_guidance
        self.use_cfg = force_guidance or any(s != 0.0 for s in scale)
        nsteps = len(scale)
        self.arrays = ((C.c_float * nsteps)(*scale), (C.c_float * nsteps)(*temperature), ((C.c_float if edit else C.c_int) * nsteps)(*third), self.use_cfg)
        return self


def build_plan(num_steps: int, num_maskable: Optional[int], guidance_scale: float, guidance_annealing: str, scale_pow: float,
               softmax_temperature: float, use_sampling_annealing: bool, mask_schedule_strategy: str) -> Plan:
    """Host-side per-step constants (sampling.py:82, 90-98, 103-104, 120-123): (scale, temperature, mask_len).  ``num_maskable`` None: the edit plan
    (``build_edit_plan``), with the masking ratios themselves in the third column."""
    get_masking_ratio(1.0, mask_schedule_strategy)          # raises ValueError on a bad strategy before any GPU work
    scale, temp, third = [], [], []
    for i in range(num_steps):
        a, t = _scale_temperature(i, num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing)
        scale.append(a)
        temp.append(t)
        ratio = get_masking_ratio((i + 1) / num_steps, mask_schedule_strategy)
        third.append(float(ratio) if num_maskable is None else int(torch.floor(ratio * num_maskable)))
    return Plan(scale, temp, third, edit=num_maskable is None)


def build_edit_plan(num_steps: int, guidance_scale: float, guidance_annealing: str, scale_pow: float, softmax_temperature: float,
                    use_sampling_annealing: bool, mask_schedule_strategy: str) -> Plan:
    """``build_plan`` for an edit run: the same scales and temperatures, and in the place of the mask lengths the float32 masking ratios themselves
    -- the device multiplies each by the sample's own initial masked count (``floor(ratio * M_b)`` in fp32, as ``torch.floor(ratio * num_maskable)``)."""
    return build_plan(num_steps, None, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy)


def forced_guidance(plan: Plan, guidance_scale: float) -> Plan:
    """The plan the public entries run: as in the reference's ``sample()``, the CFG forward still runs when ``guidance_scale != 0`` but every annealed
    scale happens to be 0.  (Not applied by ``build_plan`` / ``build_edit_plan``: a plan built directly runs what its scales say.)"""
    if guidance_scale != 0.0 and not plan.use_cfg:
        return Plan(*plan, edit=plan.edit, force_guidance=True)
    return plan


def seeded_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy) -> Plan:
    """The plan of a seeded or an edit run as the public entries build it: ``build_edit_plan`` (per-sample masking ratios) under ``forced_guidance``."""
    return forced_guidance(build_edit_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing,
                                           mask_schedule_strategy), guidance_scale)


def plan_arrays(plan: Plan):
    """The plan as the ctypes arrays ``mb_sample`` reads (+ whether any step is guided); of an edit plan, those ``mb_sample_edit`` reads."""
    return plan.arrays


def check_tokenizer(model, vqgan_model) -> None:
    """A lookup (VQ) tokenizer must hold every code the generator can emit: 2**model.bits <= codebook_size (the reference would fail in the
    codebook's nn.Embedding, quantizer.py:115).  Raised before any device work.  LFQ tokenizers are not checked (unchanged path)."""
    if getattr(vqgan_model, "quantizer_type", None) == "lookup" and vqgan_model.codebook_size < 2 ** model.bits:
        raise ValueError(f"the tokenizer's codebook holds {vqgan_model.codebook_size} entries, the generator emits codes up to 2**{model.bits}")


def check_models(model, vqgan_model, what: str) -> None:
    """``what()`` runs on this package's own models (there is no fall-back for others), and the tokenizer holds the generator's codes."""
    if not isinstance(model, LFQBert):
        raise TypeError(f"{what}() needs a maskbit_amd LFQBert generator, got {type(model).__name__}")
    if isinstance(vqgan_model, OriginalVQModel):
        raise TypeError(f"{what}() does not take the Taming VQGAN tokenizer (OriginalVQModel): the sampling loop decodes through a ConvVQModel engine, "
                        "and the reference pairs no generator with this tokenizer")
    if not isinstance(vqgan_model, ConvVQModel):
        raise TypeError(f"{what}() needs a maskbit_amd ConvVQModel tokenizer, got {type(vqgan_model).__name__}")
    check_tokenizer(model, vqgan_model)


NOISE_CHUNK_BYTES = 1 << 30       # sample() / generate_uint8() draw and feed the Exp(1) noise in step chunks of at most this size
OVERLAP_CHUNKS = 8                # ... and in at least this many chunks (+ a one-step head): the host draws chunk k+1 while the device runs chunk k


class _DrawThread:
    """The host-side draws are a few small CPU tensor ops per step.  With the default intra-op pool of a many-core host (128 OpenMP / MKL threads on the
    256-CPU MI355X boxes) every such op wakes the pool, whose workers then spin -- and the HIP runtime's own host threads starve: measured on BASELINE
    configs[1] (16 steps, batch 16) 182-189 ms per run against 118 ms with the draws at one thread (tools/host_draw_ab.py; a `log` over 8 192 values takes
    2.7 ms there: MKL's vector math threads by itself, so drawing in pieces below ATen's own parallel grain does not help -- round 6 tried).
    Rounds 3-5 flipped ``torch.set_num_threads`` to 1 around every draw ON THE CALLING THREAD: the caller's own setting changed under it, per draw.  Now the
    draws run on ONE dedicated worker thread whose OWN intra-op thread count is 1 (OpenMP's and MKL's thread counts are per-thread settings); the caller
    blocks until its draws are done, so the order in which a run consumes the process-global default CPU generator is the caller's program order.  ATen
    also remembers the last value ANY thread set as the default for threads created later, so the worker's one-time 1 is followed, once, by the caller
    re-asserting the count it already has: after that no draw touches any thread setting."""
    _pool = None

    @classmethod
    def run(cls, fn):
        if cls._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            n = torch.get_num_threads()
            pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="maskbit-draw")
            # (get first: ATen initialises a thread's count lazily, from the last value set anywhere, on its first intra-op call -- that must not come later)
            pool.submit(lambda: (torch.get_num_threads(), torch.set_num_threads(1))).result()          # the worker's own setting ...
            torch.set_num_threads(n)                                # ... and the default new threads inherit is the caller's again (its own count is n already)
            cls._pool = pool
        return cls._pool.submit(fn).result()


def _draw_conf(gumbel, num_samples: int, n: int, m: int, steps, num_steps: int, randomize_temperature: float) -> torch.Tensor:
    """The reference's per-step confidence noise (sampling.py:113-117): one ``Gumbel(0, 1).sample([B, n, m])`` from the CPU default generator per step,
    scaled by randomize_temperature * (1 - progress) (in the reference's order of the two products)."""
    return torch.stack([gumbel.sample((num_samples, n, m)) * randomize_temperature * (1 - (i + 1) / num_steps) for i in steps])


_COPY_STREAMS = {}


def _to_device_early(cpu: torch.Tensor, device) -> torch.Tensor:
    """Host -> device copy of a chunk's confidence noise that neither holds the host nor sits in the launch stream's order.  A pageable-memory copy
    (``.to(device)``) holds the HOST until the device has run everything enqueued before it -- the whole previous step chunk -- and the device then
    idles while the host enqueues this chunk (BASELINE configs[1] at batch 16: eight gaps of 0.4-0.9 ms per 126 ms run, tools/launch_gaps.py); a pinned
    asynchronous copy IN the launch stream still puts its own latency (0.1-0.3 ms through the copy engine) between two chunks.  So: pinned staging, the
    copy on a side stream (it runs while the previous chunk computes), the launch stream waits for its event; the pinned block and the device
    block are kept alive by torch's allocators (non_blocking copy / record_stream).  Same-box A/B, ms per run of configs[1]: batch 16 pageable 124.2,
    pinned in-stream 121.7, side stream 121.4; batch 64 332 / 330 / 328.5."""
    device = torch.device(device)
    if device.type != "cuda":
        return cpu.to(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    main = torch.cuda.current_stream(idx)
    side = _COPY_STREAMS.get(idx)
    if side is None:
        side = _COPY_STREAMS[idx] = torch.cuda.Stream(idx)
    with torch.cuda.stream(side):
        out = cpu.pin_memory().to(device, non_blocking=True)
    main.wait_stream(side)
    out.record_stream(main)
    return out


def draw_noise(num_samples: int, n: int, m: int, C_: int, num_steps: int, randomize_temperature: float,
               device: torch.device, step_begin: int = 0, step_end: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Noise for steps [step_begin, step_end) of a run (default: the whole run), drawn in the reference's per-generator order: consecutive
    chunks consume the generators exactly as one whole-run draw does.
    Returns exp_noise [steps, B*n*m, C] (device) and conf_noise [steps, B, n, m] (device) where
    conf_noise = gumbel * randomize_temperature * (1 - progress) (sampling.py:117)."""
    step_end = num_steps if step_end is None else step_end
    exp_noise = torch.empty((step_end - step_begin, num_samples * n * m, C_), dtype=torch.float32, device=device)
    for i in range(step_end - step_begin):
        exp_noise[i].exponential_(1)
    gumbel = torch.distributions.Gumbel(loc=0.0, scale=1.0)                     # python-float params => CPU draws
    conf = _DrawThread.run(lambda: _draw_conf(gumbel, num_samples, n, m, range(step_begin, step_end), num_steps, randomize_temperature))
    return exp_noise, _to_device_early(conf, device)


def step_chunks(num_samples: int, n: int, m: int, C_: int, num_steps: int):
    """[(begin, end)] such that one chunk's Exp(1) noise stays under NOISE_CHUNK_BYTES (the reference holds one step at a time; a whole
    256-step run at batch 100 would be 6.7 GB) and that the run has a one-step head followed by >= OVERLAP_CHUNKS chunks: ``mb_sample`` only
    enqueues work, so the host-side draws of a chunk (the reference's CPU Gumbel noise: ~1.5 ms per step at batch 64, 100 ms per 64-step run
    when drawn up front) run while the device is busy with the previous chunk -- only the head's draw is exposed."""
    per_step = num_samples * n * m * C_ * 4
    k = max(1, min(num_steps, NOISE_CHUNK_BYTES // max(per_step, 1)))
    if OVERLAP_CHUNKS > 1 and num_steps > 1:
        k = max(1, min(k, -(-(num_steps - 1) // OVERLAP_CHUNKS)))
        return [(0, 1)] + [(b, min(b + k, num_steps)) for b in range(1, num_steps, k)]
    return [(b, min(b + k, num_steps)) for b in range(0, num_steps, k)]


def run_chunked(model: "LFQBert", vqgan_model, labels: torch.Tensor, plan: Plan, randomize_temperature: float, *, seeds: Optional[torch.Tensor] = None,
                noise_rows: Optional[Tuple[int, int, int]] = None, **kw):
    """A whole run -> what ``run_loop`` returns.  The noise is drawn chunk by chunk (same random streams as one whole-run draw), each chunk one ``run_loop``
    call; an edit plan with ``init_tokens=`` runs the edit loop: same draws, same chunks.
    ``seeds`` (what ``check_seeds`` returns): one ``run_seeded`` call instead -- no chunks, nothing drawn.
    ``noise_rows`` = (nb, lo, hi): the noise is drawn for ``nb`` samples and the run is fed the rows of samples [lo, hi) (``parallel.slice_noise``) --
    ``labels`` are those samples'; lo == hi: the draws alone (-> four Nones), which keep the generators in step with the callers that have samples."""
    if seeds is not None:
        return run_seeded(model, vqgan_model, labels, plan, seeds, randomize_temperature, **kw)
    steps = len(plan[0])
    n, m, C_ = model.seq_len, model.splits, model.effective_codebook_size
    nb, lo, hi = noise_rows if noise_rows is not None else (labels.shape[0], 0, labels.shape[0])
    chunks = step_chunks(nb, n, m, C_, steps)
    parts, out = [], (None, None, None, None)
    for (b0, b1) in chunks:
        e, c = draw_noise(nb, n, m, C_, steps, randomize_temperature, model.device, b0, b1)
        if noise_rows is not None:
            if lo == hi:
                continue
            e, c = slice_noise(e, c, lo, hi, n * m)
        out = run_loop(model, vqgan_model, labels, plan, e, c, step_range=(b0, b1) if len(chunks) > 1 else None, **kw)
        parts.append(out[2])
    if len(parts) > 1 and parts[0] is not None:
        out = out[0], out[1], torch.cat(parts), out[3]
    return out


def _run(model: LFQBert, vqgan_model: Optional[ConvVQModel], labels: torch.Tensor, plan: Plan, want_steps: bool, want_image: bool, want_u8: bool,
         step_range: Optional[Tuple[int, int]], init_tokens: Optional[torch.Tensor], noise=None, seeded=None):
    """One call of a run entry, for ``run_loop`` (``noise`` = (exp_noise, conf_noise) of the step range: ``mb_sample``, or ``mb_sample_edit`` with an edit
    plan) and ``run_seeded`` (``seeded`` = (seeds, randomize_temperature): ``mb_sample_seeded``)."""
    dev = model._require_cuda("sample" if seeded is None else "sample_seeded")
    nsteps = len(plan[0])
    sb, se = step_range if step_range is not None else (0, nsteps)
    steps = se - sb
    B = labels.shape[0]
    n, m = model.seq_len, model.splits
    if seeded is None:
        exp_noise, conf_noise = noise
        if exp_noise.shape[0] != steps or conf_noise.shape[0] != steps:
            raise ValueError(f"noise holds {exp_noise.shape[0]} steps, the step range {steps}")
        if plan.edit != (init_tokens is not None):
            raise ValueError("an edit plan (build_edit_plan) and init_tokens go together")
    else:
        seeds, randomize_temperature = seeded
        if not plan.edit:
            raise ValueError("a seeded run takes an edit plan (build_edit_plan): it re-masks by the per-sample rule")
        if seeds.shape != (B,) or seeds.dtype != torch.int64:
            raise ValueError(f"seeds must be int64 [{B}]")
    if init_tokens is not None and (init_tokens.shape != (B, n, m) or init_tokens.dtype != torch.int64 or init_tokens.device.type != dev.type
                                    or not init_tokens.is_contiguous()):
        raise ValueError(f"init_tokens must be a contiguous int64 [{B}, {n}, {m}] tensor on {dev}")
    c_scale, c_temp, c_third, use_cfg = plan.arrays
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    ptr = lambda t: t.data_ptr() if t is not None else None
    if seeded is None:
        entry = "mb_sample_edit" if plan.edit else "mb_sample"
        source = ((init_tokens.data_ptr(),) if plan.edit else ()) + (exp_noise.data_ptr(), conf_noise.data_ptr())
    else:
        # (host-resident seeds: a pageable-memory copy would hold the host until the device has run everything enqueued before it -- the previous batch --
        # and the device then idles while this run is enqueued; pinned and asynchronous, as _to_device_early's)
        seeds = seeds.to(dev) if seeds.device.type != "cpu" else seeds.pin_memory().to(dev, non_blocking=True)
        conf_w = (C.c_float * nsteps)(*[1 - (i + 1) / nsteps for i in range(nsteps)])   # float32(1 - progress), sampling.py:117
        entry = "mb_sample_seeded"
        source = (ptr(init_tokens), seeds.data_ptr(), float(randomize_temperature), conf_w)
    step_tokens = torch.empty((steps, B, n, m), dtype=torch.int64, device=dev) if want_steps else None
    last = se == nsteps                                  # only the chunk that ends the run combines and decodes: earlier chunks need no outputs
    codes = torch.empty((B, n), dtype=torch.int64, device=dev) if last else None
    img = u8 = hdec = None
    if last and vqgan_model is not None and (want_image or want_u8):
        side = int(round(n ** 0.5))
        res = side << (vqgan_model.num_resolutions - 1)
        if want_image:
            img = torch.empty((B, vqgan_model.num_channels, res, res), dtype=torch.float32, device=dev)
        if want_u8:
            u8 = torch.empty((B, res, res, vqgan_model.num_channels), dtype=torch.uint8, device=dev)
        hdec = vqgan_model.engine(B, side)
    hgen = model.engine(2 * B if use_cfg else B)
    cplan = (_lib.EditPlan if plan.edit else _lib.SamplePlan)(nsteps, 1 if use_cfg else 0, c_scale, c_temp, c_third, sb if step_range is not None else 0,
                                                              se if step_range is not None else 0)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), entry)(hgen, hdec, C.byref(cplan), labels.data_ptr(), B, *source, ptr(step_tokens), ptr(codes), ptr(img), ptr(u8),
                                               torch.cuda.current_stream().cuda_stream), entry)
    return img, u8, step_tokens, codes


def run_loop(model: LFQBert, vqgan_model: Optional[ConvVQModel], labels: torch.Tensor, plan: Plan, exp_noise: torch.Tensor,
             conf_noise: torch.Tensor, want_steps: bool = True, want_image: bool = True, want_u8: bool = False,
             step_range: Optional[Tuple[int, int]] = None, init_tokens: Optional[torch.Tensor] = None):
    """One ``mb_sample`` call.  -> (image or None, uint8 NHWC or None, step tokens [steps,B,n,m] or None, codes [B,n]).
    ``init_tokens`` (int64 [B,n,m] on the model's device, ``model.mask_token`` at the slots to regenerate) with an edit plan: one ``mb_sample_edit``
    call -- the run starts from those tokens instead of the all-masked state (read by the chunk that starts the run).
    ``step_range`` = (begin, end): only those steps of the plan, with ``exp_noise`` / ``conf_noise`` holding that chunk's noise; chunk (0, e)
    starts the run, later chunks continue from the engine's token state, the chunk ending at the last step combines and decodes (image / codes
    are meaningful only then)."""
    return _run(model, vqgan_model, labels, plan, want_steps, want_image, want_u8, step_range, init_tokens, noise=(exp_noise, conf_noise))


def check_seeds(seeds, num_samples: int) -> torch.Tensor:
    """``seeds`` -- a length-``num_samples`` sequence of Python ints in [0, 2**64), or a one-dimensional int64 tensor holding those bit patterns -- as
    the int64 tensor ``mb_sample_seeded`` reads (a tensor stays on its device: nothing is copied or synchronised).  A wrong length, type or range
    raises ``ValueError``; no device is touched."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or seeds.dim() != 1:
            raise ValueError(f"a seeds tensor must be one-dimensional int64 (the bit patterns of the 64-bit seeds), got {seeds.dtype} {tuple(seeds.shape)}")
        if seeds.shape[0] != num_samples:
            raise ValueError(f"{seeds.shape[0]} seeds for {num_samples} samples")
        return seeds.detach().contiguous()
    try:
        seeds = list(seeds)
    except TypeError:
        raise ValueError(f"seeds must be a sequence of {num_samples} ints or an int64 tensor, got {type(seeds).__name__}") from None
    if len(seeds) != num_samples:
        raise ValueError(f"{len(seeds)} seeds for {num_samples} samples")
    out = []
    for v in seeds:
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"a seed must be an int in [0, 2**64), got {type(v).__name__}")
        if not 0 <= v < 1 << 64:
            raise ValueError(f"seed {v} outside [0, 2**64)")
        out.append(v - (1 << 64) if v >= 1 << 63 else v)
    return torch.tensor(out, dtype=torch.int64)


def run_seeded(model: LFQBert, vqgan_model: Optional[ConvVQModel], labels: torch.Tensor, plan: Plan, seeds: torch.Tensor, randomize_temperature: float,
               want_steps: bool = True, want_image: bool = True, want_u8: bool = False, step_range: Optional[Tuple[int, int]] = None,
               init_tokens: Optional[torch.Tensor] = None):
    """One ``mb_sample_seeded`` call: ``run_loop`` for an edit plan whose steps generate their own noise from ``seeds`` (int64 [B], what
    ``check_seeds`` returns).  No noise tensor exists, no generator is consumed, nothing is drawn on the host.  ``init_tokens`` None: the run starts
    all-masked.  -> (image or None, uint8 NHWC or None, step tokens or None, codes [B,n] or None), as ``run_loop``."""
    return _run(model, vqgan_model, labels, plan, want_steps, want_image, want_u8, step_range, init_tokens, seeded=(seeds, randomize_temperature))


@torch.no_grad()
def sample_seeded(
    model,
    vqgan_model,
    seeds,
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
) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """``sample()`` with per-sample seeds: sample ``b`` is generated for ``labels[b]`` from ``seeds[b]`` (a Python int in [0, 2**64), or the int64 bit
    pattern in a tensor), and its tokens and image depend on that seed, that label and the sampling arguments alone -- not on the batch size, its
    position in the batch or anything drawn before.  The step kernel computes its noise from (seed, step, slot, class) with a counter-based generator
    (include/maskbit_hip.h): no noise tensor is created, neither the CPU nor the device torch generator is consumed, and the whole run is one
    ``mb_sample_seeded`` call.  The samples are re-masked by the per-sample rule of the edit step.  Same return value as ``sample()``; the noise is
    NOT the reference's, so a seeded run does not reproduce a ``sample()`` run."""
    check_models(model, vqgan_model, "sample_seeded")
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels must be a tensor of class ids, got {type(labels).__name__}")
    seeds = check_seeds(seeds, int(labels.numel()))
    model._check_labels(labels)
    plan = seeded_plan(num_steps, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing, mask_schedule_strategy)
    model.eval()
    vqgan_model.eval()
    img, _, step_tokens, _ = run_chunked(model, vqgan_model, labels.reshape(-1), plan, randomize_temperature, seeds=seeds)
    return img, list(step_tokens.unbind(0))


@dataclasses.dataclass(frozen=True)
class SampleRequest:
    """One request of a ``sample_requests`` batch: its seed and label, and its own sampling arguments with the defaults of ``sample_seeded``."""
    seed: int
    label: int
    num_steps: int = 12
    guidance_scale: float = 3.0
    guidance_annealing: Text = "none"
    scale_pow: float = 4.0
    softmax_temperature: float = 1.0
    use_sampling_annealing: bool = False
    randomize_temperature: float = 4.5
    mask_schedule_strategy: Text = "linear"


REQUEST_COLUMNS = ("scale", "temperature", "mask_ratio", "randomize_temperature", "conf_weight", "step")   # mb_request_step, field for field


def build_request_plan(requests: Sequence[SampleRequest]):
    """The host side of a requests run (include/maskbit_hip.h "per-sample sampling arguments") -> ``(order, active, table)``; no device is touched.
    ``order``: the stable permutation that sorts the requests by ``num_steps`` descending (position p of the run holds ``requests[order[p]]``; ties keep
    request order).  ``active``: for each of the S = max ``num_steps`` global steps the number of requests that run it -- a prefix of the sorted batch,
    since request b is right-aligned: it runs its local step i = t - (S - N_b) at global step t >= S - N_b.  ``table``: int32 [S, B, 6], one
    ``mb_request_step`` record per (global step, position) in the order of ``REQUEST_COLUMNS`` -- the first five columns hold float32 BIT PATTERNS
    (``table.view(torch.float32)``): scale, temperature and masking ratio of local step i from ``seeded_plan`` of the request's settings, its
    randomize temperature, and float32(1 - (i + 1) / N_b); the sixth is i, the step's noise counter.  Inactive records are zero with step = -1.
    ``ValueError``: no requests, a ``num_steps`` below 1, an unknown annealing or schedule, a seed outside [0, 2**64)."""
    requests = list(requests)
    if not requests:
        raise ValueError("no requests")
    for r in requests:
        if not isinstance(r, SampleRequest):
            raise TypeError(f"a request must be a SampleRequest, got {type(r).__name__}")
        if isinstance(r.num_steps, bool) or not isinstance(r.num_steps, int) or r.num_steps < 1:
            raise ValueError(f"num_steps must be an int >= 1, got {r.num_steps!r}")
    check_seeds([r.seed for r in requests], len(requests))
    B, S = len(requests), max(r.num_steps for r in requests)
    order = sorted(range(B), key=lambda b: -requests[b].num_steps)            # (sorted is stable)
    table = torch.zeros((S, B, len(REQUEST_COLUMNS)), dtype=torch.int32)
    table[:, :, 5] = -1
    as_f32 = table.view(torch.float32)                                         # the same memory: the float columns are written through it
    columns = {}                                                               # one seeded_plan per distinct setting
    for p, b in enumerate(order):
        r = requests[b]
        N = r.num_steps
        key = (N, r.guidance_scale, r.guidance_annealing, r.scale_pow, r.softmax_temperature, r.use_sampling_annealing, r.mask_schedule_strategy)
        if key not in columns:
            scale, temp, ratio = seeded_plan(*key)
            conf_w = [1 - (i + 1) / N for i in range(N)]                       # float32(1 - progress) once stored: the expression of _run
            columns[key] = torch.tensor([scale, temp, ratio, conf_w], dtype=torch.float64).to(torch.float32).t()   # [N, 4]; one rounding, as ctypes' c_float
        col = columns[key]
        as_f32[S - N:, p, 0:3] = col[:, 0:3]
        as_f32[S - N:, p, 3] = float(r.randomize_temperature)
        as_f32[S - N:, p, 4] = col[:, 3]
        table[S - N:, p, 5] = torch.arange(N, dtype=torch.int32)
    active = [sum(1 for r in requests if r.num_steps >= S - t) for t in range(S)]
    return order, active, table


def run_requests(model: LFQBert, vqgan_model: Optional[ConvVQModel], requests: Sequence[SampleRequest], guided: Optional[bool] = None,
                 init_tokens: Optional[torch.Tensor] = None, want_image: bool = True, want_u8: bool = False):
    """One ``mb_sample_requests`` call (``run_seeded`` for requests) -> (image or None, uint8 NHWC or None -- both in REQUEST order --, step tokens
    [S, B, n, m] in the run's own order, of which only the active (t, position) are written, position [B]: request b ran at ``position[b]``).
    ``vqgan_model`` None: tokens only.  Arguments as ``sample_requests``; every check of the requests comes before any device work."""
    order, active, table = build_request_plan(requests)
    requests = list(requests)
    B, S = len(requests), len(active)
    any_scale = any(r.guidance_scale != 0.0 for r in requests)
    if guided is None:
        guided = any_scale
    elif not guided and any_scale:
        raise ValueError("guided=False, but a request has a non-zero guidance_scale")
    n, m = model.seq_len, model.splits
    labels = torch.tensor([int(requests[b].label) for b in order], dtype=torch.int64)
    model._check_labels(labels)
    if init_tokens is not None:
        if not isinstance(init_tokens, torch.Tensor) or init_tokens.dtype != torch.int64:
            raise TypeError("init_tokens must be an int64 tensor")
        if tuple(init_tokens.shape) != (B, n, m):
            raise ValueError(f"init_tokens must be [{B}, {n}, {m}], got {tuple(init_tokens.shape)}")
        if init_tokens.device.type == "cpu" and (int(init_tokens.min()) < 0 or int(init_tokens.max()) > model.mask_token):
            raise ValueError(f"token outside [0, {model.mask_token}] (mask_token = {model.mask_token} marks a slot to regenerate)")
    seeds = check_seeds([requests[b].seed for b in order], B)
    dev = model._require_cuda("sample_requests")
    identity = order == list(range(B))
    position = torch.empty(B, dtype=torch.int64)
    position[torch.tensor(order)] = torch.arange(B)                            # request b runs at position[b]
    # (every upload pinned and asynchronous, as _run uploads the seeds: a pageable copy would hold the host until the device has run the previous batch)
    up = lambda cpu: cpu.pin_memory().to(dev, non_blocking=True)
    with torch.cuda.device(dev):
        labels, seeds, table = up(labels), up(seeds), up(table)
        if not identity:
            order_dev, position_dev = up(torch.tensor(order)), up(position)
        if init_tokens is not None:
            init_tokens = init_tokens.to(dev) if init_tokens.device.type != "cpu" else up(init_tokens.contiguous())
            init_tokens = (init_tokens if identity else init_tokens[order_dev]).contiguous()
        step_tokens = torch.empty((S, B, n, m), dtype=torch.int64, device=dev)
        img = u8 = hdec = None
        if vqgan_model is not None and (want_image or want_u8):
            side = int(round(n ** 0.5))
            res = side << (vqgan_model.num_resolutions - 1)
            if want_image:
                img = torch.empty((B, vqgan_model.num_channels, res, res), dtype=torch.float32, device=dev)
            if want_u8:
                u8 = torch.empty((B, res, res, vqgan_model.num_channels), dtype=torch.uint8, device=dev)
            hdec = vqgan_model.engine(B, side)
        hgen = model.engine(2 * B if guided else B)
        cplan = _lib.RequestPlan(S, 1 if guided else 0, (C.c_int * S)(*active), table.data_ptr())
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(_lib.load().mb_sample_requests(hgen, hdec, C.byref(cplan), labels.data_ptr(), B, ptr(init_tokens), seeds.data_ptr(), step_tokens.data_ptr(),
                                                  None, ptr(img), ptr(u8), torch.cuda.current_stream().cuda_stream), "mb_sample_requests")
        if not identity:
            img, u8 = (None if t is None else t[position_dev] for t in (img, u8))
    return img, u8, step_tokens, position


def request_steps(requests: Sequence[SampleRequest], step_tokens: torch.Tensor, position: torch.Tensor) -> List[List[torch.Tensor]]:
    """Per request the list of its own ``num_steps`` step tokens [n, m], out of what ``run_requests`` returns (views: nothing is copied)."""
    S = step_tokens.shape[0]
    return [list(step_tokens[S - r.num_steps:, p].unbind(0)) for r, p in zip(requests, position.tolist())]


@torch.no_grad()
def sample_requests(model, vqgan_model, requests: Sequence[SampleRequest], *, guided: Optional[bool] = None, init_tokens: Optional[torch.Tensor] = None,
                    return_uint8: bool = False) -> Tuple[torch.Tensor, List[List[torch.Tensor]]]:
    """``sample_seeded`` for a batch of requests that each bring their own sampling arguments (``SampleRequest``): one ``mb_sample_requests`` call runs
    them together, each right-aligned in max ``num_steps`` global steps, at the cost of sum ``num_steps`` sequence-forwards.  A request's tokens and
    image depend on its own fields and on ``guided`` alone -- not on the other requests, its position or the batch size.
    ``guided``: one flag for the run.  None: guided if any request has a non-zero ``guidance_scale``; False with a non-zero scale raises; True forces
    the guided forward.  In a guided run EVERY step runs the guided forward (a zero scale gets ``c + 0 * (c - u)``) -- unlike ``sample_seeded``, which
    runs the plain forward on zero-scale steps below precision 4; the two agree where both run the same forwards.
    ``init_tokens`` int64 [B, n, m], in request order: each request starts from its own token map, as ``sample_from_tokens(seeds=)`` does.
    -> (images in REQUEST order: float32 [B, 3, H, W] unclamped, or with ``return_uint8`` uint8 [B, H, W, 3]; per request the list of its own
    ``num_steps`` step tokens [n, m]).  Nothing synchronises with the host, no torch generator is consumed."""
    check_models(model, vqgan_model, "sample_requests")
    requests = list(requests)
    model.eval()
    vqgan_model.eval()
    img, u8, step_tokens, position = run_requests(model, vqgan_model, requests, guided, init_tokens, want_image=not return_uint8, want_u8=return_uint8)
    return (u8 if return_uint8 else img), request_steps(requests, step_tokens, position)


@torch.no_grad()
def sample(
    model,
    vqgan_model,
    num_samples: int = 10,
    labels: Optional[torch.Tensor] = None,
    softmax_temperature: float = 1.0,
    randomize_temperature: float = 4.5,
    mask_schedule_strategy: Text = "linear",
    num_steps: int = 12,
    guidance_scale: float = 3.0,
    mask_token: int = 1024,
    patch_size: int = 16,
    guidance_annealing: Text = "none",
    use_sampling_annealing: bool = False,
    scale_pow: float = 4.0,
    codebook_size: int = 1024,
    codebook_splits: int = 1,
    use_tqdm: bool = False,
) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Generate ``num_samples`` class-conditional images.  See the module docstring; arguments as in the
    reference (sampling.py:32-54).  ``use_tqdm`` is accepted and ignored (the loop runs on the device)."""
    check_models(model, vqgan_model, "sample")
    device = model.device
    model.eval()
    vqgan_model.eval()
    n, m = int(patch_size ** 2), int(codebook_splits)
    if n != model.seq_len or m != model.splits:
        raise ValueError(f"patch_size/codebook_splits ({patch_size}, {m}) do not match the generator ({model.seq_len} tokens, {model.splits} groups)")
    if mask_token != model.mask_token:
        raise ValueError(f"mask_token={mask_token} but the generator masks with {model.mask_token} (= 2**(bits/splits))")
    if 2 ** model.bits != codebook_size:
        raise ValueError(f"codebook_size={codebook_size} does not match the generator's 2**{model.bits}")
    if labels is None:
        # goldfish, chicken, tiger cat, hourglass, ship, dog, race car, airliner, teddy bear, random (sampling.py:60-63)
        labels = torch.LongTensor([1, 7, 282, 604, 724, 179, 751, 404, 850, int(torch.randint(0, 999, size=(1,)))] * (num_samples // 10))
    model._check_labels(labels)
    labels = labels.to(device)
    if labels.numel() != num_samples:
        raise ValueError(f"{labels.numel()} labels for num_samples={num_samples}")
    plan = forced_guidance(build_plan(num_steps, n * m, guidance_scale, guidance_annealing, scale_pow, softmax_temperature, use_sampling_annealing,
                                      mask_schedule_strategy), guidance_scale)
    img, _, step_tokens, _ = run_chunked(model, vqgan_model, labels, plan, randomize_temperature)
    return img, list(step_tokens.unbind(0))
