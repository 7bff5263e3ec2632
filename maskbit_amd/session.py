"""A sampling session: requests join and leave a running batch (include/maskbit_hip.h "sampling session").

``sample_requests`` runs a closed batch: planned for a fixed set of requests, busy for max ``num_steps`` steps.  A ``SamplingSession`` is the open
form for an interactive front end: ``submit`` queues a request at any time, every ``step`` admits what fits, runs ONE step for every active request
and returns the requests that finished with it.  A request's codes and image are bit for bit what ``sample_requests([request], guided=...)`` gives
for it alone, whatever else is in the session.

This module validates, queues and uploads; the rule that keeps the active requests a dense prefix lives in the library (kernels and the session
object's host mirror), not here."""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
from typing import Deque, Dict, List, Optional, Tuple

import torch

from . import _lib
from .bert import LFQBert
from .conv_vqgan import ConvVQModel
from .sampling import SampleRequest, build_request_plan, check_models


@dataclasses.dataclass(frozen=True)
class Finished:
    """A request that left the session: its ticket, the request, its codes int64 [n] and its image (float32 [3, H, W] unclamped, or with
    ``return_uint8`` uint8 [H, W, 3]; None without a tokenizer) -- device tensors, nothing has synchronised."""
    ticket: int
    request: SampleRequest
    codes: torch.Tensor
    image: Optional[torch.Tensor]


class SamplingSession:
    """``max_active`` rows, requests of at most ``max_steps`` steps, ONE ``guided`` flag (the ``sample_requests`` rule: in a guided session every step
    runs the guided forward and a zero scale gets ``c + 0 * (c - u)``; an unguided session refuses a non-zero scale).  ``vqgan_model`` None: codes only.
    Nothing touches the device before the first ``step()``."""

    def __init__(self, model: LFQBert, vqgan_model: Optional[ConvVQModel], max_active: int = 64, max_steps: int = 256, guided: bool = True,
                 return_uint8: bool = False):
        if vqgan_model is None:
            if not isinstance(model, LFQBert):
                raise TypeError(f"SamplingSession needs a maskbit_amd LFQBert generator, got {type(model).__name__}")
        else:
            check_models(model, vqgan_model, "SamplingSession")
        for name, v in (("max_active", max_active), ("max_steps", max_steps)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, got {v!r}")
        self.model, self.vqgan_model = model, vqgan_model
        self.max_active, self.max_steps, self.guided, self.return_uint8 = max_active, max_steps, bool(guided), bool(return_uint8)
        self.ticks = 0                                                     # steps that ran (a step of an empty session does not count)
        self._queue: Deque[Tuple[int, SampleRequest, torch.Tensor, Optional[torch.Tensor]]] = collections.deque()
        self._running: Dict[int, SampleRequest] = {}
        self._next_ticket = 0
        self._handle = None

    # ---- state -----------------------------------------------------------------------------------------------------------------------------
    @property
    def active(self) -> int:
        """Requests in the running batch (the library's count)."""
        return 0 if self._handle is None else int(_lib.load().mb_session_active(self._handle))

    @property
    def queued(self) -> int:
        """Requests submitted and not yet admitted."""
        return len(self._queue)

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _lib.load().mb_session_destroy(self._handle)
                self._handle = None
        except Exception:                                                      # (interpreter shutdown: the module may be gone already)
            pass

    # ---- submit ----------------------------------------------------------------------------------------------------------------------------
    def submit(self, request: SampleRequest, init_tokens: Optional[torch.Tensor] = None) -> int:
        """Queue ``request`` -> its ticket (0, 1, 2, ... in submission order, which is also the admission order).  ``init_tokens`` int64 [n, m]: the
        request starts from this token map (``model.mask_token`` at the slots to regenerate) instead of the all-masked state.  Raises before any
        device work: ``TypeError`` for a non-``SampleRequest`` or non-int64 tokens, ``ValueError`` for a bad field (``build_request_plan``),
        ``num_steps > max_steps``, a non-zero scale in an unguided session, tokens of the wrong shape or range; ``IndexError`` for a bad label."""
        _, _, table = build_request_plan([request])                        # validates the request; [N, 1, 6]: local step i of an N-step run
        if request.num_steps > self.max_steps:
            raise ValueError(f"num_steps = {request.num_steps} exceeds the session's max_steps = {self.max_steps}")
        if not self.guided and request.guidance_scale != 0.0:
            raise ValueError("guided=False, but the request has a non-zero guidance_scale")
        self.model._check_labels(torch.tensor([int(request.label)], dtype=torch.int64))
        n, m = self.model.seq_len, self.model.splits
        if init_tokens is not None:
            if not isinstance(init_tokens, torch.Tensor) or init_tokens.dtype != torch.int64:
                raise TypeError("init_tokens must be an int64 tensor")
            if tuple(init_tokens.shape) != (n, m):
                raise ValueError(f"init_tokens must be [{n}, {m}], got {tuple(init_tokens.shape)}")
            if init_tokens.device.type == "cpu" and (int(init_tokens.min()) < 0 or int(init_tokens.max()) > self.model.mask_token):
                raise ValueError(f"token outside [0, {self.model.mask_token}] (mask_token = {self.model.mask_token} marks a slot to regenerate)")
            init_tokens = init_tokens.detach()
        ticket = self._next_ticket
        self._next_ticket += 1
        self._queue.append((ticket, request, table[:, 0, :].contiguous(), init_tokens))
        return ticket

    # ---- step ------------------------------------------------------------------------------------------------------------------------------
    def _admit(self, lib, dev, stream) -> None:
        K = min(len(self._queue), self.max_active - self.active)
        if K < 1:
            return
        batch = [self._queue.popleft() for _ in range(K)]                  # FIFO: never a request ahead of an earlier one
        n, m = self.model.seq_len, self.model.splits
        # (every upload pinned and asynchronous, as run_requests': a pageable copy would hold the host until the device has run what is enqueued)
        up = lambda cpu: cpu.pin_memory().to(dev, non_blocking=True)
        seeds = [r.seed - (1 << 64) if r.seed >= 1 << 63 else r.seed for _, r, _, _ in batch]
        labels = up(torch.tensor([int(r.label) for _, r, _, _ in batch], dtype=torch.int64))
        seeds = up(torch.tensor(seeds, dtype=torch.int64))
        schedule = up(torch.cat([t for _, _, t, _ in batch]))              # int32 [sum N, 6]: the requests' records, one request after the other
        init = None
        if any(t is not None for _, _, _, t in batch):
            host = [b for b, (_, _, _, t) in enumerate(batch) if t is None or t.device.type == "cpu"]
            stacked = torch.full((len(host), n, m), self.model.mask_token, dtype=torch.int64)   # (no map: every slot masked, the same start state)
            for j, b in enumerate(host):
                if batch[b][3] is not None:
                    stacked[j] = batch[b][3]
            if len(host) == K:
                init = up(stacked)
            else:
                init = torch.empty((K, n, m), dtype=torch.int64, device=dev)
                if host:
                    init[up(torch.tensor(host))] = up(stacked)
                for b, (_, _, _, t) in enumerate(batch):
                    if t is not None and t.device.type != "cpu":
                        init[b] = t.to(dev)
        num_steps = (C.c_int * K)(*[r.num_steps for _, r, _, _ in batch])
        tickets = (C.c_uint64 * K)()
        _lib.check(lib.mb_session_admit(self._handle, K, labels.data_ptr(), seeds.data_ptr(), num_steps, schedule.data_ptr(),
                                        init.data_ptr() if init is not None else None, tickets, stream), "mb_session_admit")
        assert list(tickets) == [t for t, _, _, _ in batch], "the library's tickets count as submit's do"
        for t, r, _, _ in batch:
            self._running[t] = r

    @torch.no_grad()
    def step(self, return_predictions: bool = False):
        """Admit the queued requests that fit, run one step for every active request -> the list of ``Finished`` for the requests this step was the
        last of (in the order of their rows).  ``return_predictions``: -> (that list, {ticket: this step's predicted tokens int64 [n, m]}) for every
        request that ran -- ``combine_factorized_tokens`` and ``decode_tokens`` turn one into a preview.  Enqueue-only: nothing synchronises.  An empty
        session with an empty queue returns ``[]`` and launches nothing."""
        if self._handle is None and not self._queue:
            return ([], {}) if return_predictions else []
        dev = self.model._require_cuda("SamplingSession.step")
        lib = _lib.load()
        model, tok = self.model, self.vqgan_model
        model.eval()
        n, m = model.seq_len, model.splits
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            if self._handle is None:
                h = C.c_void_p()
                _lib.check(lib.mb_session_create(n, m, model.bits, self.max_active, self.max_steps, 1 if self.guided else 0, C.byref(h)), "mb_session_create")
                self._handle = h
            self._admit(lib, dev, stream)
            A, due = self.active, int(lib.mb_session_due(self._handle))
            if A == 0:
                return ([], {}) if return_predictions else []
            pred = torch.empty((A, n, m), dtype=torch.int64, device=dev) if return_predictions else None
            codes = torch.empty((due, n), dtype=torch.int64, device=dev)
            img = u8 = hdec = None
            if tok is not None and due:
                tok.eval()
                side = int(round(n ** 0.5))
                res = side << (tok.num_resolutions - 1)
                if self.return_uint8:
                    u8 = torch.empty((due, res, res, tok.num_channels), dtype=torch.uint8, device=dev)
                else:
                    img = torch.empty((due, tok.num_channels, res, res), dtype=torch.float32, device=dev)
                hdec = tok.engine(due, side)
            hgen = model.engine(2 * self.max_active if self.guided else self.max_active)
            finished, ran, k = (C.c_uint64 * max(due, 1))(), (C.c_uint64 * A)(), C.c_int(0)
            ptr = lambda t: t.data_ptr() if t is not None else None
            _lib.check(lib.mb_session_tick(self._handle, hgen, hdec, ptr(pred), codes.data_ptr() if due else None, ptr(img), ptr(u8), finished, ran,
                                           C.byref(k), stream), "mb_session_tick")
        self.ticks += 1
        assert k.value == due
        images = u8 if self.return_uint8 else img
        out = [Finished(int(finished[j]), self._running.pop(int(finished[j])), codes[j], images[j] if images is not None else None) for j in range(due)]
        if return_predictions:
            return out, {int(ran[r]): pred[r] for r in range(A)}
        return out

    def drain(self) -> List[Finished]:
        """Step until nothing is active or queued -> everything that finished on the way, in order."""
        out: List[Finished] = []
        while self.active or self.queued:
            out.extend(self.step())
        return out
