"""Model base for the HIP-backed MaskBit modules.

Mirrors the surface of the reference's ``BaseModel`` (modeling/modules/base_model.py:44-185):
``load_pretrained`` / ``save_pretrained`` / ``.device`` / ``.dtype`` / ``num_parameters`` with the
same checkpoint format (a flat ``torch.save``d state_dict, optional key-prefix renaming), so the
reference's drivers keep working.  Unlike the reference, a model here is a *spec-driven parameter
tree*: subclasses list ``(checkpoint key, shape, init)`` and the tree of (empty) container modules
is generated from the dotted names, which reproduces the reference's state_dict keys exactly
without mirroring its module classes.  Compute happens in libmaskbit_hip.so; the torch parameters
are the weight store the engine is (re)loaded from whenever they change.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, Iterable, Mapping, Optional, Tuple, Union

import torch

from . import _lib


class _Node(torch.nn.Module):
    """Empty container; exists only to give parameters their dotted checkpoint names."""


ParamSpec = Tuple[str, Tuple[int, ...], str]          # (key, shape, init kind)


def _init_tensor(shape, kind: str) -> torch.Tensor:
    if kind == "normal":                               # trunc-normal(0.02) like the reference's Linear/Embedding init
        return torch.nn.init.trunc_normal_(torch.empty(shape), mean=0.0, std=0.02)
    if kind == "ones":
        return torch.ones(shape)
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "kaiming":                              # conv default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        bound = 1.0 / max(fan_in, 1) ** 0.5
        return torch.empty(shape).uniform_(-bound, bound)
    raise ValueError(kind)


StateLike = Union[str, os.PathLike, Mapping[str, torch.Tensor]]


def read_state(src: StateLike) -> Dict[str, torch.Tensor]:
    """a checkpoint path (``torch.load`` onto the CPU) or a state dict -> a dict of its own"""
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(os.fspath(src), map_location="cpu")
    return dict(src)


class BaseModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._engine = None            # ctypes handle (c_void_p)
        self._engine_key = None        # (device index, capacity)
        self._engine_sig = None        # weight signature the engine was loaded from

    # ------------------------------------------------------------------ parameter tree
    def _attach(self, key: str, tensor: torch.Tensor, buffer: bool = False) -> None:
        parts = key.split(".")
        mod: torch.nn.Module = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        if buffer:
            mod.register_buffer(parts[-1], tensor)
        else:
            mod.register_parameter(parts[-1], torch.nn.Parameter(tensor))

    def _attach_convbn(self, conv: str, bn: str, shape, counter: bool) -> None:
        """a bias-free convolution ``conv``.weight [cout, cin, kh, kw] and its BatchNorm ``bn``.* -- weight, bias, the two running statistics
        and, with ``counter``, torch's ``num_batches_tracked`` buffer -- as zeros"""
        cout = shape[0]
        self._attach(conv + ".weight", torch.zeros(*shape))
        self._attach(bn + ".weight", torch.zeros(cout))
        self._attach(bn + ".bias", torch.zeros(cout))
        self._attach(bn + ".running_mean", torch.zeros(cout), buffer=True)
        self._attach(bn + ".running_var", torch.zeros(cout), buffer=True)
        if counter:
            self._attach(bn + ".num_batches_tracked", torch.zeros((), dtype=torch.int64), buffer=True)

    def _build(self, specs: Iterable[ParamSpec]) -> None:
        for key, shape, kind in specs:
            self._attach(key, _init_tensor(tuple(shape), kind))

    # ------------------------------------------------------------------ reference surface
    @property
    def device(self) -> torch.device:
        for p in self.parameters():
            return p.device
        for b in self.buffers():
            return b.device
        return torch.device("cpu")

    @property
    def dtype(self) -> torch.dtype:
        for p in self.parameters():
            return p.dtype
        return torch.float32

    def num_parameters(self, only_trainable: bool = False, exclude_embeddings: bool = False) -> int:
        skip = {"class_emb.weight"} if exclude_embeddings else set()
        return sum(p.numel() for n, p in self.named_parameters() if n not in skip and (p.requires_grad or not only_trainable))

    def save_pretrained(self, save_directory: Union[str, os.PathLike], save_function: Optional[Callable] = None,
                        state_dict: Optional[Dict[str, torch.Tensor]] = None) -> None:
        if os.path.isfile(save_directory):
            print(f"Provided path ({save_directory}) should be a directory, not a file")
            return
        os.makedirs(save_directory, exist_ok=True)
        path = os.path.join(save_directory, "pytorch_model.bin")
        (save_function or torch.save)(self.state_dict() if state_dict is None else state_dict, path)
        print(f"Model weights saved in {path}")

    def load_pretrained(self, pretrained_model_path: Union[str, os.PathLike], strict_loading: bool = True,
                        torch_dtype: Optional[torch.dtype] = None, rename_keys: Optional[Dict[str, str]] = None) -> None:
        path = str(pretrained_model_path)
        if os.path.isdir(path):
            path = os.path.join(path, "pytorch_model.bin")
        if not os.path.isfile(path):
            raise ValueError(f"{path} does not exist")
        ckpt = torch.load(path, map_location="cpu")
        if rename_keys:
            renamed = {}
            for k, v in ckpt.items():
                for old, new in rename_keys.items():
                    if k.startswith(old):
                        k = k.replace(old, new)
                        break
                renamed[k] = v
            ckpt = renamed
        self.load_state_dict(ckpt, strict=strict_loading)
        if torch_dtype is not None:
            if not isinstance(torch_dtype, torch.dtype):
                raise ValueError(f"{torch_dtype} needs to be of type `torch.dtype`, e.g. `torch.float16`, but is {type(torch_dtype)}.")
            self.to(torch_dtype)
        self.eval()

    # ------------------------------------------------------------------ engine plumbing
    def _weight_signature(self):
        """Identity of the current weights (storage, in-place version counter, dtype per entry).  Computed once per engine() call -- the walk over ~300 entries costs
        ~1 ms of host time and engine() sits on the per-step-chunk path --: a caller may hand the value on (`_sig_hint`) for the duration of ONE call."""
        hint = getattr(self, "_sig_hint", None)
        if hint is not None:
            return hint
        return tuple((k, t.data_ptr(), t._version, t.dtype) for k, t in self.state_dict(keep_vars=True).items())

    def _require_cuda(self, what: str) -> torch.device:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__}.{what} runs only on an AMD GPU through libmaskbit_hip.so (model is on {dev}); "
                "maskbit_amd has no CPU path. Move the model with .to('cuda').")
        return dev

    def _drop_engine(self) -> None:
        if self._engine is not None:
            self._engine_destroy(self._engine)
            self._engine = None
            self._engine_key = None
            self._engine_sig = None

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    # subclasses provide _engine_create(capacity) -> handle and _ABI, the family of their handle's entry points: mb_{_ABI}_load / _destroy /
    # _saturation_count ("gen", "dec", "lpips", "inception", "taming")
    _ABI = ""
    _COUNTS = ""                       # what saturation_count() counts in this class, in words

    def _engine_destroy(self, h) -> None:
        getattr(_lib.load(), f"mb_{self._ABI}_destroy")(h)

    def _engine_load(self, h, key: str, t: torch.Tensor, stream: int) -> None:
        entry = f"mb_{self._ABI}_load"
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(getattr(_lib.load(), entry)(h, key.encode(), t.data_ptr(), shape, t.dim(), stream), f"{entry}({key})")

    def saturation_count(self, reset: bool = True) -> int:
        """What the current engine clamped at the fp16 range (+-65504) since the last reset -- the class's ``_COUNTS`` says what is counted; 0
        without an engine.  A checkpoint whose activations need more range shows up here instead of being clipped silently.  Synchronises the
        current stream."""
        if self._engine is None:
            return 0
        entry = f"mb_{self._ABI}_saturation_count"
        n = C.c_uint(0)
        with torch.cuda.device(self._require_cuda("saturation_count")):
            _lib.check(getattr(_lib.load(), entry)(self._engine, C.byref(n), 1 if reset else 0, torch.cuda.current_stream().cuda_stream), entry)
        return int(n.value)

    def _ensure_engine(self, capacity: int):
        """Create (or grow) the device engine and (re)load weights if the torch parameters changed."""
        dev = self._require_cuda("forward")
        key_dev = dev.index if dev.index is not None else torch.cuda.current_device()
        if self._engine is not None and (self._engine_key[0] != key_dev or self._engine_key[1] < capacity):
            self._drop_engine()
        with torch.cuda.device(key_dev):
            if self._engine is None:
                self._engine = self._engine_create(capacity)
                self._engine_key = (key_dev, capacity)
            sig = self._weight_signature()
            if sig != self._engine_sig:
                stream = torch.cuda.current_stream().cuda_stream
                keep = []
                for k, t in self.state_dict(keep_vars=True).items():
                    if not t.is_floating_point():
                        continue                                   # integer buffers are derived on the device
                    src = t.detach()
                    if src.dtype != torch.float32 or not src.is_contiguous():
                        src = src.float().contiguous()
                    keep.append(src)
                    self._engine_load(self._engine, k, src, stream)
                torch.cuda.current_stream().synchronize()          # temporaries in `keep` must outlive the repack
                self._engine_sig = sig
        return self._engine


class PairLoss(BaseModel):
    """What the image-pair losses (``LPIPS``, ``PerceptualLoss``) share: the shape checks, the run in chunks into a float64 [B] device tensor,
    ``per_image`` and the grow-only engine.  A subclass states its network (``_INPUT``, for the messages), its size rule (``_size_error``), what
    to say while it has no weights (``_no_weights``), its chunk size (``_chunk``) and the one ``mb_*_forward`` call (``_forward_chunk``)."""
    max_pairs_per_call = 16
    _INPUT = ""

    @staticmethod
    def _size_error(H: int, W: int) -> Optional[str]:
        """what the engine takes instead, when it does not take H x W"""
        raise NotImplementedError

    def _no_weights(self) -> Optional[str]:
        """which loaders to call first, while weights are missing"""
        raise NotImplementedError

    def note_loaded_keys(self, keys) -> None:
        """Counts as loaded every part of the network that the state-dict keys ``keys`` (relative to this module) cover completely.  The
        module's own ``load_state_dict`` calls it; a parent that loaded this module's entries through torch's recursive loader (``VQGANLoss``)
        calls it with its own keys, stripped of the prefix."""
        raise NotImplementedError

    def _chunk(self, H: int, W: int) -> int:
        return int(self.max_pairs_per_call)

    def _forward_chunk(self, h, a: int, b: int, n: int, H: int, W: int, clamp: int, out: int, running_sum: Optional[int], stream: int) -> int:
        raise NotImplementedError

    def engine(self, pairs: int, H: int = 0, W: int = 0):
        have = self._engine_key[1] if self._engine_key else 0
        return self._ensure_engine(max(pairs, have))

    @classmethod
    def check_images(cls, shape_a, shape_b) -> None:
        """``ValueError`` for what the engine does not take; no device work."""
        name = cls.__name__
        if len(shape_a) != 4 or tuple(shape_a) != tuple(shape_b):
            raise ValueError(f"{name} expects two [B, 3, H, W] batches of one shape, got {tuple(shape_a)} and {tuple(shape_b)}")
        B, Cc, H, W = (int(v) for v in shape_a)
        if B < 1:
            raise ValueError(f"{name}: empty batch {tuple(shape_a)}")
        if Cc != 3:
            raise ValueError(f"{name} takes 3 channels (the {cls._INPUT} input), got {Cc}")
        why = cls._size_error(H, W)
        if why:
            raise ValueError(f"{name}: images of {H} x {W}: the HIP engine takes {why}")

    def _run(self, a: torch.Tensor, b: torch.Tensor, clamp: bool, running_sum: Optional[torch.Tensor] = None) -> torch.Tensor:
        self.check_images(a.shape, b.shape)
        why = self._no_weights()
        if why:
            raise RuntimeError(f"{type(self).__name__} has no weights yet: call {why} first (nothing is loaded at construction)")
        dev = self._require_cuda("forward")
        B, _, H, W = (int(v) for v in a.shape)
        a = a.to(device=dev, dtype=torch.float32).contiguous()
        b = b.to(device=dev, dtype=torch.float32).contiguous()
        chunk = max(1, min(B, self._chunk(H, W)))
        h = self.engine(chunk, H, W)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        total = running_sum.data_ptr() if running_sum is not None else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for b0 in range(0, B, chunk):
                n = min(chunk, B - b0)
                rc = self._forward_chunk(h, a[b0:b0 + n].data_ptr(), b[b0:b0 + n].data_ptr(), n, H, W, 1 if clamp else 0, out[b0:b0 + n].data_ptr(),
                                         total, stream)
                _lib.check(rc, f"mb_{self._ABI}_forward")
        return out

    @torch.no_grad()
    def per_image(self, input: torch.Tensor, target: torch.Tensor, clamp: bool = False) -> torch.Tensor:
        """The loss of every pair as float64 [B] on the device (``clamp=True``: both images clamped to [0, 1] inside the input kernel).  Batches
        beyond the chunk size (``max_pairs_per_call``) are walked in chunks; a pair's value does not depend on the chunking.  No synchronisation."""
        return self._run(input, target, clamp)
