"""Plain restatements of the quantizer kernels (csrc/vq.hip; lfq_kernel, latent_kernel, pack_image_kernel of csrc/conv.hip) and the inputs of
their exact tests (tests/test_quantizer_cpu.py, tests/test_hip_quantizer.py).  torch on the CPU, float64 / int64 / uint64 where a value is decided.

Every kernel here selects, compares, copies or rounds once; none accumulates anything that is kept.  With operands that are small integers the
scores of the lookup search are exact in fp32 in any order (asserted by `search_premise`), so the tests compare bit for bit and leave no row out.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

H16_MAX = 65504.0


# --------------------------------------------------------------------------------------------------------------- restatements
def lookup_search(z: torch.Tensor, cb: torch.Tensor, B: int, HW: int):
    """SimpleVectorizer.forward without normalisation (quantizer.py:64-72): z [B*HW, K], cb [C, K] ->
    idx int64 [N] = argmin_j ||e_j||^2 - 2 z.e_j, the LOWEST index among equal scores, 0 where no score compares (a row of NaN);
    dist float64 [N] = sum_k (z_k - e_idx,k)^2; zq float32 [B, K, HW] = the chosen rows; zraw float32 [B, K, HW] = the rows as given.
    Defined for rows whose scores are all finite or all NaN only: with SOME scores NaN this gives 0 (NaN propagates through min), while the
    kernel skips NaN scores and picks the best of the others."""
    N, K = z.shape
    assert N == B * HW and cb.shape[1] == K
    zd, e = z.double(), cb.double()
    en = (e * e).sum(1)
    idx = torch.empty(N, dtype=torch.int64)
    for r0 in range(0, N, 64):
        score = en[None, :] - 2.0 * (zd[r0:r0 + 64] @ e.T)
        best = score.min(dim=1, keepdim=True).values                # NaN for a row with a NaN score: nothing equals it, argmax of all-False is 0
        idx[r0:r0 + 64] = (score == best).to(torch.int8).argmax(dim=1)
    sel = e[idx]
    dist = ((zd - sel) ** 2).sum(1)
    nchw = lambda rows: rows.reshape(B, HW, K).permute(0, 2, 1).contiguous()
    return idx, dist, nchw(cb.float()[idx]), nchw(z.float())


def to_h16_saturating(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp16, round to nearest even, +-65504 instead of +-inf."""
    return v.float().clamp(-H16_MAX, H16_MAX).to(torch.float16)


def saturated(v: torch.Tensor) -> int:
    return int((v.float().abs() > H16_MAX).sum())


def gather_latent(codes: torch.Tensor, cb: torch.Tensor, cin_pad: int):
    """get_codebook_entry (quantizer.py:106-119) on device-resident codes: clamped to [0, C), fp16 NHWC rows padded with +0 to cin_pad channels ->
    (out fp16 [npix, cin_pad], number of stored elements beyond +-65504)."""
    C, K = cb.shape
    v = torch.zeros(codes.numel(), cin_pad, dtype=torch.float32)
    v[:, :K] = cb.float()[codes.clamp(0, C - 1)]
    return to_h16_saturating(v), saturated(v)


def pack_latent(z_nchw: torch.Tensor, cin_pad: int):
    """fp32 [B, K, HW] -> (fp16 [B*HW, cin_pad], saturation count), as gather_latent stores."""
    B, K, HW = z_nchw.shape
    v = torch.zeros(B * HW, cin_pad, dtype=torch.float32)
    v[:, :K] = z_nchw.float().permute(0, 2, 1).reshape(B * HW, K)
    return to_h16_saturating(v), saturated(v)


def bits_to_code(bits: torch.Tensor) -> torch.Tensor:
    """bool [N, K] -> int64 [N], bit j = bits[:, j] (LSB first), by shifts in uint64: K = 64 gives the two's-complement pattern."""
    b = bits.numpy().astype(np.uint64)
    code = np.zeros(b.shape[0], dtype=np.uint64)
    for j in range(b.shape[1]):
        code |= b[:, j] << np.uint64(j)
    return torch.from_numpy(code.view(np.int64).copy())


def lfq_pack(z16: torch.Tensor, B: int, HW: int, K: int):
    """LookupFreeQuantizer.forward / convert_bits_to_indices (lookup_free.py:57-62,113-127) with int64 codes: z16 fp16 [B*HW, Kp] ->
    idx int64 [N], bit j = (z_j > 0); zq float32 [B, K, HW] = where(z > 0, 1, -1); zraw float32 [B, K, HW] = the fp16 values."""
    v = z16[:, :K].float()
    pos = v > 0.0
    nchw = lambda rows: rows.reshape(B, HW, K).permute(0, 2, 1).contiguous()
    return bits_to_code(pos), nchw(torch.where(pos, torch.ones_like(v), -torch.ones_like(v))), nchw(v)


def lfq_latent(tokens: torch.Tensor, K: int) -> torch.Tensor:
    """get_codebook_entry (lookup_free.py:96-111) with int64 codes: tokens [N] -> fp16 [N, 64], +-1 in the first K channels, +0 beyond."""
    out = torch.zeros(tokens.numel(), 64, dtype=torch.float16)
    for j in range(K):
        out[:, j] = (((tokens >> j) & 1) != 0).to(torch.float16) * 2.0 - 1.0
    return out


def pack_image(img: torch.Tensor) -> torch.Tensor:
    """fp32 [B, C, H, W] -> fp16 [B*H*W, 64], channels >= C are +0."""
    B, C, H, W = img.shape
    out = torch.zeros(B * H * W, 64, dtype=torch.float16)
    out[:, :C] = to_h16_saturating(img.permute(0, 2, 3, 1).reshape(-1, C))
    return out


# --------------------------------------------------------------------------------------------------------------- the search cases
SPLITS = (1, 0, 2, 3, 7, 64)
K_VALUES = (1, 3, 4, 5, 48, 64, 65, 100, 128, 129, 255, 256)
C_VALUES = (2, 63, 64, 65, 128, 1000)
BHW_VALUES = ((1, 1), (1, 127), (1, 128), (1, 129), (3, 25), (2, 256))


class SearchCase(NamedTuple):
    name: str
    K: int
    C: int
    B: int
    HW: int
    kind: str = "random"      # "random": entries and rows from {-3 .. 3}; see search_case for the others


def _search_cases():
    """Every value of every parameter with the others at their smallest and at their largest, a few mixed ones, and the special codebooks."""
    seen, out = set(), []

    def add(K, C, bhw, kind="random"):
        key = (K, C, bhw, kind)
        if key not in seen:
            seen.add(key)
            out.append(SearchCase(f"{kind}-K{K}-C{C}-{bhw[0]}x{bhw[1]}", K, C, bhw[0], bhw[1], kind))

    lo, hi = (K_VALUES[0], C_VALUES[0], BHW_VALUES[0]), (K_VALUES[-1], C_VALUES[-1], BHW_VALUES[-1])
    for ext in (lo, hi):
        for K in K_VALUES:
            add(K, ext[1], ext[2])
        for C in C_VALUES:
            add(ext[0], C, ext[2])
        for bhw in BHW_VALUES:
            add(ext[0], ext[1], bhw)
    for K, C, bhw in ((100, 65, (3, 25)), (5, 63, (1, 129)), (129, 128, (1, 127)), (65, 64, (1, 128)), (48, 1000, (3, 25)), (3, 65, (2, 256))):
        add(K, C, bhw)
    add(4, 65536, (1, 129), "grid")          # the 16^4 grid on {-8 .. 7}: all entries distinct, rows are chosen entries
    add(8, 65, (1, 129), "padding")          # z = 0: the smallest-norm real entry, never one of the 63 padding entries
    add(256, 256, (1, 256), "impulse")       # e_j = one-hot(j), z = one-hot(k)
    add(100, 100, (1, 100), "impulse")
    add(16, 512, (3, 25), "ties")            # duplicated entries in other lanes, chunks and splits
    return tuple(out)


SEARCH_CASES = _search_cases()


def _gen(*seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(sum((i + 1) * 1009 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _small_ints(g, *shape) -> torch.Tensor:
    return torch.randint(-3, 4, shape, generator=g).float()


# where the copies of each base entry of the "ties" codebook sit: neighbouring lanes, other column tiles of one chunk, other chunks (other splits
# for every split count > 1 of an 8-chunk codebook), the lowest copy not always the first chunk's
TIE_PLACES = ((5, 6, 22, 70), (17, 16, 80, 300), (63, 64, 448), (130, 129, 190, 128 + 63), (200, 264, 328, 392, 456, 201), (511, 510, 447),
              (321, 385, 322), (40, 41, 42, 43, 104, 168), (259, 258, 257, 256 + 48), (12, 500), (76, 75, 140), (460, 396, 461))


@functools.lru_cache(maxsize=None)
def search_case(case: SearchCase):
    """-> (z fp32 [N, K], codebook fp32 [C, K], expected index int64 [N] known by construction, or None)"""
    K, C, N = case.K, case.C, case.B * case.HW
    g = _gen(K, C, N, len(case.kind))
    if case.kind == "random":
        return _small_ints(g, N, K), _small_ints(g, C, K), None
    if case.kind == "grid":
        v = torch.arange(-8, 8).float()
        cb = torch.cartesian_prod(v, v, v, v)
        cb = cb[torch.randperm(C, generator=g)].contiguous()
        want = torch.cat([torch.tensor([0, C - 1, 63, 64, 32767, 32768]), torch.randint(0, C, (N - 6,), generator=g)])
        return cb[want].clone(), cb, want
    if case.kind == "padding":
        cb = _small_ints(g, C, K)
        cb[:, 0], cb[:, 1] = 2.0, -1.0                              # every norm >= 5 ...
        cb[37] = 0.0
        cb[37, 3] = 1.0                                             # ... but one, and that is not entry 0
        return torch.zeros(N, K), cb, torch.full((N,), 37)
    if case.kind == "impulse":
        return torch.eye(K)[:N].clone(), torch.eye(K)[:C].clone(), torch.arange(N)
    assert case.kind == "ties"
    base = _small_ints(g, len(TIE_PLACES), K)
    base[:, 0] = 0.0
    base[:, 1] = torch.arange(len(TIE_PLACES)).float() % 7 - 3       # together with column 2: all different
    base[:, 2] = torch.arange(len(TIE_PLACES)).float() // 7
    cb = torch.where(torch.rand(C, K, generator=g) < 0.5, -3.0, 3.0)  # the filler has no zero: never equal to a base entry
    for i, places in enumerate(TIE_PLACES):
        cb[list(places)] = base[i]
    rows = torch.arange(N) % len(TIE_PLACES)
    return base[rows].clone(), cb, torch.tensor([min(p) for p in TIE_PLACES])[rows]


def search_premise(z: torch.Tensor, cb: torch.Tensor) -> float:
    """The largest value any partial sum of a z.e product, in any order, or any score ||e||^2 - 2 z.e can reach in absolute value: while it stays
    below 2^24 with integer operands, fp32 computes every one of them exactly."""
    assert torch.equal(z, z.round()) and torch.equal(cb, cb.round())
    dot = float((z.double().abs() @ cb.double().abs().T).max())
    return float((cb.double() ** 2).sum(1).max()) + 2.0 * dot


def nonfinite_case():
    """Ordinary integer rows with one row of NaN (5) and one of +inf (77).  K = 48 < Kp = 64: the zero padding columns make every score of the
    +inf row NaN as well (inf * 0), as the zeros among the entries do in the reference expression."""
    g = _gen(48, 300, 129, 99)
    z, cb = _small_ints(g, 129, 48), _small_ints(g, 300, 48)
    z[5], z[77] = float("nan"), float("inf")
    return z, cb, (5, 77)


def fp16_rows(z: torch.Tensor, stride: int) -> torch.Tensor:
    """[N, K] -> fp16 [N, stride], NaN in the columns at and beyond K"""
    out = torch.full((z.shape[0], stride), float("nan"), dtype=torch.float16)
    out[:, :z.shape[1]] = z.to(torch.float16)
    return out


def strides16(K: int):
    return sorted({K, (K + 3) // 4 * 4, K + 24})


# --------------------------------------------------------------------------------------------------------------- gather / latent pack
GATHER_CASES = ((12, 300, 333), (64, 2, 130), (100, 65, 97), (256, 1000, 1100), (12, 64, 4096 * 256 // 64 + 1))   # (K, C, npix); cin_pad = K up to 64
PACK_LATENT_CASES = ((3, 12, 25), (2, 64, 256), (1, 100, 16), (5, 12, 3277))                                     # (B, K, HW); 5 * 3277 * 64 > 4096 * 256
ROUNDING_PROBES = (70000.0, -70000.0, 65504.0, -65504.0, 65519.996, -65520.0, 65504.004, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, -2.0 ** -24,
                   6.0e-8, 1.0e-8, 0.0, -0.0, 3.0e38, -3.0e38)


def cin_pad_of(K: int) -> int:
    return (K + 63) // 64 * 64


def _plant(flat: torch.Tensor, values, g) -> None:
    n = min(len(values), flat.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = torch.tensor(values[:n], dtype=flat.dtype)


@functools.lru_cache(maxsize=None)
def gather_case(K: int, C: int, npix: int):
    """-> (codes int64 [npix], codebook fp32 [C, K]): nearly every entry is used, the rounding probes are in the codebook, codes beyond both ends."""
    g = _gen(K, C, npix, 7)
    cb = torch.randn(C, K, generator=g) * 3.0
    _plant(cb.view(-1), ROUNDING_PROBES, g)
    codes = torch.arange(npix) % C
    codes = codes[torch.randperm(npix, generator=g)]
    special = torch.tensor([0, C - 1, -1, -2 ** 40, C, 2 ** 40, -2 ** 63, 2 ** 63 - 1, 2 ** 32, -2 ** 32 + 1])
    codes[torch.randperm(npix, generator=g)[:min(npix, len(special))]] = special[:npix]
    return codes, cb


@functools.lru_cache(maxsize=None)
def pack_latent_case(B: int, K: int, HW: int):
    g = _gen(B, K, HW, 8)
    z = torch.randn(B, K, HW, generator=g) * 3.0
    _plant(z.view(-1), ROUNDING_PROBES, g)
    return z


# --------------------------------------------------------------------------------------------------------------- LFQ
LFQ_K = (1, 10, 12, 18, 31, 32, 33, 62, 63, 64)
LFQ_BHW = ((1, 1), (3, 25), (2, 256))
LFQ_BIG = (12, 1, 1024 * 256 + 1)          # (K, B, HW): the pack's grid-stride loop takes a second pass
LATENT_BIG = 2048 * 256 // 64 + 1          # pixels: the latent kernel's grid-stride loop takes a second pass
H16_PROBES_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x03FF, 0x83FF, 0x0400, 0x8400)
# +0, -0, the smallest subnormals, +-65504, +-inf, NaN, the largest subnormals, the smallest normals


def lfq_pack_cases():
    out = []
    for K in LFQ_K:
        for Kp in ((K + 3) // 4 * 4, K + 8):
            out.append((K, Kp, 3, 25))
    for K in LFQ_K:
        for B, HW in LFQ_BHW:
            if (B, HW) != (3, 25):
                out.append((K, (K + 3) // 4 * 4, B, HW))
    out.append((LFQ_BIG[0], 12, LFQ_BIG[1], LFQ_BIG[2]))
    return out


@functools.lru_cache(maxsize=None)
def lfq_pack_case(K: int, Kp: int, B: int, HW: int) -> torch.Tensor:
    """fp16 [B*HW, Kp]: random values, the probes planted in the first K columns (as many as fit), NaN in the columns beyond K"""
    g = _gen(K, Kp, B, HW)
    N = B * HW
    z = torch.full((N, Kp), float("nan"), dtype=torch.float16)
    live = (torch.randn(N, K, generator=g) * 0.7).to(torch.float16)
    probes = torch.tensor(np.array(H16_PROBES_BITS, dtype=np.uint16).view(np.int16).copy()).view(torch.float16)
    reps = 1 if N * K < 64 else 4
    flat = live.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:reps * len(probes)]
    flat[pos] = probes.repeat(reps)[:len(pos)]
    z[:, :K] = live
    return z


@functools.lru_cache(maxsize=None)
def lfq_tokens(K: int, n: int) -> torch.Tensor:
    """all 2^K codes for K = 10, else n random codes over the whole K-bit range (K = 64: negative int64 values included) with the two ends"""
    if K == 10:
        return torch.arange(1024)
    bits = torch.randint(0, 2, (n, K), generator=_gen(K, n, 5)).bool()
    bits[0], bits[-1] = False, True
    return bits_to_code(bits)


# --------------------------------------------------------------------------------------------------------------- image pack
def pack_image_cases():
    return [(B, C, H, W) for C in (1, 3, 4) for (H, W) in ((5, 7), (16, 16)) for B in (1, 3)]


@functools.lru_cache(maxsize=None)
def pack_image_case(B: int, C: int, H: int, W: int) -> torch.Tensor:
    g = _gen(B, C, H, W)
    img = torch.rand(B, C, H, W, generator=g) * 2.0 - 0.5
    _plant(img.view(-1), ROUNDING_PROBES, g)
    return img


# --------------------------------------------------------------------------------------------------------------- l2 cases of test_hip_vq.py
ARGMIN_L2_ADDED = ((512, 128), (300, 100))      # (C, K): the Kp = 128 instantiation under normalisation
ARGMIN_ROWS = (1, 255, 16401)


@functools.lru_cache(maxsize=None)
def argmin_inputs(C: int, K: int, l2: bool):
    """The inputs of test_argmin_exact_vs_fp64 for the added (C, K), seeded on the CPU so that tests/test_quantizer_cpu.py sees the same numbers:
    -> (codebook [C, K], {N: z [N, K]}) in the distribution that test draws."""
    g = _gen(C, K, int(l2), 3)
    cb = torch.randn(C, K, generator=g)
    return cb, {N: torch.randn(N, K, generator=g) * 1.1 + 0.05 for N in ARGMIN_ROWS}


def clear_rows(z: torch.Tensor, cb: torch.Tensor, l2: bool):
    """test_argmin_exact_vs_fp64's own definition: -> (clear mask, fp64 argmin)"""
    zd, e = z.double(), cb.double()
    if l2:
        zd, e = torch.nn.functional.normalize(zd, dim=-1), torch.nn.functional.normalize(e, dim=-1)
    d = torch.cdist(zd, e).pow(2)
    top2 = d.topk(2, dim=1, largest=False)
    gap = top2.values[:, 1] - top2.values[:, 0]
    scale = zd.pow(2).sum(1) + e.pow(2).sum(1).max()
    return gap > 1e-5 * scale, top2.indices[:, 0]
