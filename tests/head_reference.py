"""References of the head path of gemm.hip, shared by tests/test_head_cpu.py and tests/test_hip_head.py: the two head GEMMs (GemmArgs.W2 / scale /
bias_per_pos, as engine.hip head_gemms launches them) and the kernels that run once per checkpoint load (split_f32_to_h16_planes, cast_f32_to_h16,
w4_from_f32, w4lo_from_f32).

The method of gemm_reference.py: operands for which the float64 result is what ANY fp32 order of additions gives, so the comparison is for equality;
statements written from the contract in mb_kernels.h, not from the kernels; and, for every statement, the wrong kernels it is meant to catch, as hooks
of the same statement -- the CPU file proves each of them is caught.  Weights beyond fp16's range (|w| >= 65520) are out of scope for w4 / w4lo: no
checkpoint has them and their e2m1 copies are not defined.  A plain module: nothing here touches the GPU."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from gemm_reference import _gen, int_operand, int_values
from hip_helpers import _F4V, f4_block_exponent, f4_codes

# ---- the shapes of the GPU file --------------------------------------------------------------------------------------------------------------------
HEAD_M, HEAD_N, HEAD_KW = (1, 127, 129, 600), (4, 132, 256), (64, 128, 192)           # epilogue 3
LOGITS_SHAPES = ((10, 5), (6, 2), (257, 257), (600, 257), (2313, 257), (1025, 1025))   # epilogue 4: (M, period); 600 is no multiple of 257: refused
SCALES = (1.0, 2.0 ** -7, 2.0 ** 3)
REAL_SHAPE = (514, 256, 128)                                                           # (M, N, kw) of the real-valued cases; epilogue 4: period 257
GELU_BOUND = 2e-4                          # of max |ref|: the project's bound for fp32 GELU outputs (test_hip_gemm_exact.py)
HI_ONLY_FACTOR = 8.0                       # the three-sweep result is this much closer to float64 than the hi plane alone (test_split_activation_gemm's factor)
# Real-valued head GEMMs: kernel error <= max(F * E_ref, 2 ulp32), E_ref = the error of a plain fp32 CPU matmul of the same operands.  F = twice the
# worst ratio measured on the MI355X (profiles/head_kernels.md, "E_ref ratios").
F_REF = 1.93
SPLIT_SHAPES = ((1, 4), (3, 5), (64, 128), (768, 768))                                  # the last: more than 2048 * 256 elements, a second grid pass
GRID_PASS = 2048 * 256                                                                  # elements the first pass of absmax_kernel / split_kernel covers
CAST_N = (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2048 * 256 * 4 + 3)
W4_SHAPES = ((64, 128), (64, 256), (128, 1024), (192, 1152), (64, 2048), (64, 4096))
MAX_UNDECIDED = 0.02                       # share of (row, 128-column) blocks whose scale choice float64 does not decide
DECIDED_GAP, DECIDED_HALF = 1e-4, 1e-3     # relative gap between the two best candidates; distance of log2(2.2 / rms) from a half-integer
UNDECIDED_SLACK = 1e-3


# ===== head GEMM =======================================================================================================================================
@dataclass
class HeadCase:
    epi: int                                 # 3 (GELU) or 4 (logits)
    M: int
    N: int
    kw: int
    A: torch.Tensor                          # fp16 [M, kw], integers -3..3
    A2: torch.Tensor                         # fp16 [M, kw], -2..2
    W: torch.Tensor                          # fp16 [N, kw], -2..2
    W2: Optional[torch.Tensor]               # fp16 [N, kw], -2..2; None: the two-sweep form
    scale: Optional[float]                   # with W2
    bias: torch.Tensor                       # fp32 [N], or [period - 1, N] with per_pos
    period: int = 0
    per_pos: bool = False

    @property
    def label(self):
        return (f"epi {self.epi} M {self.M} N {self.N} kw {self.kw}" + (f" period {self.period}" if self.epi == 4 else "") +
                (f" three sweeps scale {self.scale}" if self.W2 is not None else " two sweeps") + (" bias per position" if self.per_pos else ""))


def make_head_case(epi, M, N, kw, *, period=0, three=True, per_pos=False, scale=1.0, seed=1, dev="cpu") -> HeadCase:
    assert kw % 64 == 0 and (epi == 4 or not per_pos)
    if per_pos:                                                                         # a different integer row per position
        bias = int_values((period - 1, N), 8, seed + 2) + 20.0 * (torch.arange(period - 1) % 13 - 6).float()[:, None]
    else:
        bias = int_values((N,), 8, seed + 2)
    return HeadCase(epi, M, N, kw, int_operand(M, kw, 3, seed).half().to(dev), int_operand(M, kw, 2, seed + 4).half().to(dev),
                    int_operand(N, kw, 2, seed + 1).half().to(dev), int_operand(N, kw, 2, seed + 5).half().to(dev) if three else None,
                    scale if three else None, bias.to(dev), period, per_pos)


def _kt(x, t):
    return x[:, t * 64:(t + 1) * 64]


def head_accumulator(c: HeadCase, *, third_a=False, third_w=False, second_w2=False, boundary=0) -> torch.Tensor:
    """float64 [M, N]: the accumulator after the K-tile walk -- K-tile t of the 3 kw (2 kw) columns belongs to sweep t // (kw / 64) and multiplies tile
    t % (kw / 64) of that sweep's operands: (A, W), (A2, W), (A, W2).  Hooks: the third sweep reads A2 / reads W, the second reads W2, the sweep boundaries
    lie `boundary` K-tiles late (+1) or early (-1)."""
    A, A2, W = c.A.double(), c.A2.double(), c.W.double()
    W2 = c.W2.double() if c.W2 is not None else None
    nkw = c.kw // 64
    nsweep = 3 if W2 is not None else 2
    asrc = [A, A2, A2 if third_a else A]
    wsrc = [W, W2 if second_w2 else W, W if third_w else W2]
    acc = torch.zeros(c.M, c.N, dtype=torch.float64, device=A.device)
    for t in range(nsweep * nkw):
        seg = min(nsweep - 1, max(0, (t - boundary) // nkw))
        acc = acc + _kt(asrc[seg], t % nkw) @ _kt(wsrc[seg], t % nkw).t()
    return acc


def head_bias_rows(c: HeadCase, index="pos") -> torch.Tensor:
    """float64 [M, N]: the bias every (uncompacted) row m receives.  index: "pos" (the truth, m % period), "m", "orow" (the compacted row) -- a read
    beyond the [period - 1][N] array is modelled as its last row (the class row's own, which no kept row may see)."""
    b = c.bias.double()
    if not c.per_pos:
        return b[None, :].expand(c.M, c.N)
    m = torch.arange(c.M, device=b.device)
    pos = m % c.period
    idx = {"pos": pos, "m": m, "orow": (m // c.period) * (c.period - 1) + pos}[index]
    return b[idx.clamp(max=c.period - 2)]


def head_pre_activation(c: HeadCase, *, no_scale=False, scale_bias=False, bias_index="pos", **walk) -> torch.Tensor:
    """float64 [M, N] = acc * scale + bias, uncompacted."""
    s = 1.0 if (c.scale is None or no_scale) else c.scale
    acc, bias = head_accumulator(c, **walk), head_bias_rows(c, bias_index)
    return (acc + bias) * s if scale_bias else acc * s + bias


def head_image(c: HeadCase, pre: torch.Tensor, rows="last") -> torch.Tensor:
    """What the launch leaves in an output buffer of M rows that held NaN: epilogue 3: float64 GELU [M, N]; epilogue 4: fp32 [M, N], row m at
    (m // period) * (period - 1) + m % period, rows with m % period == period - 1 dropped, the unwritten tail NaN.  rows: "last" (the truth), "first"
    (row 0 of each period dropped instead), "keep" (the class row is kept), "stride" (compaction stride period instead of period - 1)."""
    if c.epi == 3:
        return torch.nn.functional.gelu(pre)
    m = torch.arange(c.M, device=pre.device)
    sq, pos = m // c.period, m % c.period
    keep, orow = {"last": (pos != c.period - 1, sq * (c.period - 1) + pos), "first": (pos != 0, sq * (c.period - 1) + pos - 1),
                  "keep": (pos >= 0, m), "stride": (pos != c.period - 1, sq * c.period + pos)}[rows]
    img = torch.full((c.M, c.N), float("nan"), dtype=torch.float32, device=pre.device)
    img[orow[keep]] = pre[keep].float()
    return img


def head_out_rows(c: HeadCase) -> int:
    return c.M - c.M // c.period if c.epi == 4 else c.M


def head_expected(c: HeadCase) -> torch.Tensor:
    """[head_out_rows, N]: fp32 bits to equal (epilogue 4), float64 GELU values (epilogue 3)."""
    return head_image(c, head_pre_activation(c))[:head_out_rows(c)]


def head_precondition(c: HeadCase) -> float:
    """What makes equality legitimate: every partial sum of an output element, in any order, is an integer below 2^24 (sum |a| |w| over all sweeps bounds
    it), and every expected value acc * scale + bias survives a float32 round trip -- then neither the accumulation nor the fmaf of the epilogue rounds.
    -> the largest sum |a| |w|."""
    A, A2, W = c.A.double().abs(), c.A2.double().abs(), c.W.double().abs()
    tot = (A + A2) @ W.t() + (A @ c.W2.double().abs().t() if c.W2 is not None else 0)
    worst = float(tot.max())
    assert worst < 2.0 ** 24, worst
    acc = head_accumulator(c)
    assert torch.equal(acc, acc.round())
    pre = head_pre_activation(c)
    assert torch.equal(pre.float().double(), pre), "an expected value is no float32"
    assert c.epi == 4 or gelu_case_is_meaningful(c)
    for x in (c.A, c.A2, c.W) + ((c.W2,) if c.W2 is not None else ()):
        assert torch.equal(x.double(), x.double().round()) and float(x.double().abs().max()) <= 3
    return worst


def gelu_case_is_meaningful(c: HeadCase) -> bool:
    """The GELU bound is relative to max |ref|.  Where every pre-activation of a case is negative -- possible with a handful of outputs -- max |ref| is
    the size of GELU's tail (1e-8 and less), below the absolute error of ANY fp32 erf, and the bound says nothing about the sums: a case must hold an
    output of at least 1.  Decided by the float64 reference alone; head_cases draws such a case again with another seed."""
    return float(head_expected(c).abs().max()) >= 1.0


def images_differ(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bool [M, N]: elements that differ, an unwritten (NaN) element equal to another unwritten one."""
    if a.dtype == torch.float32:
        return a.view(torch.int32) != b.view(torch.int32)
    return a != b


def head_tiles(c: HeadCase):
    """The kernel's 128-row tiles of the UNCOMPACTED rows m, and the 128-column slices."""
    return ([torch.arange(m, min(m + 128, c.M), device=c.A.device) for m in range(0, c.M, 128)], [slice(n, min(n + 128, c.N)) for n in range(0, c.N, 128)])


def head_mutations(c: HeadCase):
    """-> list of (name, wrong image [M, N], [(image rows, column slice), ...] = where each 128 x 128 tile the mutation touches shows it).  Only the
    mutations that apply to the case's form are listed."""
    rt, ct = head_tiles(c)
    m = torch.arange(c.M, device=c.A.device)
    if c.epi == 4:
        sq, pos = m // c.period, m % c.period
        kept, orow = pos != c.period - 1, sq * (c.period - 1) + pos
    else:
        sq, pos, kept, orow = m * 0, m, m >= 0, m
    out = []

    def add(name, where, rows_of=orow, rows="last", **hooks):
        """where: bool [M] = the rows m the mutation changes; rows_of: the image row in which row m shows"""
        touched = [(rows_of[r[where[r]]], s) for r in rt if bool(where[r].any()) for s in ct]
        assert touched, name
        out.append((name, head_image(c, head_pre_activation(c, **hooks), rows), touched))

    three = c.W2 is not None
    if three:
        add("third sweep reads A2", kept, third_a=True)
        add("third sweep reads W", kept, third_w=True)
        add("second sweep reads W2", kept, second_w2=True)
    add("sweep boundary one K-tile early", kept, boundary=-1)
    add("sweep boundary one K-tile late", kept, boundary=1)
    if three and c.scale != 1.0:
        add("scale dropped", kept, no_scale=True)
        add("scale also applied to the bias", kept, scale_bias=True)
    if c.epi == 4:
        if c.per_pos and c.period > 2 and c.M > c.period:
            other = kept & (m >= c.period) & (pos != c.period - 2)                     # (rows whose wrong index is their own position are right)
            add("per-position bias indexed by m", other, bias_index="m")
            add("per-position bias indexed by the compacted row", other & (orow.clamp(max=c.period - 2) != pos), bias_index="orow")
        add("row 0 of each period dropped instead of the last", kept, rows="first")
        add("class row kept", m >= c.period - 1, rows_of=m, rows="keep")
        if c.M > c.period:
            add("compaction stride period", kept & (m >= c.period), rows_of=sq * c.period + pos, rows="stride")
    return out


HEAD_MUTATIONS = ("third sweep reads A2", "third sweep reads W", "second sweep reads W2", "sweep boundary one K-tile early", "sweep boundary one K-tile late",
                  "scale dropped", "scale also applied to the bias", "per-position bias indexed by m", "per-position bias indexed by the compacted row",
                  "row 0 of each period dropped instead of the last", "class row kept", "compaction stride period")


def head_cases(dev="cpu"):
    """Every exact case of the GPU file."""
    cases = []
    i = 0
    for M in HEAD_M:
        for N in HEAD_N:
            for kw in HEAD_KW:
                for three in (True, False):
                    seed = 300 + i
                    c = make_head_case(3, M, N, kw, three=three, scale=SCALES[i % 3], seed=seed, dev=dev)
                    while not gelu_case_is_meaningful(c):                               # (M = 1, N = 4: four outputs, all of which may be negative)
                        seed += 1000
                        c = make_head_case(3, M, N, kw, three=three, scale=SCALES[i % 3], seed=seed, dev=dev)
                    cases.append(c)
                    i += 1
    for M, period in LOGITS_SHAPES:
        if M % period:
            continue
        for per_pos in (False, True):
            for three in (True, False):
                N, kw = HEAD_N[i % 3], HEAD_KW[(i // 3) % 3]
                cases.append(make_head_case(4, M, N, kw, period=period, three=three, per_pos=per_pos, scale=SCALES[i % 3], seed=300 + i, dev=dev))
                i += 1
    return cases


# ---- real-valued data ---------------------------------------------------------------------------------------------------------------------------------
def real_inputs(seed=7):
    """-> (y fp32 [M, kw] rows for mb_layernorm, gamma, beta, W32 [N, kw] Gaussian with rows of different scale, bias [N])."""
    M, N, kw = REAL_SHAPE
    g = _gen(seed)
    y = torch.randn(M, kw, generator=g) * 1.7 + 0.3
    gamma, beta = torch.rand(kw, generator=g) + 0.5, torch.randn(kw, generator=g) * 0.2
    W = torch.randn(N, kw, generator=g) * 0.03 * (0.5 + 2.0 * torch.rand(N, 1, generator=g))
    return y, gamma, beta, W, torch.randn(N, generator=g) * 0.1


def ulp32(x: float) -> float:
    return 2.0 ** (math.frexp(abs(x))[1] - 24) if x else 2.0 ** -149


def real_reference(epi, x_hi, x_lo, W32, bias, w_hi, scale, rows=None):
    """-> (ref float64 [rows, N], E_hi, E_ref): the float64 result over the operands the kernel is given, x = x_hi + x_lo and the fp32 weight;
    E_hi = the largest error of the float64 product with the weights' hi plane ALONE; E_ref = that of a plain fp32 CPU matmul of the same operands.
    All CPU tensors; rows: the rows the launch keeps (epilogue 4 drops the class rows), all of them by default."""
    f = torch.nn.functional.gelu if epi == 3 else (lambda t: t)
    x = x_hi.double() + x_lo.double()
    if rows is not None:
        x = x[rows]
    ref = f(x @ W32.double().t() + bias.double())
    e_hi = float((f(x @ (w_hi.double() * float(scale)).t() + bias.double()) - ref).abs().max())
    e_ref = float((f(x.float() @ W32.t() + bias).double() - ref).abs().max())
    return ref, e_hi, e_ref


# ===== split planes =====================================================================================================================================
def _trunc_f16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp16 rounded towards zero (the mutation)."""
    h = x.half()
    over = h.float().abs() > x.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)       # one step down in magnitude: sign bit apart, the bits order like |h|


def split_planes(w: torch.Tensor, *, s_delta=0, lo_from_w=False, lo_trunc=False, first_pass_only=False, signed_max=False):
    """W fp32 [N, K] -> (hi fp16, lo fp16, scale fp32 scalar tensor): mx = max |w| = f 2^e with f in [0.5, 1), S = 15 - e (0 for an all-zero weight),
    hi = fp16_rne(w 2^S), lo = fp16_rne(w 2^S - hi) (the subtraction is exact in fp32), scale = 2^-S.  The keyword arguments are the mutations."""
    flat = w.reshape(-1)
    seen = flat[:GRID_PASS] if first_pass_only else flat
    mx = float(seen.max().clamp(min=0.0)) if signed_max else float(seen.abs().max())
    S = (15 - math.frexp(mx)[1] if mx > 0 else 0) + s_delta
    ws = w.double() * 2.0 ** S
    assert torch.equal(ws.float().double(), ws), "w * 2^S is no float32"
    ws = ws.float()
    hi = ws.clamp(-65504.0, 65504.0).half()
    rem = (w.double() if lo_from_w else ws.double()) - hi.double()
    if not lo_from_w:
        assert torch.equal(rem.float().double(), rem)
    rem = rem.float().clamp(-65504.0, 65504.0)
    return hi, (_trunc_f16(rem) if lo_trunc else rem.half()), torch.tensor(2.0 ** -S, dtype=torch.float32)


SPLIT_MUTATIONS = {"S one too large": dict(s_delta=1), "S one too small": dict(s_delta=-1), "lo computed from w": dict(lo_from_w=True),
                   "lo truncated": dict(lo_trunc=True), "maximum over the first grid pass only": dict(first_pass_only=True), "signed maximum": dict(signed_max=True)}


def split_inputs(N, K, seed=1):
    """-> list of (name, W fp32 [N, K], the mutations this input is built to catch)."""
    n = N * K
    g = _gen(seed + n)
    gauss = torch.randn(N, K, generator=g) * 0.03 * (0.5 + 2.0 * torch.rand(N, 1, generator=g))
    big = int(gauss.abs().argmax())
    always = ("S one too large", "S one too small")
    out = [("gaussian", gauss, always + (("lo computed from w", "lo truncated") if n >= 1024 else ())),
           ("all zero", torch.zeros(N, K), always)]

    def single(idx, v):
        w = torch.zeros(n)
        w[idx] = v
        return w.reshape(N, K)

    out += [("single first", single(0, 0.37), always + ("lo computed from w",)), ("single last", single(n - 1, -1.3e-3), always + ("signed maximum",))]
    if n > GRID_PASS:
        out.append(("single in the second pass", single(GRID_PASS + 4321, 11.0), always + ("maximum over the first grid pass only",)))
        far = gauss.clone()                                                             # the maximum, binades above the rest, beyond the first pass
        far.reshape(-1)[n - 77] = 3.0
        out.append(("gaussian, maximum in the second pass", far, always + ("maximum over the first grid pass only", "lo truncated")))
    neg = gauss.clone()
    neg.reshape(-1)[big] = -4.0 * gauss.abs().max()                                     # the maximum is negative and two binades above every positive value
    out.append(("negative maximum", neg, always + ("signed maximum",)))
    p2 = gauss.clone()
    p2.reshape(-1)[big] = 1.0
    out.append(("power-of-two maximum", p2, always))
    below = gauss.clone()
    below.reshape(-1)[big] = 1.0 - 2.0 ** -24                                           # one fp32 ulp below 1: S = 15, and the hi plane rounds it to 2^15
    out.append(("one ulp below a power of two", below, always))
    tiny = gauss.clone() * 2.0 ** -26                                                   # S = 14: w 2^S ~ 1e-5, below 2^-14: fp16-subnormal hi values
    tiny.reshape(-1)[big] = 1.0
    out.append(("far below the maximum", tiny, always))
    return out


# ===== cast =============================================================================================================================================
def cast_values(n, seed=3):
    """fp32 [n]: Gaussian values over fp16's whole range with the edge values cycled through the first elements and the LAST ones (the n % 4 tail)."""
    g = _gen(seed + n)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-26, 15, (n,), generator=g).float())
    t = 2.0 ** -24                                                                        # the smallest fp16 subnormal
    edge = torch.tensor([65504.0, -65504.0, 65520.0, -65520.0, 65519.996, 1e5, -1e5, float("inf"), float("-inf"), float("nan"), -0.0, 0.0,
                         t, -t, 0.5 * t, 1.5 * t, 2.5 * t, 0.5 * t * (1 + 2.0 ** -20), 1023.5 * t, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 2.0 ** -11 + 2.0 ** -23, 2049.0, 2051.0, 3.0e-8, 1e-40],
                        dtype=torch.float32)
    k = min(n, len(edge))
    x[:k] = edge[:k]
    if n > len(edge) + 8:
        x[-7:] = edge[torch.tensor([2, 9, 5, 17, 21, 0, 12])]
    elif n:
        x[-1] = edge[(n * 5) % len(edge)]
    return x


def cast_reference(x: torch.Tensor) -> torch.Tensor:
    return x.half()                                                                       # IEEE round to nearest even: 65520 and beyond -> inf, NaN stays NaN


def same_f16(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Bit-equal, any NaN equal to any NaN."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool((gn == wn).all()) and torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn])


# ===== e2m1 copies of a weight ============================================================================================================================
def w4_pack(codes: torch.Tensor, sbyte: torch.Tensor, *, row_major=False, no_swizzle=False, swap_nibbles=False):
    """codes 0..15 [N, K], one scale byte per (row, 128 columns) [N, K / 128] -> (bytes [N K / 2], scale bytes [N K / 128]) as mb_kernels.h states them.
    Elements (n, k), (n, k + 1), k even, share the byte ((n >> 4) (K >> 7) + (k >> 7)) 1024 + r 64 + ((c ^ ((r >> 1) & 3)) << 4) + ((k & 31) >> 1) with
    r = n & 15, c = (k & 127) >> 5 -- [N / 16][K / 128] chunks of 16 rows x 64 B, the 16-byte pieces of a row swizzled --, element k in the low nibble;
    the scale of (n, block j) is byte (((n >> 6) (K >> 7) + j) 16 + (n & 15)) 4 + ((n >> 4) & 3)."""
    N, K = codes.shape
    n, k = torch.meshgrid(torch.arange(N), torch.arange(0, K, 2), indexing="ij")
    r, c = n & 15, (k & 127) >> 5
    if row_major:
        off = n * (K // 2) + (k >> 1)
    else:
        off = ((n >> 4) * (K >> 7) + (k >> 7)) * 1024 + r * 64 + ((c if no_swizzle else c ^ ((r >> 1) & 3)) << 4) + ((k & 31) >> 1)
    lo, hi = (codes[:, 1::2], codes[:, 0::2]) if swap_nibbles else (codes[:, 0::2], codes[:, 1::2])
    w4 = torch.full((N * K // 2,), 0xA5, dtype=torch.uint8)
    w4[off.reshape(-1)] = (lo | (hi << 4)).to(torch.uint8).reshape(-1)
    n, j = torch.meshgrid(torch.arange(N), torch.arange(K // 128), indexing="ij")
    ws = torch.full((N * K // 128,), 0xA5, dtype=torch.uint8)
    ws[((((n >> 6) * (K >> 7) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3)).reshape(-1)] = sbyte.to(torch.uint8).reshape(-1)
    return w4, ws


def w4_unpack(w4: torch.Tensor, ws: torch.Tensor, N: int, K: int):
    """The inverse of w4_pack's true layout -> (codes [N, K], scale bytes [N, K / 128]) int64."""
    n, k = torch.meshgrid(torch.arange(N), torch.arange(0, K, 2), indexing="ij")
    r, c = n & 15, (k & 127) >> 5
    off = ((n >> 4) * (K >> 7) + (k >> 7)) * 1024 + r * 64 + ((c ^ ((r >> 1) & 3)) << 4) + ((k & 31) >> 1)
    b = w4.cpu().reshape(-1)[off].to(torch.int64)
    codes = torch.stack([b & 15, b >> 4], dim=-1).reshape(N, K)
    n, j = torch.meshgrid(torch.arange(N), torch.arange(K // 128), indexing="ij")
    return codes, ws.cpu().reshape(-1)[(((n >> 6) * (K >> 7) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3)].to(torch.int64)


def w4lo_reference(w: torch.Tensor, **layout):
    """W fp32 [N, K] (|w| inside fp16's range) -> (bytes, scale bytes) of the e2m1 copy of the fp16 rounding error e = w - fp16(w) (exact in fp32): per
    (row, 128 columns) mx = max |e|, E = the biased exponent with mx 2^(129 - E) in (3, 6], scale byte E - 2 and codes e2m1(e 2^(129 - E)); byte 0 and codes
    0 when E < 2 -- in particular for a block of fp16-representable weights."""
    N, K = w.shape
    e = (w.double() - w.half().double()).reshape(N, K // 128, 128)
    mx = e.abs().amax(-1)
    E = torch.where(mx > 0, f4_block_exponent(mx.clamp(min=2.0 ** -160)).to(torch.int64), torch.zeros_like(mx, dtype=torch.int64))
    live = E >= 2
    codes = torch.where(live[..., None], f4_codes(e * (2.0 ** (129 - E).double())[..., None]), torch.zeros_like(e, dtype=torch.int64))
    return w4_pack(codes.reshape(N, K), torch.where(live, E - 2, torch.zeros_like(E)), **layout)


def _w4_err(v: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """float64 squared quantisation error of blocks v [..., 128] at the scale exponents r [...]: sum (|v| - e2m1(|v| 2^r) 2^-r)^2."""
    m = (2.0 ** r.double())[..., None]
    a = v.abs() * m
    return (((a - _F4V[f4_codes(a)]) / m) ** 2).sum(-1)


def w4_choice(v: torch.Tensor):
    """Blocks v = fp16(w) [..., 128] float64 -> (r0, errors of the candidates r0 - 1, r0, r0 + 1 [..., 3], argmin r, decided): r0 = rint(log2(2.2 / rms))
    (0 for an all-zero block, clamped to +-100), the candidate with the smallest summed squared error wins (ties: the middle one, then the lower).
    decided: float64 settles the choice -- the two best errors differ by more than DECIDED_GAP relative and log2(2.2 / rms) is more than DECIDED_HALF
    from a half-integer -- or the block is all zero (every error is exactly 0 in any arithmetic: the middle candidate, r = 0)."""
    rms = (v ** 2).sum(-1).div(128.0).sqrt()
    zero = rms == 0
    l2 = torch.log2(2.2 / rms.clamp(min=1e-300))
    r0 = torch.where(zero, torch.zeros_like(l2), l2.round()).clamp(-100, 100).to(torch.int64)
    err = torch.stack([_w4_err(v, r0 + d) for d in (-1, 0, 1)], dim=-1)
    e0, e1, e2 = err.unbind(-1)
    best = torch.where((e1 <= e0) & (e1 <= e2), 1, torch.where(e0 <= e2, 0, 2))
    srt = err.sort(-1).values
    gap = (srt[..., 1] - srt[..., 0]) > DECIDED_GAP * srt[..., 1]
    half = ((l2 - torch.floor(l2)) - 0.5).abs() > DECIDED_HALF
    return r0, err, r0 - 1 + best, zero | (gap & half & ~zero)


def w4_emulate(w: torch.Tensor, *, from_w=False, block=128, byte_plus=False, nosat=False, **layout):
    """What a kernel that follows the contract in float64 writes: (bytes, scale bytes).  Mutations: quantise w instead of fp16(w); one scale per `block`
    = 64 / 256 columns; scale byte 127 + r; r from the block maximum without saturation; the layout hooks of w4_pack."""
    N, K = w.shape
    v16 = w.half().double()
    vb = v16.reshape(N, K // block, block)
    if nosat:
        mx = vb.abs().amax(-1)
        r = torch.where(mx > 0, 129 - f4_block_exponent(mx.clamp(min=2.0 ** -160)).to(torch.int64), torch.zeros_like(mx, dtype=torch.int64))
    elif block == 128:
        r = w4_choice(vb)[2]
    else:                                                                                 # (the rms and the errors of another block width)
        rms = (vb ** 2).sum(-1).div(block).sqrt()
        r0 = torch.where(rms == 0, torch.zeros_like(rms), torch.log2(2.2 / rms.clamp(min=1e-300)).round()).to(torch.int64)
        err = torch.stack([_w4_err(vb, r0 + d) for d in (-1, 0, 1)], dim=-1)
        r = r0 - 1 + torch.where((err[..., 1] <= err[..., 0]) & (err[..., 1] <= err[..., 2]), 1, torch.where(err[..., 0] <= err[..., 2], 0, 2))
    src = (w.double() if from_w else v16).reshape(N, K // block, block)
    codes = f4_codes(src * (2.0 ** r.double())[..., None]).reshape(N, K)
    r128 = r.repeat_interleave(2, 1) if block == 256 else r[:, 0::2] if block == 64 else r
    return w4_pack(codes, ((127 + r128) if byte_plus else (127 - r128)).clamp(0, 254), **layout)


def w4_check(w: torch.Tensor, w4: torch.Tensor, ws: torch.Tensor, label=""):
    """The e2m1 VALUE copy of W fp32 [N, K] against the contract -> (undecided share, blocks whose r is not the float64 argmin).  The kernel chooses r by
    fp32 sums and log2f, which at near-ties may legitimately differ from float64, so: r is read from the kernel's scale byte 127 - r; given r, every code
    must equal e2m1(fp16(w) 2^r) exactly; on a decided block (w4_choice) r must be the float64 argmin; on an undecided one r lies within r0 +- 2 and its
    float64 error within UNDECIDED_SLACK relative of the float64 minimum; at most MAX_UNDECIDED of the blocks are undecided."""
    N, K = w.shape
    codes, sb = w4_unpack(w4[: N * K // 2], ws[: N * K // 128], N, K)
    assert int(sb.min()) > 0 and int(sb.max()) < 254, f"{label}: scale byte at the clamp"
    r = 127 - sb
    v = w.half().double().reshape(N, K // 128, 128)
    want = f4_codes(v * (2.0 ** r.double())[..., None])
    bad = (want != codes.reshape(N, K // 128, 128)).nonzero()
    assert not len(bad), f"{label}: {len(bad)} codes are not e2m1(fp16(w) * 2^r) for the r of their scale byte, first (row, block, column) {bad[0].tolist()}"
    r0, err, best, decided = w4_choice(v)
    wrong = (decided & (r != best)).nonzero()
    assert not len(wrong), (f"{label}: {len(wrong)} decided blocks carry another r than the float64 argmin, first (row, block) {wrong[0].tolist()}: "
                            f"r {int(r[tuple(wrong[0])])}, argmin {int(best[tuple(wrong[0])])}")
    und = ~decided
    share = float(und.double().mean())
    assert share <= MAX_UNDECIDED, f"{label}: {share:.4f} of the blocks are undecided"
    if bool(und.any()):
        assert bool(((r - r0).abs()[und] <= 2).all()), f"{label}: an undecided block's r is outside r0 +- 2"
        assert bool((_w4_err(v, r)[und] <= err.amin(-1)[und] * (1 + UNDECIDED_SLACK)).all()), f"{label}: an undecided block's error is above the float64 minimum"
    return share, int((r != best).sum())


def w4lo_check(w: torch.Tensor, w4: torch.Tensor, ws: torch.Tensor, label=""):
    """Every byte of both arrays equals the statement."""
    N, K = w.shape
    want4, wants = w4lo_reference(w)
    got4, gots = w4[: N * K // 2].cpu().reshape(-1), ws[: N * K // 128].cpu().reshape(-1)
    bad = (got4 != want4).nonzero()
    assert not len(bad), f"{label}: {len(bad)} code bytes differ, first at byte {int(bad[0])}: {int(got4[bad[0]])} != {int(want4[bad[0]])}"
    bad = (gots != wants).nonzero()
    assert not len(bad), f"{label}: {len(bad)} scale bytes differ, first at byte {int(bad[0])}: {int(gots[bad[0]])} != {int(wants[bad[0]])}"


W4_LAYOUT_MUTATIONS = {"row-major layout": dict(row_major=True), "swizzle dropped": dict(no_swizzle=True), "nibble order swapped": dict(swap_nibbles=True)}
W4_MUTATIONS = {"quantise w instead of fp16(w)": dict(from_w=True), "one scale per 64 columns": dict(block=64), "one scale per 256 columns": dict(block=256),
                "scale byte 127 + r": dict(byte_plus=True), "saturation forbidden": dict(nosat=True), **W4_LAYOUT_MUTATIONS}

_MID = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)                                           # the midpoints of the e2m1 grid


def w4_inputs(N, K, seed=5):
    """-> list of (name, W fp32 [N, K], which copies it is for: "w4", "w4lo" or both)."""
    g = _gen(seed + N * K)
    gauss = torch.randn(N, K, generator=g) * 0.03 * (0.5 + 2.0 * torch.rand(N, 1, generator=g))
    z = torch.randn(N, K, generator=g)
    chi = (torch.randn(3, N, K, generator=g) ** 2).sum(0).div(3.0).sqrt()
    student = z / chi * 0.02 * (0.5 + 2.0 * torch.rand(N, 1, generator=g))
    out = [("gaussian", gauss, "both"), ("student-t(3)", student, "both")]
    h = gauss.clone()
    h[0::3] = h[0::3].half().float()                                                      # every third row exactly fp16: w4lo writes byte 0, codes 0
    out.append(("rows exactly fp16", h, "both"))
    zb = gauss.clone()
    zb[N // 2, K - 128:] = 0.0
    zb[0, :128] = 0.0
    out.append(("an all-zero block", zb, "both"))
    o = gauss.clone()
    for n in range(0, N, 7):
        j = (n // 7) % (K // 128)
        blk = o[n, 128 * j:128 * j + 128]
        blk[(n * 13) % 128] = 50.0 * blk.pow(2).mean().sqrt() * (1 if n % 2 else -1)
    out.append(("outlier 50 x rms", o, "both"))
    # the hardware converter's round-half-even, for w4lo: w = 1 + t 2^-14 with t on the e2m1 midpoints plus one 6: fp16(w) = 1, e = t 2^-14, the block's
    # maximum 6 2^-14 gives the multiplier 2^14 exactly, so every t lands ON a midpoint
    # (negative t up to 3.5 only: below 1 the fp16 grid is twice as fine, and 1 - 5 2^-14 no longer rounds to 1)
    t = torch.tensor(_MID + tuple(-x for x in _MID[:6]))[torch.randint(0, 13, (N, K), generator=g)]
    t[:, 5::128] = 6.0
    ties = (1.0 + t.double() * 2.0 ** -14).float()
    assert torch.equal(ties.double(), 1.0 + t.double() * 2.0 ** -14)
    out.append(("tie block", ties, "w4lo"))
    # the same for w4's "quantise w instead of fp16(w)": four elements per block a quarter fp16-ulp above a midpoint of the block's own scale, so that
    # fp16(w) lies ON the midpoint (rounds to even) while w itself lies above it (rounds up)
    s = gauss.clone()
    r = w4_choice(gauss.half().double().reshape(N, K // 128, 128))[2]
    sb = s.reshape(N, K // 128, 128)
    for i, mid in enumerate((0.25, 0.75, 1.25, 1.75)):
        sb[:, :, 17 + 29 * i] = ((mid * (1.0 + 2.0 ** -13)) * 2.0 ** (-r.double())).float() * (1 if i % 2 else -1)
    out.append(("a quarter ulp above the midpoints", s, "w4"))
    return out
