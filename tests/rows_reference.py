"""Reference for the row kernels of norm_embed.hip (embed_ln, embed_pair, ln_rows, ln_pair, pairify): CPU only, nothing here touches a GPU.

Three kinds of statement, and the checkers built from them (tests/test_hip_rows.py calls only the check_* functions, on device outputs copied to the CPU;
tests/test_rows_cpu.py proves that they tell wrong kernels from the right one):

* float64 statements of the embedding row (modeling/bert.py preprocess_tokens: bit projection + bias or table sum, class row LAST, a dropped label
  becomes class_emb[nclass], + pos_emb) and of LayerNorm.  Row values, mean and rstd of a kernel are compared with them inside a bound that is MEASURED
  per case: E_ref = the largest error of a plain fp32 restatement (torch two-pass LayerNorm; for the embedding the kernel's own chain of fp32 adds in
  front of it) on the same inputs, and the kernel must lie within max(4 E_ref, 2 fp32 ulp of the reference value).  The factor 4 covers what differs
  between the wave's xor-tree summation order + the hardware rsqrt (about 1 ulp) and torch's order and sqrt.  There is no bit-exact restatement of
  mean / rstd: they depend on the approximate rsqrt and on the compiler's fma contraction.
* EXACT functions of a kernel's own fp32 outputs, without tolerance: the fp16 copy, the fp16 lo halves, the pair operands, the e2m1 bytes with their
  lane-ordered scale bytes, and the row re-derived from {mean, rstd} by ln_affine's three explicit roundings (rows_from_stats).
* Every output buffer is filled with the byte 0xA5 and carries GUARD_ROWS rows / GUARD_BYTES bytes past its end; what a kernel must not write (guards,
  class-token rows of the e2m1 arrays, bytes d/2 .. 2d of an e2m1 row) must still hold it.
"""
from fractions import Fraction

import numpy as np
import torch

from hip_helpers import f4_block_exponent, f4_codes, f4_scale_index

SENT = 0xA5
GUARD_ROWS = 4
GUARD_BYTES = 256
H16_MAX = 65504.0
LN_EPS = 1e-12


class RowsMismatch(AssertionError):
    pass


# --------------------------------------------------------------------------- buffers
def alloc(rows: int, cols: int, dtype, device="cpu") -> torch.Tensor:
    """[rows + GUARD_ROWS, cols] of dtype, every byte SENT."""
    size = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((rows + GUARD_ROWS) * cols * size,), SENT, dtype=torch.uint8, device=device)
    return raw.view(dtype).reshape(rows + GUARD_ROWS, cols)


def scale_bytes(d: int, nseq: int, seq_rows: int) -> int:
    """Bytes of a lane-ordered scale array: one per (64-column block, token), groups = (seq_rows - 1) / 64 token groups of 64 per sequence."""
    return (d // 64) * nseq * ((seq_rows - 1) // 64) * 64


def alloc_scales(d: int, nseq: int, seq_rows: int, device="cpu") -> torch.Tensor:
    return torch.full((scale_bytes(d, nseq, seq_rows) + GUARD_BYTES,), SENT, dtype=torch.uint8, device=device)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Equal bit patterns (so that -0 != +0 and a NaN equals itself), else the first offending (row, column)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        raise RowsMismatch(f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}")
    ne = (_bits(got) != _bits(want)).reshape(got.shape[0], -1)
    if bool(ne.any()):
        r, c = (int(v) for v in ne.nonzero()[0])
        raise RowsMismatch(f"{what}: row {r}, column {c}: got {got.reshape(got.shape[0], -1)[r, c].item()!r}, want "
                           f"{want.reshape(got.shape[0], -1)[r, c].item()!r} ({int(ne.sum())} elements differ)")


def check_sentinel(region: torch.Tensor, what: str) -> None:
    """Every byte of `region` still SENT."""
    if region.numel() == 0:
        return
    b = region.contiguous()
    b = (b if b.dtype == torch.uint8 else b.view(torch.uint8)).reshape(region.shape[0], -1)
    ne = b != SENT
    if bool(ne.any()):
        r, c = (int(v) for v in ne.nonzero()[0])
        raise RowsMismatch(f"{what}: written at row {r}, byte {c} ({int(ne.sum())} bytes)")


def check_guard_rows(out: dict, rows: int, what: str) -> None:
    """Rows past `rows` of every row buffer of `out` and the bytes past the scale arrays' own are untouched."""
    for k, t in out.items():
        if t is None:
            continue
        if k in ("x4s", "xl4s"):
            check_sentinel(t[-GUARD_BYTES:].reshape(1, -1), f"{what}: guard bytes of {k}")
        else:
            check_sentinel(t[rows:], f"{what}: rows past {rows} of {k}")


# --------------------------------------------------------------------------- float64 statements
def embed_rows64(tokens, labels, drop, gbits, nclass, class_emb, pos, w_in=None, b_in=None, tables=None) -> torch.Tensor:
    """The pre-LayerNorm rows [nb, seq + 1, d] in float64.  tokens [nb, seq, m] with the mask token 2^gbits; w_in [d, m gbits] as the checkpoint holds
    it (channel g * gbits + j = bit j, LSB first, of group g: +1 set, -1 clear, 0 for the mask token), or tables [m, 2^gbits + 1, d]."""
    tokens = tokens.long()
    nb, seq, m = tokens.shape
    if tables is not None:
        x = sum(tables[g].double()[tokens[..., g]] for g in range(m))
    else:
        sign = (((tokens.unsqueeze(-1) >> torch.arange(gbits)) & 1) * 2 - 1).double()
        sign = torch.where((tokens == (1 << gbits)).unsqueeze(-1), torch.zeros_like(sign), sign)
        x = sign.reshape(nb, seq, m * gbits) @ w_in.double().t() + b_in.double()
    lab = labels.long().clone()
    if drop is not None:
        lab = torch.where(drop.bool(), torch.full_like(lab, nclass), lab)
    return torch.cat([x, class_emb.double()[lab].unsqueeze(1)], dim=1) + pos.double().reshape(1, seq + 1, -1)


def layernorm64(y, gamma, beta, eps=LN_EPS):
    """-> (rows, mean, rstd) in float64 over the last dimension."""
    y = y.double()
    mean = y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (y - mean) * rstd * gamma.double() + beta.double(), mean.squeeze(-1), rstd.squeeze(-1)


# --------------------------------------------------------------------------- plain fp32 restatements (for E_ref only)
def embed_rows32(tokens, labels, drop, gbits, nclass, class_emb, pos, w_in=None, b_in=None, tables=None) -> torch.Tensor:
    """The pre-LayerNorm rows in fp32, summed in the kernel's order: bias, then one fp32 add per bit channel (fma(+-1, w, e) = fp32(e +- w)), or
    0 + table row after table row; + pos last.  [nb, seq + 1, d]."""
    tokens = tokens.long()
    nb, seq, m = tokens.shape
    d = class_emb.shape[1]
    if tables is not None:
        e = torch.zeros(nb, seq, d, dtype=torch.float32)
        for g in range(m):
            e = e + tables[g].float()[tokens[..., g]]
    else:
        e = b_in.float().expand(nb, seq, d).clone()
        for g in range(m):
            live = (tokens[..., g] != (1 << gbits)).float().unsqueeze(-1)
            for j in range(gbits):
                sign = (((tokens[..., g] >> j) & 1) * 2 - 1).float().unsqueeze(-1) * live
                e = e + sign * w_in.float()[:, g * gbits + j]
    lab = labels.long().clone()
    if drop is not None:
        lab = torch.where(drop.bool(), torch.full_like(lab, nclass), lab)
    return torch.cat([e, class_emb.float()[lab].unsqueeze(1)], dim=1) + pos.float().reshape(1, seq + 1, d)


def layernorm32(y, gamma, beta, eps=LN_EPS):
    """torch fp32 two-pass LayerNorm -> (rows, mean, rstd), all fp32."""
    y = y.float()
    mean = y.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((y - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (y - mean) * rstd * gamma.float() + beta.float(), mean.squeeze(-1), rstd.squeeze(-1)


def ulp32(ref64: torch.Tensor) -> torch.Tensor:
    """The fp32 spacing at |ref| (float64)."""
    _, e = torch.frexp(ref64.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref64), e - 24)


class Figures(dict):
    """name -> (E_ref, kernel error, bound at the worst element) of one case; str() is a row of profiles/rows_kernels.md."""

    def __str__(self):
        return " | ".join(f"{k} {v[0]:.3e} {v[1]:.3e} {v[2]:.3e}" for k, v in self.items())


def check_bound(got32, ref64, plain32, what: str, figures: Figures = None, name: str = "x", e_ref: float = None) -> None:
    """|got - ref| <= max(4 E_ref, 2 ulp32(ref)) elementwise with E_ref = max |plain32 - ref| (or e_ref: measured over the whole input of a case of
    which this launch ran the first rows)."""
    ref64 = ref64.double()
    e_ref = float((plain32.double() - ref64).abs().max()) if e_ref is None else e_ref
    err = (got32.double() - ref64).abs()
    bound = torch.maximum(torch.full_like(ref64, 4.0 * e_ref), 2.0 * ulp32(ref64))
    bad = ~(err <= bound)                                          # (a NaN is bad)
    worst = int((err / bound).reshape(-1).nan_to_num(nan=float("inf")).argmax())
    if figures is not None:
        figures[name] = (e_ref, float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))
    if bool(bad.any()):
        b2 = bad.reshape(bad.shape[0], -1)
        r, c = (int(v) for v in b2.nonzero()[0])
        raise RowsMismatch(f"{what}: {name} row {r}, column {c}: got {float(got32.reshape(b2.shape)[r, c])!r}, float64 reference "
                           f"{float(ref64.reshape(b2.shape)[r, c])!r}, bound {float(bound.reshape(b2.shape)[r, c]):.3e} (E_ref {e_ref:.3e}; {int(bad.sum())} elements outside)")


# --------------------------------------------------------------------------- exact functions of a kernel's own fp32 outputs
def h16_of(x32: torch.Tensor) -> torch.Tensor:
    """mb_common.h to_h: clamp to the fp16 range, round to nearest even."""
    return x32.float().clamp(-H16_MAX, H16_MAX).half()


def lo32_of(x32: torch.Tensor) -> torch.Tensor:
    """x - float(fp16(x)) in fp32 (exact: the difference is representable)."""
    return x32.float() - h16_of(x32).float()


def lo_of(x32: torch.Tensor) -> torch.Tensor:
    return h16_of(lo32_of(x32))


def pair_operands(xc32: torch.Tensor, xu32: torch.Tensor):
    """(fp16(x_c), fp16(x_u - x_c)) with the difference in fp32."""
    return h16_of(xc32), h16_of(xu32.float() - xc32.float())


def _round_f32(fr: Fraction) -> np.float32:
    """The fp32 nearest to an exact rational, ties to even."""
    c = np.float32(float(fr))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda z: (abs(Fraction(float(z)) - fr), int(np.float32(z).view(np.uint32)) & 1))


def rows_from_stats(y, mean, rstd, gamma, beta) -> torch.Tensor:
    """mb_common.h ln_affine on rows y [R, d] with per-row mean / rstd [R]: fp32(fp32(y - mean) * rstd), then ONE fused multiply-add with gamma and
    beta.  The two fp32 roundings are torch's; the product u * gamma is exact in float64, and so is the fma wherever the float64 sum does not lie
    within one float64 ulp of an fp32 rounding midpoint -- those few elements are decided in rational arithmetic."""
    u = (y.float() - mean.float().unsqueeze(-1)) * rstd.float().unsqueeze(-1)
    g64, b64 = gamma.double().expand_as(u), beta.double().expand_as(u)
    s = u.double() * g64 + b64
    out = s.float()
    low = s.view(torch.int64) & ((1 << 29) - 1)
    doubt = (((low - (1 << 28)).abs() <= 1) | ((s.abs() < 2.0 ** -100) & (s != 0))) & torch.isfinite(s)
    for r, c in doubt.nonzero().tolist():
        out[r, c] = float(_round_f32(Fraction(float(u[r, c])) * Fraction(float(g64[r, c])) + Fraction(float(b64[r, c]))))
    return out


def f4_expected(v32: torch.Tensor, nseq: int, seq_rows: int):
    """The e2m1 copy of fp32 rows v32 [nseq * seq_rows, d] as fp4_row_store writes it -> (bytes uint8 [R, d / 2], scale bytes int64 [R, d / 64], their
    index in the lane-ordered array int64 [R, d / 64], keep bool [R]: False on the class-token rows, which receive nothing).  One scale per 64 columns
    from the block's largest element WITHOUT saturation (amax * 2^(129 - E) in (3, 6]); an all-zero block has scale byte 0 and codes 0."""
    v = v32.double()
    R, d = v.shape
    assert R == nseq * seq_rows and d % 64 == 0 and (seq_rows - 1) % 64 == 0
    blocks = v.reshape(R, d // 64, 64)
    amax = blocks.abs().amax(-1)
    E = torch.where(amax > 0, f4_block_exponent(amax.clamp(min=1e-300)).to(torch.int64), torch.zeros_like(amax, dtype=torch.int64))
    mul = torch.where((E >= 2) & (E <= 254), 2.0 ** (129 - E).double(), torch.zeros_like(amax))
    codes = f4_codes(blocks * mul.unsqueeze(-1)).reshape(R, d)
    want = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    rows = torch.arange(R)
    seq, tok = rows // seq_rows, rows % seq_rows
    groups = (seq_rows - 1) // 64
    idx = torch.stack([f4_scale_index(b, nseq, seq, tok.clamp(max=seq_rows - 2), groups) for b in range(d // 64)], dim=1)
    return want, (E - 2).clamp(min=0), idx, tok < seq_rows - 1


def check_f4(x4: torch.Tensor, x4s: torch.Tensor, v32: torch.Tensor, nseq: int, seq_rows: int, what: str) -> None:
    """x4 uint8 [R + guard, 2 d] and x4s (lane-ordered scale bytes + guard) are EXACTLY the e2m1 copy of v32 [R, d]: token rows' first d / 2 bytes, every
    scale byte at its index; bytes d / 2 .. 2 d of every row, whole class-token rows and the guards still hold the sentinel."""
    R, d = v32.shape
    want, sbyte, idx, keep = f4_expected(v32, nseq, seq_rows)
    full = torch.full((R, 2 * d), SENT, dtype=torch.uint8)
    full[:, : d // 2] = torch.where(keep.unsqueeze(-1), want, torch.full_like(want, SENT))
    check_sentinel(x4[:R][~keep], f"{what}: class-token rows of the e2m1 array")
    check_sentinel(x4[:R, d // 2:], f"{what}: bytes d/2 .. 2d of the e2m1 rows")
    check_bits(x4[:R], full, f"{what}: e2m1 bytes")
    check_sentinel(x4[R:], f"{what}: rows past {R} of the e2m1 array")
    scales = torch.full_like(x4s, SENT)
    assert x4s.numel() == scale_bytes(d, nseq, seq_rows) + GUARD_BYTES
    scales[idx[keep].reshape(-1)] = sbyte[keep].reshape(-1).to(torch.uint8)
    check_sentinel(x4s[-GUARD_BYTES:].reshape(1, -1), f"{what}: guard bytes of the scale array")
    check_bits(x4s.reshape(1, -1), scales.reshape(1, -1), f"{what}: lane-ordered scale bytes (row 0, column = byte index)")


def check_copies(out: dict, rows: int, nseq: int, seq_rows: int, what: str, x32: torch.Tensor = None) -> None:
    """The copies of the fp32 rows a kernel wrote (out['x32'], or x32 where the kernel keeps them in registers): xh = fp16, xlo = lo halves, x4 / x4s =
    e2m1 of the values, xl4 / xl4s = e2m1 of the fp32 lo halves -- all exact."""
    x32 = out["x32"][:rows] if x32 is None else x32
    if out.get("xh") is not None:
        check_bits(out["xh"][:rows], h16_of(x32), f"{what}: x_h16 against fp16(x_f32)")
    if out.get("xlo") is not None:
        check_bits(out["xlo"][:rows], lo_of(x32), f"{what}: x_lo against fp16(x_f32 - fp16(x_f32))")
    if out.get("x4") is not None:
        check_f4(out["x4"], out["x4s"], x32, nseq, seq_rows, f"{what}: values")
    if out.get("xl4") is not None:
        check_f4(out["xl4"], out["xl4s"], lo32_of(x32), nseq, seq_rows, f"{what}: lo halves")


# --------------------------------------------------------------------------- one checker per kernel
def layernorm_e_ref(y, gamma, beta, eps=LN_EPS) -> dict:
    """E_ref of x / mean / rstd over ALL rows of a case's input y: the largest error of the plain fp32 restatement against float64."""
    ref, mean, rstd = layernorm64(y, gamma, beta, eps)
    p32, pm, pr = layernorm32(y, gamma, beta, eps)
    return {k: float((a.double() - b).abs().max()) for k, a, b in (("x", p32, ref), ("mean", pm, mean), ("rstd", pr, rstd))}


def check_layernorm(out: dict, y, gamma, beta, eps, M: int, what: str, nseq: int = 0, seq_rows: int = 0, figures: Figures = None, e_ref: dict = None) -> None:
    """ln_rows_kernel with every output present: out = {x32, xh, xlo?, stats?, x4 / x4s?, xl4 / xl4s?} of M rows (+ guards) from y [M, d].  e_ref
    (layernorm_e_ref of the case's whole input): for launches over the first M rows of a larger case -- the maximum over one or three rows of a
    rounding error that is as good as random says little about fp32's error on that input, the maximum over the case's rows does."""
    e_ref = e_ref or {}
    y = y[:M]
    check_guard_rows(out, M, what)
    check_copies(out, M, nseq, seq_rows, what)
    ref, mean, rstd = layernorm64(y, gamma, beta, eps)
    p32, pm, pr = layernorm32(y, gamma, beta, eps)
    if out.get("stats") is not None:
        st = out["stats"][:M]
        check_bits(out["x32"][:M], rows_from_stats(y, st[:, 0], st[:, 1], gamma, beta), f"{what}: x_f32 against ln_affine(y, own stats)")
        check_bound(st[:, :1], mean.unsqueeze(-1), pm.unsqueeze(-1), what, figures, "mean", e_ref.get("mean"))
        check_bound(st[:, 1:], rstd.unsqueeze(-1), pr.unsqueeze(-1), what, figures, "rstd", e_ref.get("rstd"))
    check_bound(out["x32"][:M], ref, p32, what, figures, "x", e_ref.get("x"))


def check_pair(out: dict, y, gamma, beta, eps, P: int, what: str, nseq: int = 0, seq_rows: int = 0, figures: Figures = None) -> None:
    """ln_pair_kernel with stats: out = {xh [2 P], stats [2 P], e2m1 set?} from y [2 P, d]: conditional rows = fp16(ln_affine(y_r, stats_r)), twin rows =
    fp16(ln_affine(y_{r+P}, stats_{r+P}) - that) in fp32, the e2m1 set from the conditional rows alone; both rows' stats against float64."""
    y = y[:2 * P]
    check_guard_rows(out, 2 * P, what)
    st = out["stats"][:2 * P]
    x = rows_from_stats(y, st[:, 0], st[:, 1], gamma, beta)
    hc, hu = pair_operands(x[:P], x[P:])
    check_bits(out["xh"][:P], hc, f"{what}: conditional rows against fp16(ln_affine(y, own stats))")
    check_bits(out["xh"][P:2 * P], hu, f"{what}: twin rows against fp16(x_u - x_c)")
    _check_pair_f4(out, x[:P], P, nseq, seq_rows, what)
    ref, mean, rstd = layernorm64(y, gamma, beta, eps)
    _, pm, pr = layernorm32(y, gamma, beta, eps)
    check_bound(st[:, :1], mean.unsqueeze(-1), pm.unsqueeze(-1), what, figures, "mean")
    check_bound(st[:, 1:], rstd.unsqueeze(-1), pr.unsqueeze(-1), what, figures, "rstd")


def _check_pair_f4(out, xc32, P, nseq, seq_rows, what):
    """The e2m1 arrays of a pair kernel hold the CONDITIONAL rows' copies in rows [0, P); rows [P, 2 P) (the twins) and the guards are untouched."""
    for k, v in (("x4", xc32), ("xl4", lo32_of(xc32))):
        if out.get(k) is not None:
            a = out[k]
            check_sentinel(a[P:], f"{what}: twin rows of {k}")
            check_f4(torch.cat([a[:P], a[-GUARD_ROWS:]]), out[k + "s"], v, nseq, seq_rows, f"{what}: {k}")


def check_pairify(out: dict, x32, P: int, what: str, nseq: int = 0, seq_rows: int = 0) -> None:
    """pairify_kernel is a pure function of x32 [2 P, d]: every output exactly."""
    check_guard_rows(out, 2 * P, what)
    hc, hu = pair_operands(x32[:P], x32[P:2 * P])
    check_bits(out["xh"][:P], hc, f"{what}: conditional rows against fp16(x_c)")
    check_bits(out["xh"][P:2 * P], hu, f"{what}: twin rows against fp16(x_u - x_c)")
    _check_pair_f4(out, x32[:P].float(), P, nseq, seq_rows, what)


def check_embed(out: dict, case: dict, drop, what: str, figures: Figures = None) -> None:
    """embed_ln_kernel: out = {x32, xh, xlo?, e2m1 set?} of nb (seq + 1) rows; case = the arguments of embed_rows64 + gamma, beta."""
    args = {k: case.get(k) for k in ("gbits", "nclass", "class_emb", "pos", "w_in", "b_in", "tables")}
    nb, seq, _ = case["tokens"].shape
    M = nb * (seq + 1)
    d = case["class_emb"].shape[1]
    check_guard_rows(out, M, what)
    check_copies(out, M, nb, seq + 1, what)
    ref, _, _ = layernorm64(embed_rows64(case["tokens"], case["labels"], drop, **args).reshape(M, d), case["gamma"], case["beta"])
    p32, _, _ = layernorm32(embed_rows32(case["tokens"], case["labels"], drop, **args).reshape(M, d), case["gamma"], case["beta"])
    check_bound(out["x32"][:M], ref, p32, what, figures, "x")


def check_embed_pair(out: dict, two: dict, case: dict, what: str) -> None:
    """embed_pair_kernel over nb conditional sequences against the two-kernel path on the same inputs (`two` = x32 / xh / e2m1 set that embed_ln over
    [conditional | label-dropped twins] followed by pairify wrote): equal bit for bit (mb_kernels.h), and by construction the twin half of x_h16 is
    all zero bits on image-token rows and on class rows whose label is nclass itself; any other class row differs from its twin."""
    nb, seq, _ = case["tokens"].shape
    N, P = seq + 1, nb * (seq + 1)
    check_guard_rows(out, 2 * P, what)
    for k in ("x32", "xh", "x4", "x4s", "xl4", "xl4s"):
        if (out.get(k) is None) != (two.get(k) is None):
            raise RowsMismatch(f"{what}: {k} present in one path only")
        if out.get(k) is not None:
            a, b = (t.reshape(1, -1) if t.dim() == 1 else t for t in (out[k], two[k]))
            check_bits(a, b, f"{what}: {k} against embed_ln + pairify")
    twin = out["xh"][P:2 * P].reshape(nb, N, -1)
    zero = torch.zeros_like(twin[:, :seq])
    check_bits(twin[:, :seq].reshape(nb * seq, -1), zero.reshape(nb * seq, -1), f"{what}: twin operand of the image-token rows (row = sequence * seq + token)")
    same = case["labels"].long() == case["nclass"]
    for s in range(nb):
        nz = bool((_bits(twin[s, seq]) != 0).any())
        if bool(same[s]) and nz:
            raise RowsMismatch(f"{what}: sequence {s}: label == nclass, yet its class-row difference is not zero")
        if not bool(same[s]) and not nz:
            raise RowsMismatch(f"{what}: sequence {s}: the class-row difference is zero although the labels differ")
    check_bits(out["x32"][P:2 * P].reshape(nb, N, -1)[:, :seq].reshape(nb * seq, -1), out["x32"][:P].reshape(nb, N, -1)[:, :seq].reshape(nb * seq, -1),
               f"{what}: x_f32 of the twins' image-token rows against the conditional rows")
