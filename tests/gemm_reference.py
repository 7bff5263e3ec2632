"""Exact-operand references of the trunk GEMM family (gemm.hip, gemm_ht.hip), shared by tests/test_gemm_exact_cpu.py and tests/test_hip_gemm_exact.py.

The method: operands are small INTEGERS held in fp16 (A in -3..3, the lo halves A2 and the pair difference rows in -2..2, W in -2..2, integer bias and
residual).  With K <= 4096 every partial sum is an integer below 2^15, so an fp32 accumulator holds it exactly whatever the order of the additions: the
kernel's output must EQUAL the float64 result, bit for bit, and a fragment read from the wrong lane, row, K-tile or sequence cannot hide inside a
tolerance.  The MX-fp4 mini-tile operands are e2m1 grid values times a power of two per block (scale bytes 125..129); there the same argument needs
sum |a| |w| below 2^22 quanta, which `mini_precondition` checks.  `mutations` lists the wrong kernels this net is meant to catch, as wrong references:
the CPU file proves that each of them changes the expected output in every tile it touches (the generators have no blind spot).
A plain module: no fixtures, nothing here touches the GPU unless it is handed GPU tensors."""
from dataclasses import dataclass, field, replace
from typing import List, Optional

import torch

from hip_helpers import _F4V, f4_encode_rows, w4_decode

F16_MAX = 65504.0
EXACT_EPIS = (0, 2, 4)                       # the epilogues whose output is the exact sum (1 and 3 apply GELU)

# ---- the shapes of the GPU file (the CPU file walks the same families) -------------------------------------------------------------------------
KS = (128, 192, 320, 1024)
SMALL_M, SMALL_N = (1, 127, 129, 257, 600), (4, 132, 256)                     # the 128 x 128 kernel (variant -1)
LOGITS_SHAPES = ((600, 257), (2313, 257), (1025, 1025), (2050, 1025))         # (M, period) of epilogue 4
HT_SHAPES = ((512, 256, 128), (513, 512, 192), (771, 768, 320), (1288, 512, 1024), (2313, 768, 128), (4369, 768, 192))    # (M, N, K), half-tile kernel
HT_VARIANTS = (6, 8, 257, 0)
CU_COUNTS = (0, 1, 3, 13)                    # walk lengths: 1, all tiles, ragged tails that are no multiple of the 8 XCDs
# sequence tiles: (pair, sequences (pairs), seq_rows, N, K, nlo)
SEQ_SHAPES = ((0, 3, 257, 512, 192, 0), (0, 3, 257, 768, 128, 1), (0, 1, 257, 256, 1024, 1), (0, 2, 1025, 256, 320, 0), (0, 1, 1025, 256, 128, 1),
              (0, 18, 1025, 256, 128, 1),
              (1, 2, 257, 512, 320, 0), (1, 3, 257, 768, 128, 1), (1, 2, 257, 256, 1024, 2), (1, 1, 1025, 512, 192, 0), (1, 1, 1025, 256, 128, 1),
              (1, 2, 1025, 256, 128, 2))
MINI_SPLIT_SHAPES = ((3, 512, 128), (2, 256, 1024))                             # (sequences, N, kw) of mb_gemm_mini_split


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def int_operand(rows: int, cols: int, lim: int, seed: int) -> torch.Tensor:
    """Integers in -lim..lim [rows, cols] (int64, CPU), cols % 64 == 0.  Every (16-row group, 64-column K-tile) has its own distribution (share of zeros
    0 .. 42 %, odd modes lean positive); no K-tile of any single row is all zero."""
    g = _gen(seed)
    v = torch.randint(-lim, lim + 1, (rows, cols), generator=g)
    u = torch.rand((rows, cols), generator=g)
    mode = (3 * (torch.arange(rows) // 16)[:, None] + 5 * (torch.arange(cols) // 64)[None, :]) % 7
    v = torch.where(u < 0.07 * mode, torch.zeros_like(v), v)
    v = torch.where(((mode & 1) == 1) & (u > 0.8), v.abs(), v)
    blocks = v.reshape(rows, cols // 64, 64)
    dead = blocks.abs().sum(-1) == 0
    blocks[..., 0][dead] = lim
    return blocks.reshape(rows, cols)


def int_values(shape, lim: int, seed: int) -> torch.Tensor:
    return torch.randint(-lim, lim + 1, shape, generator=_gen(seed)).float()


# ---- e2m1 operands of the mini-tile passes ---------------------------------------------------------------------------------------------------------
def f4_grid_operand(rows: int, K: int, block: int, seed: int):
    """-> (codes 0..15 [rows, K], block exponents e in -2..2 [rows, K / block], values float64 = e2m1(code) * 2^e).  Half of the entries are zero; element 0
    of every 64-column block is +-4 or +-6, so the block maximum lies in (3, 6] * 2^e and the producers' rule (mb_common.h) gives exactly the scale
    byte 127 + e: 125..129."""
    g = _gen(seed)
    idx = torch.randint(1, 8, (rows, K), generator=g)
    idx = torch.where(torch.rand((rows, K), generator=g) < 0.5, idx, torch.zeros_like(idx))
    idx[:, 0::64] = torch.randint(6, 8, (rows, K // 64), generator=g)
    codes = idx | (torch.randint(0, 2, (rows, K), generator=g) << 3)
    e = torch.randint(-2, 3, (rows, K // block), generator=g)
    return codes, e, _F4V[codes] * (2.0 ** e.double()).repeat_interleave(block, 1)


def w4_encode(codes: torch.Tensor, sbyte: torch.Tensor):
    """The inverse of hip_helpers.w4_decode: e2m1 codes [N, K] + one scale byte per (row, 128 K-elements) -> (mini-tile-packed bytes [N K / 2], lane-ordered
    scale bytes [N K / 128])."""
    N, K = codes.shape
    nn, kk = torch.meshgrid(torch.arange(N), torch.arange(0, K, 2), indexing="ij")
    r, c = nn & 15, (kk & 127) >> 5
    off = ((nn >> 4) * (K >> 7) + (kk >> 7)) * 1024 + r * 64 + ((c ^ ((r >> 1) & 3)) << 4) + ((kk & 31) >> 1)
    w4 = torch.zeros(N * K // 2, dtype=torch.uint8)
    w4[off.reshape(-1)] = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).reshape(-1)
    n, j = torch.meshgrid(torch.arange(N), torch.arange(K // 128), indexing="ij")
    ws = torch.zeros(N * K // 128, dtype=torch.uint8)
    ws[((((n >> 6) * (K // 128) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3)).reshape(-1)] = sbyte.to(torch.uint8).reshape(-1)
    return w4, ws


@dataclass
class MiniSet:
    """One MX-fp4 operand set: what the kernel reads (x4, xs, w4, ws) and what it is asked to compute with (a_dec [rows, K] with zero class-token rows,
    w_dec [N, K], float64); a_val / a_e: the grid values and block exponents, for the scale mutation."""
    x4: torch.Tensor
    xs: torch.Tensor
    w4: torch.Tensor
    ws: torch.Tensor
    a_dec: torch.Tensor
    w_dec: torch.Tensor
    a_val: torch.Tensor
    a_e: torch.Tensor

    def tensors(self):
        return (self.x4, self.xs, self.w4, self.ws)


def make_mini_set(nseq: int, seq_rows: int, N: int, K: int, seed: int, dev="cpu") -> MiniSet:
    R = nseq * seq_rows
    codes, e, v = f4_grid_operand(R, K, 64, seed)
    x4, xs, dec = f4_encode_rows(v, nseq, dev="cpu", seq_rows=seq_rows)
    tok = (torch.arange(R) % seq_rows) < seq_rows - 1
    assert torch.equal(dec[tok], v[tok]), "the token operand is not on the e2m1 grid of the producers' own scale"
    assert not bool(dec[~tok].any())
    wc, we, wv = f4_grid_operand(N, K, 128, seed + 1)
    w4, ws = w4_encode(wc, 127 + we)
    assert torch.equal(w4_decode(w4, ws, N, K), wv), "w4_encode is not the inverse of w4_decode"
    val = (_F4V[codes]).clone()
    val[~tok] = 0.0
    pad = torch.zeros(4096, dtype=torch.uint8)                                  # (slack behind the weight operand, as the other tests' buffers have)
    return MiniSet(x4.to(dev), xs.to(dev), torch.cat([w4, pad]).to(dev), torch.cat([ws, pad]).to(dev), dec.to(dev), wv.to(dev), val.to(dev), e.to(dev))


# ---- a case: the operands of one launch ---------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    epi: int
    M: int                                   # rows of A and of the (uncompacted) output; pair: 2 * pair_rows
    N: int
    K: int                                   # K extent of one sweep (split activations: kw, the kernel's K is twice that)
    A: torch.Tensor                          # fp16 [M, K]
    W: torch.Tensor                          # fp16 [N, K]
    bias: torch.Tensor                       # fp32 [N]
    res: Optional[torch.Tensor] = None       # fp32 [M, N] (epilogue 2)
    A2: Optional[torch.Tensor] = None        # fp16 [M, K]: the lo halves of split activations
    period: int = 0                          # epilogue 4: every period-th row is dropped
    seq_rows: int = 0                        # sequence tiles: rows per sequence, class token last (0: no sequence structure)
    pair_rows: int = 0                       # pair tiles: conditional rows
    lo: List[MiniSet] = field(default_factory=list)

    @property
    def rows_c(self):
        return self.pair_rows or self.M

    @property
    def nseq(self):
        return self.rows_c // self.seq_rows if self.seq_rows else 0

    def with_epi(self, epi):
        return replace(self, epi=epi)


def make_case(epi, M, N, K, *, split=False, period=0, seq_rows=0, pair=False, nlo=0, seed=1, dev="cpu") -> Case:
    """M: rows (sequence tiles: sequences * seq_rows; pair: the CONDITIONAL rows, A and the output get twice as many)."""
    assert K % 64 == 0 and K <= 4096
    a = int_operand(M, K, 3, seed)
    if pair:
        a = torch.cat([a, int_operand(M, K, 2, seed + 7)])
    rows = a.shape[0]
    c = Case(epi, rows, N, K, a.half().to(dev), int_operand(N, K, 2, seed + 1).half().to(dev), int_values((N,), 8, seed + 2).to(dev),
             res=int_values((rows, N), 16, seed + 3).to(dev), period=period, seq_rows=seq_rows, pair_rows=M if pair else 0)
    if split:
        c.A2 = int_operand(M, K, 2, seed + 4).half().to(dev)
    c.lo = [make_mini_set(M // seq_rows, seq_rows, N, K, seed + 10 + 2 * i, dev) for i in range(nlo)]
    return c


def mini_precondition(c: Case) -> float:
    """sum |a| |w| over EVERYTHING an output element's fp32 accumulator receives (fp16 products, mini-tile products, bias, residual), in units of the smallest
    decoded quantum 2^-6 (e2m1 step 1/2 * 2^-2, squared); asserts it is below 2^22, i.e. every partial sum in any order is a multiple of the quantum
    below 2^24 quanta: exact in fp32, so the float64 result is what any fp32 order gives.  Returns the largest value in quanta."""
    P = c.rows_c
    A = c.A.double().abs()
    tot = (A[:P] + (c.A2.double().abs() if c.A2 is not None else 0) + (A[P:] if c.pair_rows else 0)) @ c.W.double().abs().t() + c.bias.double().abs()
    for s in c.lo:
        assert int(s.a_e.min()) >= -2 and int(s.a_e.max()) <= 2                # scale bytes 125..129
        tot = tot + s.a_dec.abs() @ s.w_dec.abs().t()
    if c.res is not None:
        tot = tot + (c.res[:P].double().abs() + (c.res[P:].double().abs() if c.pair_rows else 0))
    worst = float(tot.max()) * 64.0
    assert worst < 2.0 ** 22, worst
    return worst


# ---- float64 references ----------------------------------------------------------------------------------------------------------------------------------
def _ktile(x, t):
    return x[:, t * 64:(t + 1) * 64]


def class_rows(c: Case) -> torch.Tensor:
    """Rows of A / the output that are class-token rows (pair: of both halves)."""
    r = torch.arange(c.nseq, device=c.A.device) * c.seq_rows + c.seq_rows - 1
    return torch.cat([r, r + c.pair_rows]) if c.pair_rows else r


def pre_activation(c: Case, *, ktile_delta=(), lo_reads_hi=False, cls_shift=False, no_delta=False, scale_shift=None, skip_half=False, bias_shift=False):
    """float64 [M, N]: what the accumulators + bias hold before the epilogue.  The keyword arguments are the hooks of `mutations`; the default is the truth."""
    A, W = c.A.double(), c.W.double()
    A2 = c.A2.double() if c.A2 is not None else None
    if cls_shift:                                                               # class row of sequence s + 1 (cyclic)
        cls = class_rows(c)
        src = torch.cat([cls[:c.nseq].roll(-1), cls[c.nseq:].roll(-1)])
        A = A.clone()
        A[cls] = c.A.double()[src]
        if A2 is not None:
            A2 = A2.clone()
            A2[cls] = c.A2.double()[src]
    acc = (A + (A if lo_reads_hi else A2) if A2 is not None else A) @ W.t()
    for sign, src, ta, tw in ktile_delta:                                       # + / - one K-tile product: A (0) / A2 (1) tile ta against W tile tw
        acc = acc + sign * (_ktile(A2 if src else A, ta) @ _ktile(W, tw).t())
    P = c.rows_c
    corr = torch.zeros(P, c.N, dtype=torch.float64, device=A.device)
    for i, s in enumerate(c.lo):
        a_dec = s.a_dec
        if scale_shift == i:                                                    # the scales of the 64-token group g + 1 (cyclic inside the sequence)
            rows = torch.arange(P, device=A.device)
            sq, tok = rows // c.seq_rows, rows % c.seq_rows
            other = sq * c.seq_rows + torch.where(tok < c.seq_rows - 1, (tok + 64) % (c.seq_rows - 1), tok)
            a_dec = s.a_val * (2.0 ** s.a_e[other].double()).repeat_interleave(64, 1)
        ci = a_dec @ s.w_dec.t()
        if skip_half:
            tok = torch.arange(P, device=A.device) % c.seq_rows
            ci[(tok % 256) >= 128] = 0.0
        corr = corr + ci
    bias = c.bias.double()
    if bias_shift:                                                              # the previous column block's bias (n0 - 256)
        bias = torch.cat([bias[:256], bias[:-256]])
    if c.pair_rows:
        pc = acc[:P] + corr + bias
        return torch.cat([pc, pc if no_delta else pc + acc[P:]])
    return acc + corr + bias


def to_f16(x: torch.Tensor) -> torch.Tensor:
    """The fp16 store: clamp to +-65504, round to nearest even."""
    return x.clamp(-F16_MAX, F16_MAX).to(torch.float16)


def finish(c: Case, pre: torch.Tensor) -> torch.Tensor:
    """The epilogue on a float64 pre-activation -> the uncompacted output [M, N]: fp16 (epi 0) or fp32 (2, 4) bits for the exact epilogues, float64
    GELU values (1, 3; pair: the u rows are gelu(u) - gelu(c)) to compare within the GELU bound."""
    if c.epi == 0:
        return to_f16(pre)
    if c.epi == 2:
        return (pre + c.res.double()).to(torch.float32)
    if c.epi == 4:
        return pre.to(torch.float32)
    g = torch.nn.functional.gelu(pre)
    if c.pair_rows:
        P = c.pair_rows
        g = torch.cat([g[:P], g[P:] - g[:P]])
    return g


def kept_rows(c: Case) -> torch.Tensor:
    r = torch.arange(c.M, device=c.A.device)
    return r[r % c.period != c.period - 1] if c.epi == 4 else r


def expected(c: Case, **hooks) -> torch.Tensor:
    """What the launch must write (epilogue 4: compacted)."""
    out = finish(c, pre_activation(c, **hooks))
    return out[kept_rows(c)] if c.epi == 4 else out


def einsum_reference(c: Case) -> torch.Tensor:
    """The same pre-activation written separately and plainly (the CPU file compares the two)."""
    A, W = c.A.double(), c.W.double()
    P = c.rows_c
    y = torch.einsum("mk,nk->mn", A[:P], W)
    if c.A2 is not None:
        y = y + torch.einsum("mk,nk->mn", c.A2.double(), W)
    for s in c.lo:
        y = y + torch.einsum("mk,nk->mn", s.a_dec, s.w_dec)
    y = y + c.bias.double()[None, :]
    if c.pair_rows:
        y = torch.cat([y, y + torch.einsum("mk,nk->mn", A[P:], W)])
    return y


# ---- tiles and mutations -------------------------------------------------------------------------------------------------------------------------------------
def row_tiles(c: Case):
    """Index tensors of 128-row tiles of the uncompacted output -- finer than any kernel's, so "every tile" below covers every kernel tile.  Sequence
    tiles: 128-token parts of a sequence, the class row in a tile of its own; pair: both halves; epilogue 4: without the dropped rows."""
    dev = c.A.device
    tiles = []
    if c.seq_rows:
        for half in range(2 if c.pair_rows else 1):
            for s in range(c.nseq):
                base = half * c.pair_rows + s * c.seq_rows
                tiles += [torch.arange(base + t, base + t + 128, device=dev) for t in range(0, c.seq_rows - 1, 128)]
                tiles.append(torch.tensor([base + c.seq_rows - 1], device=dev))
    else:
        tiles = [torch.arange(m, min(m + 128, c.M), device=dev) for m in range(0, c.M, 128)]
    if c.epi == 4:
        tiles = [t[t % c.period != c.period - 1] for t in tiles]
    return [t for t in tiles if len(t)]


def col_tiles(c: Case):
    return [slice(n, min(n + 128, c.N)) for n in range(0, c.N, 128)]


def _is_class(c: Case, t: torch.Tensor) -> bool:
    if not c.seq_rows or len(t) != 1:
        return False
    r = int(t[0])
    return (r - (c.pair_rows if r >= c.rows_c else 0)) % c.seq_rows == c.seq_rows - 1


def mutations(c: Case):
    """-> list of (name, wrong uncompacted output, [(row index tensor, column slice), ...] = the tiles the mutation touches).  Only the mutations that
    exist for the case's form are listed (no lo sweep without split activations, no class row without sequences, ...)."""
    nk = c.K // 64
    rt, ct = row_tiles(c), col_tiles(c)
    everything = [(r, s) for r in rt for s in ct]
    cls_tiles = [r for r in rt if _is_class(c, r)]
    tok_tiles = [r for r in rt if not _is_class(c, r)]
    out = []

    def add(name, touched, **hooks):
        out.append((name, finish(c, pre_activation(c, **hooks)), touched))

    sweeps = [(0, t) for t in range(nk)] + ([(1, t) for t in range(nk)] if c.A2 is not None else [])
    for tag, i in (("first", 0), ("middle", len(sweeps) // 2), ("last", len(sweeps) - 1)):
        src, t = sweeps[i]
        add(f"drop the {tag} K-tile", everything, ktile_delta=[(-1, src, t, t)])
    if c.A2 is not None:
        i, j = 0, nk - 1                                                        # hi K-tile i <-> lo K-tile j: each sweep multiplies the other's operand tile
        if i != j:                                                              # (one K-tile per sweep: the swap is the identity)
            add("swap two K-tiles between the hi and lo sweeps", everything, ktile_delta=[(-1, 0, i, i), (-1, 1, j, j), (1, 1, j, i), (1, 0, i, j)])
        add("read A instead of A2 in the second sweep", everything, lo_reads_hi=True)
    if c.seq_rows and c.nseq > 1:
        add("class row of sequence s + 1", [(r, s) for r in cls_tiles for s in ct], cls_shift=True)
    if c.pair_rows:
        add("omit the A_delta term on the u rows", [(r, s) for r in rt if int(r[0]) >= c.pair_rows for s in ct], no_delta=True)
    truth = finish(c, pre_activation(c))
    perm = torch.arange(c.M, device=c.A.device)
    touched = []
    for r in tok_tiles:
        full = (len(r) // 32) * 32                                              # rows m <-> m + 16 in whole 32-row groups of the tile
        if full:
            perm[r[:full]] = r[:full].reshape(-1, 2, 16).flip(1).reshape(-1)
            touched += [(r, s) for s in ct]
    if touched:
        out.append(("swap rows m and m + 16 inside a tile", truth[perm], touched))
    if c.N >= 8:
        cols = torch.arange(c.N, device=c.A.device)
        for s in ct:
            if s.stop - s.start >= 8:
                cols[s.start:s.start + 8] = torch.cat([cols[s.start + 4:s.start + 8], cols[s.start:s.start + 4]])
        out.append(("swap two 4-column groups", truth[:, cols], [(r, s) for r in rt for s in ct if s.stop - s.start >= 8]))
    cond_tok = [r for r in tok_tiles if int(r[0]) < c.rows_c]
    for i in range(len(c.lo)):
        # (the conditional rows carry the correction; pair: the u rows inherit it through the shared accumulator)
        add(f"mini-tile set {i}: scales of the 64-token group g + 1", [(r, s) for r in (tok_tiles if c.pair_rows else cond_tok) for s in ct], scale_shift=i)
    if c.lo and not c.pair_rows:
        add("skip the mini-tile set on the second 128-row half", [(r, s) for r in cond_tok if (int(r[0]) % c.seq_rows) % 256 >= 128 for s in ct], skip_half=True)
    if c.N >= 512:
        add("bias of the previous tile (column block n0 - 256)", [(r, s) for r in rt for s in ct if s.start >= 256], bias_shift=True)
    return out


# ---- the persistent walk's index arithmetic (mb_common.h xcd_remap + gemm_ht.hip make_plan) ---------------------------------------------------------------
def xcd_remap(b: int, nblk: int) -> int:
    q, r, x, i = nblk >> 3, nblk & 7, b & 7, b >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i


def tile_of(vb: int, tiles_m: int, tiles_n: int, rows_sr_is_8: bool = False):
    """Virtual block -> (tm, tn): XCD-contiguous chunks, inside them super-rows of 8 x tiles_n with a short last one.  rows_sr_is_8: the mutation."""
    L = xcd_remap(vb, tiles_m * tiles_n)
    sr = L // (8 * tiles_n)
    rows_sr = 8 if rows_sr_is_8 else min(8, tiles_m - sr * 8)
    rem = L - sr * 8 * tiles_n
    tn = rem // rows_sr
    return sr * 8 + (rem - tn * rows_sr), tn


def gpu_geometries():
    """Every (tiles_m, tiles_n) the GPU file launches on the half-tile kernel."""
    geo = set()
    for M, N, _ in HT_SHAPES:
        for bm in (192, 256):
            geo.add(((M + bm - 1) // bm, N // 256))
        if M % 257 == 0:
            geo.add((M // 257, N // 256))
    for pair, n, sq, N, _, nlo in SEQ_SHAPES:
        tm = n * (sq - 1) // (128 if pair else 256)
        for ns in ((1, 2, 4) if (nlo and not pair) else (1,)):
            geo.add((tm, N // 256 * ns))
    for n, N, _ in MINI_SPLIT_SHAPES:
        geo.add((n, N // 256))
    return sorted(geo)


def walk_length(tiles: int, cus: int) -> int:
    grid = min(tiles, cus if cus else 256)
    return (tiles + grid - 1) // grid
