"""References of the attention kernels (attention.hip), shared by tests/test_attention_cpu.py and tests/test_hip_attention_exact.py.

Three things live here.

FLOAT64 REFERENCES on the fp16 q / k / v given: `plain` (softmax(QK^T / sqrt(dh)) V), `pair` (conditional rows o_c, twin rows o_u - o_c; the caller
applies the single fp16 rounding) and `probs` (head-averaged probabilities).  All go through `attend`, whose `fault` argument turns it into one of
the WRONG kernels of `FAULTS`: the CPU file proves that the cases below tell each of them from the right one.

EXACT CASES ("grouped keys", `grouped_case`).  The keys of a (sequence, head) are partitioned into groups of power-of-two size, scattered over the
positions by a seeded permutation; every key of group g holds A * H[g], H a row of the Sylvester Hadamard matrix of order dh, and a query aimed at
group g holds the same vector.  Scores are A^2 dh = 4096 (dh 64) or 2048 (dh 32) inside the group and exactly 0 outside, so every excluded
probability is exp2(< -150) = 0 in fp32 (and exp(< -150) in the probabilities kernel), every included one is exp2(0) = 1, the sum is 2^k and its
reciprocal 2^-k.  V holds integer multiples of 2^-6 below 64, so the fp32 sums are exact and the output is fp16(sum / 2^k) with ONE rounding, which
float64 reproduces: the kernel's output must EQUAL the reference.  An all-zero query is uniform over all N keys; V's columns are t_c + e[j, c] with
sum_j e[j, c] = 0 and t_c on the fp16 grid, so the expected output is t_c whatever the rounding of 1 / N -- and one extra counted copy of a key moves
it.  `permutation_case` (N <= dh: every key its own group, arbitrary finite fp16 V, output row = one V row) and `scale_case` (one key ahead of the
rest by a gap at which the right scale still gives an fp16 probability of 0 and a scale too small by 1 / log2(e) or sqrt(heads) does not) complete them.

BAND CASES (`band_case`) are general softmax inputs; `band_plain` / `band_pair` / `band_probs` bound the kernels' error PER ELEMENT, term by term from
the operations (derivation in profiles/attention_exact.md), from the float64 quantities alone -- nothing is measured from a kernel.
A plain module: no fixtures, nothing here touches the GPU."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

A_GROUPED = 8.0
LOG2E = 1.4426950408889634
U32, U16 = 2.0 ** -24, 2.0 ** -11           # unit roundoffs of fp32 and fp16
SAFETY = 2.0                                 # factor over the derived sum (profiles/attention_exact.md)
ATTL_KB = 128                                # keys per block of the streaming kernels

# ---- the shapes of the GPU file (the CPU file walks the same ones) --------------------------------------------------------------------------------
ONE_BLOCK_N = (1, 2, 15, 16, 17, 65, 240, 241, 255, 256, 257, 272, 273, 288)
STREAM_N = (289, 300, 384, 385, 1025)
F4_N = (257, 321, 1025)
PROBS_N = (2, 17, 65, 257, 300, 1025)
NSEQ, PAIRS = 3, 2


def widths(N):
    """(d, heads) the GPU file runs at length N: both head widths; N = 1025 only at the smallest d."""
    return ((64, 1), (32, 1)) if N == 1025 else ((128, 2), (128, 4))


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def hadamard(n: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


# ---- float64 references and their wrong variants -------------------------------------------------------------------------------------------------------
FAULTS = ("pad_copies_288", "pad_copies_block", "drop_last_key", "head_next_v", "head_next_k", "swap_kv", "scale_d", "scale_ln", "no_rescale",
          "twin_from_rounded", "twin_offset_1", "swap_p_keys", "seq_next_kv", "avg_before_norm")
SINGLE_ROUNDING_FAULTS = ("twin_from_rounded",)          # differ from the right kernel by one fp16 rounding: exact cases only


def split(qkv, nseq, N, d, heads):
    """[nseq N, 3d] -> q, k, v float64 [nseq, heads, N, dh]"""
    x = qkv.double().reshape(nseq, N, 3, heads, d // heads).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def attend(qkv, nseq, N, d, heads, fault: Optional[str] = None, want_probs=False):
    """float64 attention [nseq N, d] (want_probs: the probabilities [nseq, heads, N, N]) of packed fp16 rows; `fault` = one of FAULTS."""
    dh = d // heads
    q, k, v = split(qkv, nseq, N, d, heads)
    if fault == "head_next_v": v = v.roll(-1, 1)
    if fault == "head_next_k": k = k.roll(-1, 1)
    if fault == "swap_kv": k, v = v, k
    if fault == "seq_next_kv": k, v = k.roll(-1, 0), v.roll(-1, 0)
    s = q @ k.transpose(-1, -2) / math.sqrt(d if fault == "scale_d" else dh)
    if fault == "scale_ln": s = s / LOG2E                    # exp2 of the natural-log argument
    if fault == "drop_last_key" and N > 1: s[..., N - 1] = -math.inf
    w = torch.exp(s - s.amax(-1, keepdim=True))
    if fault in ("pad_copies_288", "pad_copies_block"):      # keys N .. padded end are copies of key N - 1 and are not masked
        end = 288 if fault == "pad_copies_288" else -(-N // ATTL_KB) * ATTL_KB
        w[..., N - 1] *= 1 + max(0, end - N)
    if fault == "avg_before_norm":
        w = w.mean(1, keepdim=True).expand_as(w)
    p = w / w.sum(-1, keepdim=True)
    if want_probs:
        return p
    if fault == "no_rescale":                                 # streaming form whose output accumulator is not rescaled when the maximum rises
        o, m_run = torch.zeros_like(q), torch.full(s.shape[:-1] + (1,), -math.inf, dtype=torch.float64)
        for b in range(0, N, ATTL_KB):
            m_run = torch.maximum(m_run, s[..., b:b + ATTL_KB].amax(-1, keepdim=True))
            o = o + torch.exp(s[..., b:b + ATTL_KB] - m_run) @ v[..., b:b + ATTL_KB, :]
        o = o / torch.exp(s - m_run).sum(-1, keepdim=True)
    else:
        pv = p
        if fault == "swap_p_keys" and N > 1:                  # two keys of a 32-key k-block exchanged on the P side only
            j2 = min(17, N - 1)
            pv = p.clone(); pv[..., 0], pv[..., j2] = p[..., j2], p[..., 0]
        o = pv @ v
    return o.permute(0, 2, 1, 3).reshape(nseq * N, d)


def plain(qkv, nseq, N, d, heads, fault=None):
    return attend(qkv, nseq, N, d, heads, fault)


def pair(qkv, pairs, N, d, heads, fault=None):
    """-> float64 [2 pairs N, d]: conditional rows o_c, then twin rows o_u - o_c"""
    o = attend(qkv, 2 * pairs, N, d, heads, fault).reshape(2 * pairs, N, d)
    oc, ou = o[:pairs], o[pairs:]
    if fault == "twin_offset_1": ou = o.roll(-1, 0)[:pairs]
    base = oc.half().double() if fault == "twin_from_rounded" else oc
    return torch.cat([oc, ou - base]).reshape(2 * pairs * N, d)


def probs(qkv, nseq, N, d, heads, fault=None):
    """-> float64 [nseq, N, N]: the head-averaged probabilities"""
    return attend(qkv, nseq, N, d, heads, fault, want_probs=True).mean(1)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------------------
def group_sizes(N: int, dh: int):
    """Power-of-two group sizes summing to N: 1, 2, 4 .. 128 as far as N reaches, then 128s, then the binary digits of the rest."""
    sizes, rem = [], N
    for k in range(8):
        if rem >= 1 << k:
            sizes.append(1 << k); rem -= 1 << k
    while rem >= 128:
        sizes.append(128); rem -= 128
    for k in range(6, -1, -1):
        if rem >= 1 << k:
            sizes.append(1 << k); rem -= 1 << k
    assert rem == 0 and sum(sizes) == N and len(sizes) <= dh, (N, dh, sizes)
    return sizes


@dataclass
class Case:
    qkv: torch.Tensor                 # fp16 [nseq N, 3d]
    nseq: int
    N: int
    d: int
    heads: int
    group: Optional[torch.Tensor] = None       # [nseq, heads, N] group of every key (exact cases)
    target: Optional[torch.Tensor] = None      # [nseq, heads, N] group every query aims at, -1 = the all-zero query
    label: str = ""

    @property
    def dh(self):
        return self.d // self.heads


def _v_quanta(N, dh, g):
    """V of one (sequence, head) in quanta of 2^-6 [N, dh]: column c = t_c + e[:, c], sum_j e[j, c] = 0, |t| < 8, key N - 1 large (16 .. 24), |v| < 64."""
    t = torch.randint(-8 * 64 + 1, 8 * 64, (dh,), generator=g)
    e = torch.randint(-4 * 64, 4 * 64 + 1, (N, dh), generator=g)
    if N > 1:
        e[N - 1] = torch.randint(16 * 64, 24 * 64 + 1, (dh,), generator=g) * (1 - 2 * torch.randint(0, 2, (dh,), generator=g))
        r = -e.sum(0)                                           # spread over keys 0 .. N - 2
        e[: N - 1] += torch.div(r, N - 1, rounding_mode="floor")
        rest = r - torch.div(r, N - 1, rounding_mode="floor") * (N - 1)            # 0 .. N - 2
        e[: N - 1] += (torch.arange(N - 1)[:, None] < rest[None, :]).long()
    else:
        e.zero_()
    assert bool((e.sum(0) == 0).all()) and int((t + e).abs().max()) < 64 * 64
    return t + e, t


def many_small_groups(N: int, dh: int, size: int):
    """Group sizes with as many groups of `size` (1 or 2) as dh allows: for the cases whose queries all aim at groups of one size."""
    n = min((dh - 16), (N - 1) // size)
    sizes, rem = [size] * n, N - size * n
    sizes += [1 << k for k in range(10, -1, -1) if rem >> k & 1]
    assert sum(sizes) == N and len(sizes) <= dh
    return sizes


def grouped_case(nseq, N, d, heads, seed=0, zero_every=5, sizes=None) -> Case:
    """The grouped-keys case: query i of (sequence s, head h) aims at group (m i + s + h) mod G, m coprime to G, every zero_every-th query is all zero."""
    dh = d // heads
    H = hadamard(dh)
    sizes = sizes or group_sizes(N, dh)
    G = len(sizes)
    qkv = torch.zeros(nseq, N, 3, heads, dh, dtype=torch.float64)
    group = torch.zeros(nseq, heads, N, dtype=torch.int64)
    target = torch.zeros(nseq, heads, N, dtype=torch.int64)
    for s in range(nseq):
        for h in range(heads):
            g = _gen(seed * 7919 + N * 64 + s * 8 + h)
            last = (s + h) % 2 if G >= 2 else 0                 # key N - 1: a group of its own, or the size-2 group
            ids = torch.cat([torch.full((n - (gi == last),), gi) for gi, n in enumerate(sizes)])
            grp = torch.empty(N, dtype=torch.int64)
            grp[torch.randperm(N - 1, generator=g)] = ids
            grp[N - 1] = last
            tgt = (next(m for m in (3, 5, 7, 11, 13) if math.gcd(m, G) == 1) * torch.arange(N) + s + h) % G      # every group, if N reaches
            if zero_every:
                tgt[torch.arange(N) % zero_every == 1 % min(N, zero_every)] = -1      # the same rows in every sequence: a twin's zero query meets a zero query
            group[s, h], target[s, h] = grp, tgt
            qkv[s, :, 1, h] = A_GROUPED * H[grp]
            qkv[s, :, 0, h] = torch.where(tgt[:, None] >= 0, A_GROUPED * H[tgt.clamp(min=0)], torch.zeros(1, dtype=torch.float64))
            qkv[s, :, 2, h] = _v_quanta(N, dh, g)[0].double() / 64
    c = Case(qkv.reshape(nseq * N, 3 * d).half(), nseq, N, d, heads, group, target, f"grouped N {N} d {d} heads {heads}")
    check_grouped(c)
    return c


def check_grouped(c: Case):
    """The builder's own assertions: in-group scores bitwise equal, excluded arguments below -150 (base 2 for the MFMA kernels, base e for the
    probabilities kernel), V on the 2^-6 grid below 64, and at the all-zero queries a column mean on the fp16 grid."""
    assert torch.equal(c.qkv.double().half(), c.qkv)
    q, k, v = split(c.qkv, c.nseq, c.N, c.d, c.heads)
    s = (q.float() @ k.float().transpose(-1, -2))               # exact integers in fp32
    assert torch.equal(s.double(), q @ k.transpose(-1, -2))
    inside = c.group[:, :, None, :] == c.target[:, :, :, None]
    zero = (c.target < 0)[..., None].expand_as(inside)
    top = A_GROUPED ** 2 * c.dh
    assert bool((s[inside] == top).all()) and bool((s[~inside] == 0).all())
    assert bool(inside.any(-1)[c.target >= 0].all()), "a query aims at an empty group"
    scale = 1.0 / math.sqrt(c.dh)
    assert -top * scale * LOG2E < -150 and -top * scale < -150
    assert bool(((v * 64) == (v * 64).round()).all()) and float(v.abs().max()) < 64
    mean = v.sum(2) / c.N
    assert torch.equal(mean.half().double(), mean) or not bool(zero.any())
    return inside | zero


def expected_grouped(c: Case, pairs: int = 0):
    """The exact outputs, computed from the groups alone (not through a softmax): fp16 [nseq N, d]; pairs: the pair form."""
    return exact_grouped(c, pairs).half()


def exact_grouped(c: Case, pairs: int = 0):
    """... before the one fp16 rounding: float64, every value representable in fp32"""
    _, _, v = split(c.qkv, c.nseq, c.N, c.d, c.heads)
    member = check_grouped(c).double()                          # [nseq, heads, query, key]
    o = (member @ v) / member.sum(-1, keepdim=True)             # sums of 2^-6 multiples over 2^k or N keys: exact in float64
    zero = c.target < 0
    o[zero] = (v.sum(2) / c.N)[:, :, None, :].expand_as(o)[zero]       # == t_c
    o = o.permute(0, 2, 1, 3).reshape(c.nseq, c.N, c.d)
    if pairs:
        o = torch.cat([o[:pairs], o[pairs:] - o[:pairs]])
    return o.reshape(c.nseq * c.N, c.d)


def expected_probs_grouped(c: Case):
    """out[s, i, j] = sum_h [j in S_h(i)] / (heads |S_h(i)|), exactly (heads a power of two)"""
    member = check_grouped(c).double()
    return (member / member.sum(-1, keepdim=True)).mean(1)


def first_blocks(c: Case):
    """For the streaming kernels: the 128-key block in which each aimed query first meets its group -> set of (block, of nblk)"""
    nblk = -(-c.N // ATTL_KB)
    out = set()
    for s in range(c.nseq):
        for h in range(c.heads):
            for gi in set(c.target[s, h].tolist()) - {-1}:
                pos = (c.group[s, h] == gi).nonzero().flatten()
                out.add((int(pos.min()) // ATTL_KB, len(set((pos // ATTL_KB).tolist())) > 1))
    return out, nblk


def permutation_case(nseq, N, d, heads, seed=0) -> Case:
    """N <= dh: every key a group of its own, query i aims at key pi(i); V = arbitrary finite fp16 (up to 60000): output row i = V row pi(i)."""
    dh = d // heads
    assert N <= dh
    H = hadamard(dh)
    g = _gen(seed + 31 * N + d)
    qkv = torch.zeros(nseq, N, 3, heads, dh, dtype=torch.float64)
    group = torch.arange(N).expand(nseq, heads, N).clone()
    target = torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(heads)]) for _ in range(nseq)])
    qkv[:, :, 1] = A_GROUPED * H[group].permute(0, 2, 1, 3)
    qkv[:, :, 0] = A_GROUPED * H[target].permute(0, 2, 1, 3)
    mag = 2.0 ** torch.randint(-8, 15, (nseq, N, heads, dh), generator=g).double()          # normal fp16 values, |v| < 2^14: the twin difference is finite
    sign = 1 - 2 * torch.randint(0, 2, (nseq, N, heads, dh), generator=g).double()
    qkv[:, :, 2] = (0.5 + 0.4 * torch.rand(nseq, N, heads, dh, generator=g).double()) * sign * mag
    c = Case(qkv.reshape(nseq * N, 3 * d).half(), nseq, N, d, heads, group, target, f"permutation N {N} d {d} heads {heads}")
    s = split(c.qkv, nseq, N, d, heads)
    assert bool(torch.isfinite(s[2]).all())
    return c


def expected_permutation(c: Case, pairs: int = 0):
    _, _, v = split(c.qkv, c.nseq, c.N, c.d, c.heads)
    o = torch.gather(v, 2, c.target[..., None].expand_as(v)).permute(0, 2, 1, 3).reshape(c.nseq, c.N, c.d)
    if pairs:                                                   # arbitrary fp16 values: the fp32 subtraction rounds, then the store rounds again
        o = torch.cat([o[:pairs], (o[pairs:].float() - o[:pairs].float()).double()])
    return o.reshape(c.nseq * c.N, c.d).half()


SCALE_ARG = 45.0                                                # |exp2 argument| of the runner-up key under the right scale


def scale_case(nseq, N, d, heads, seed=0) -> Case:
    """Every query = H[0]; key j0 = b H[0] with the score b dh ahead of all other keys (zero vectors) by the integer gap nearest to SCALE_ARG / (log2(e) /
    sqrt(dh)).  Right scale: the others' probabilities are 2^-45 -> 0 as fp16 and lost in the fp32 sum: the output is V[j0] exactly, 0 in the even
    columns.  One other key j1 holds 60000 in the even columns: 60000 * 2^-45 rounds to 0 in fp16, but a scale too small by 1 / log2(e) (2^-31) or by
    sqrt(heads >= 2) (2^-32) leaves more than 1e-5 there.  The top score is no power of two, so max * c rounds and the top probability is 1 +- 2^-20 in
    fp32: the outputs are V[j0] (1 + delta).  V[j0] is therefore kept to |v| < 8 on the 2^-6 grid, even multiples in the first half of the sequences and
    odd ones in the second: a twin difference is a non-zero multiple of 2^-6 below 16, on the fp16 grid and far from a tie, and delta cannot move it."""
    dh = d // heads
    assert N >= 2
    gap = round(SCALE_ARG * math.sqrt(dh) / LOG2E)
    b = gap / dh
    assert b * 1024 == round(b * 1024) and gap * LOG2E / math.sqrt(dh) > 44 and 60000 * 2.0 ** -44 < 2.0 ** -26
    H = hadamard(dh)
    g = _gen(seed + N)
    qkv = torch.zeros(nseq, N, 3, heads, dh, dtype=torch.float64)
    group = torch.ones(nseq, heads, N, dtype=torch.int64)
    for s in range(nseq):
        for h in range(heads):
            j0, j1 = (torch.randperm(N, generator=g)[:2]).tolist()
            qkv[s, :, 0, h] = H[0]
            qkv[s, j0, 1, h] = b * H[0]
            qkv[s, j0, 2, h, 1::2] = (2 * torch.randint(-255, 255, (dh // 2,), generator=g) + (s >= (nseq + 1) // 2)).double() / 64
            qkv[s, j1, 2, h, 0::2] = 60000.0
            group[s, h, j0] = 0
    return Case(qkv.reshape(nseq * N, 3 * d).half(), nseq, N, d, heads, group, torch.zeros(nseq, heads, N, dtype=torch.int64), f"scale N {N} d {d} heads {heads}")


def expected_scale(c: Case, pairs: int = 0):
    _, _, v = split(c.qkv, c.nseq, c.N, c.d, c.heads)
    j0 = (c.group == 0).double().argmax(-1)                                     # [nseq, heads]
    row = torch.gather(v, 2, j0[..., None, None].expand(-1, -1, 1, c.dh))       # [nseq, heads, 1, dh]
    o = row.expand(-1, -1, c.N, -1).permute(0, 2, 1, 3).reshape(c.nseq, c.N, c.d)
    if pairs:
        o = torch.cat([o[:pairs], o[pairs:] - o[:pairs]])
    return o.reshape(c.nseq * c.N, c.d).half()


# ---- e2m1 copies: V from the e2m1 grid -----------------------------------------------------------------------------------------------------------------------
_F4_POS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def f4_value_case(nseq, N, d, heads, seed=0) -> Case:
    """Every key its own V row of e2m1 grid values times 2^e, e per (key, head) in -3 .. 3, each (key, head) block holding a +-6 (its amax) -- and every
    query aimed at a SIZE-1 group (grouped keys otherwise): the fp32 output tile is one such V row, decode(out4) * 2^(scale - 127) equals it exactly."""
    c = grouped_case(nseq, N, d, heads, seed=seed, zero_every=0, sizes=many_small_groups(N, d // heads, 1))
    dh = c.dh
    g = _gen(seed + 5 * N)
    ones = [[(torch.bincount(c.group[s, h]) == 1).nonzero().flatten() for h in range(heads)] for s in range(nseq)]
    x = c.qkv.double().reshape(nseq, N, 3, heads, dh)
    H = hadamard(dh)
    for s in range(nseq):
        for h in range(heads):
            tgt = ones[s][h][(torch.arange(N) + s + h) % len(ones[s][h])]
            c.target[s, h] = tgt
            x[s, :, 0, h] = A_GROUPED * H[tgt]
    val = _F4_POS[torch.randint(0, 8, (nseq, N, heads, dh), generator=g)] * (1 - 2 * torch.randint(0, 2, (nseq, N, heads, dh), generator=g))
    val[..., 0] = 6.0
    x[:, :, 2] = val * 2.0 ** torch.randint(-3, 4, (nseq, N, heads, 1), generator=g).double()
    c.qkv = x.reshape(nseq * N, 3 * d).half()
    c.label = f"e2m1 values N {N} d {d} heads {heads}"
    check_grouped(c)
    return c


def f4_lo_case(nseq, N, d, heads, seed=0) -> Case:
    """Queries aimed at SIZE-2 groups whose two V rows are (x, x + 2^-11 u 2^e) with x = m 2^e, m an odd 11-bit integer .. so the average needs 12 bits:
    o - fp16(o) is 0 or +- one power of two (2^(e-1)... per block all of one binade), which e2m1 holds exactly."""
    c = grouped_case(nseq, N, d, heads, seed=seed, zero_every=0, sizes=many_small_groups(N, d // heads, 2))
    dh = c.dh
    g = _gen(seed + 3 * N)
    x = c.qkv.double().reshape(nseq, N, 3, heads, dh)
    H = hadamard(dh)
    for s in range(nseq):
        for h in range(heads):
            cnt = torch.bincount(c.group[s, h])
            twos = (cnt == 2).nonzero().flatten()
            assert len(twos) >= 1
            tgt = twos[(torch.arange(N) + s) % len(twos)]
            c.target[s, h] = tgt
            x[s, :, 0, h] = A_GROUPED * H[tgt]
            for gi in twos.tolist():
                a, b = (c.group[s, h] == gi).nonzero().flatten().tolist()
                m = torch.randint(1024, 2048, (dh,), generator=g).double() * (1 - 2 * torch.randint(0, 2, (dh,), generator=g).double())
                bit = torch.randint(0, 2, (dh,), generator=g).double()
                bit[0] = 1.0
                x[s, a, 2, h] = m * 2.0 ** -6                   # in [16, 32): fp16 spacing 2^-6
                x[s, b, 2, h] = (m + bit * torch.sign(m)) * 2.0 ** -6      # average = (m + bit / 2) 2^-6: 12 bits when bit = 1
    c.qkv = x.reshape(nseq * N, 3 * d).half()
    assert torch.equal(c.qkv.double().reshape(nseq, N, 3, heads, dh), x)
    c.label = f"e2m1 lo halves N {N} d {d} heads {heads}"
    check_grouped(c)
    return c


# ---- band cases ---------------------------------------------------------------------------------------------------------------------------------------------
BAND_KINDS = ("rising", "falling", "spike", "gauss0.7", "gauss3")
BAND_CASES = tuple((kind, seed) for seed in (0, 1) for kind in BAND_KINDS)        # ten per kernel form


def band_case(kind, seed, nseq, N, d, heads) -> Case:
    """rising / falling: scores grow by 3 (in the exponent) per 128 keys along / against the key index, so every block of the streaming kernel raises
    the running maximum and the earlier blocks still count; spike: one key per (sequence, head) 60 ahead of the rest; gauss: q, k ~ N(0, sigma^2)."""
    dh = d // heads
    g = _gen(1000 * seed + N + d + heads + len(kind))
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    H0 = hadamard(dh)[min(3, dh - 1)]
    if kind.startswith("gauss"):
        sigma = float(kind[5:])
        q, k = rn(nseq, N, heads, dh) * sigma, rn(nseq, N, heads, dh) * sigma
    else:
        q = H0 * (1 + 0.1 * rn(nseq, N, heads, 1)) + 0.3 * rn(nseq, N, heads, dh)
        k = 0.3 * rn(nseq, N, heads, dh)
        if kind == "spike":
            for s in range(nseq):
                for h in range(heads):
                    k[s, int(torch.randint(0, N, (1,), generator=g)), h] += H0 * 60 / math.sqrt(dh)
        else:
            j = torch.arange(N, dtype=torch.float64)
            ramp = 3 * (j if kind == "rising" else N - 1 - j) / 128 / math.sqrt(dh)
            k = k + H0 * ramp[None, :, None, None]
    v = rn(nseq, N, heads, dh) * (1 + (torch.arange(N) % 7 == 0)[None, :, None, None] * 4.0)
    qkv = torch.stack([q, k, v], 2).reshape(nseq * N, 3 * d).half()
    return Case(qkv, nseq, N, d, heads, label=f"band {kind} seed {seed} N {N} d {d} heads {heads}")


def _band_parts(c: Case):
    """Per element [nseq, heads, N, dh] float64: (o, bound without the final fp16 rounding)."""
    dh, N = c.dh, c.N
    q, k, v = split(c.qkv, c.nseq, N, c.d, heads=c.heads)
    cs = LOG2E / math.sqrt(dh)
    s = q @ k.transpose(-1, -2)
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    mx = s.amax(-1, keepdim=True)
    p = torch.exp2((s - mx) * cs)
    L = p.sum(-1, keepdim=True)
    ph = p / L
    nblk = -(-N // ATTL_KB) if (N > 288 or N < 256) else 1      # rescales of the streaming kernels
    # relative error of a probability: exp2 argument (score accumulation over dh fp32 adds; rounding of c, of max * c and of the fma; once more per
    # rescale of the streaming form), v_exp_f32 (1 ulp = 2^-23 .. 2^-22 relative, per exponential)
    e = math.log(2) * (cs * dh * U32 * sabs + 2 * U32 * cs * (mx.abs() + (s - mx).abs()) * (1 + nblk)) + (1 + nblk) * 2.0 ** -22
    # fp16 rounding of a probability: 2^-11 relative, 2^-25 absolute below the normal range; the denominator sums the UNROUNDED fp32 values
    dp16 = torch.maximum(U16 * ph, torch.full_like(ph, 2.0 ** -25) / L)
    o = ph @ v
    bound = (e * ph + dp16) @ v.abs()                            # numerator
    bound = bound + o.abs() * ((e * ph).sum(-1, keepdim=True) + (N + nblk) * U32)        # denominator: propagated + fp32 summation
    bound = bound + (N + nblk + 2) * U32 * (ph @ v.abs())       # fp32 accumulation of the numerator, rescales, the final product with 1 / l
    return o, bound


def _rows(x, c):
    return x.permute(0, 2, 1, 3).reshape(c.nseq * c.N, c.d)


def band_plain(c: Case):
    """-> (float64 reference [nseq N, d], per-element bound on |fp16 output - reference|)"""
    o, b = _band_parts(c)
    return _rows(o, c), SAFETY * _rows(b + U16 * o.abs() + 2.0 ** -25, c)


def band_pair(c: Case, pairs: int):
    """conditional rows as band_plain; twin rows: both fp32 outputs' errors, one fp32 subtraction and ONE fp16 rounding of the difference"""
    o, b = _band_parts(c)
    o, b = _rows(o, c).reshape(c.nseq, c.N, c.d), _rows(b, c).reshape(c.nseq, c.N, c.d)
    diff = o[pairs:] - o[:pairs]
    ref = torch.cat([o[:pairs], diff])
    bound = torch.cat([b[:pairs] + U16 * o[:pairs].abs() + 2.0 ** -25,
                       b[:pairs] + b[pairs:] + U32 * (o[:pairs].abs() + o[pairs:].abs() + diff.abs()) + U16 * diff.abs() + 2.0 ** -25])
    return ref.reshape(-1, c.d), SAFETY * bound.reshape(-1, c.d)


def band_probs(c: Case):
    """attention_probs_kernel: fp32 FMA scores of q * scale (dh + 2 roundings), expf (<= 2 ulp), fp32 sum over N, one division, FMA mean over heads"""
    dh, N = c.dh, c.N
    q, k, _ = split(c.qkv, c.nseq, N, c.d, c.heads)
    sc = 1 / math.sqrt(dh)
    s = q @ k.transpose(-1, -2) * sc
    ds = (dh + 3) * U32 * (q.abs() @ k.abs().transpose(-1, -2)) * sc
    ds = ds + U32 * (s.abs() + s.amax(-1, keepdim=True).abs())                    # the subtraction of the maximum
    p = torch.softmax(s, -1)
    e = ds + ds.amax(-1, keepdim=True) + 2.0 ** -21 + (N + 4) * U32               # own argument + worst argument in the sum; expf; sum, 1 / sum, fma
    ref = p.mean(1)
    return ref, SAFETY * ((e * p).mean(1) + (c.heads + 1) * U32 * ref)


def emulate_fp16_p(c: Case, pairs: int = 0):
    """The right kernel in numpy-style arithmetic: fp32 scores, exp2 in fp32, fp16 probabilities, fp32 sums, fp32 twin subtraction -> fp16 rows"""
    q, k, v = (t.float() for t in split(c.qkv, c.nseq, c.N, c.d, c.heads))
    s = q @ k.transpose(-1, -2)
    cs = torch.tensor(LOG2E / math.sqrt(c.dh), dtype=torch.float32)
    p = torch.exp2(s * cs - s.amax(-1, keepdim=True) * cs)
    o = (p.half().float() @ v) * (1.0 / p.sum(-1, keepdim=True))
    o = o.permute(0, 2, 1, 3).reshape(c.nseq, c.N, c.d)
    if pairs:
        o = torch.cat([o[:pairs], o[pairs:] - o[:pairs]])
    return o.reshape(c.nseq * c.N, c.d).half()
