"""Float64 restatement of one sampling step, the rounding model of its float32 chain, and the two checkers built on them: the yardstick of
tests/test_sampling_step_cpu.py and tests/test_hip_sampling_step.py.  Plain torch / numpy, nothing imported from the code under test.

``step64``: modeling/modules/sampling.py:98-131 as oracle/maskbit_oracle.py:201-228 restates it, the float32 inputs promoted to float64.
``RoundingModel``: what the float32 evaluation of the same lines may differ by, term by term, each term from the definition of its operation.
``draw_check`` / ``thresh_check``: what an implementation's ``pred`` / ``tokens_out`` must satisfy given the two.
``step32``: the float32 chain in torch, in the summation order the HIP kernel documents, with switches for deliberately wrong variants.
``RANDOM_CASES`` / ``make_case``: the random inputs both test files use."""
import dataclasses
import functools
import math
from typing import Optional

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of float32 round-to-nearest: fl(a op b) = (a op b)(1 + e), |e| <= U, for + - * / (IEEE 754)
# expf / logf: the HIP math API reference of the ROCm documentation ("Single precision mathematical functions", column "Maximum ULP error")
# lists 1 for expf and 1 for logf (the accurate functions, not __expf / __logf).  One ulp of a result r is at most 2 U |r|.
ULP_EXPF = 1.0
ULP_LOGF = 1.0
SLACK = 1.0 + 2.0 ** -10  # every bound below is first order in U; the products of two error terms it leaves out are below U * 600 * U


def f32(x) -> float:
    """A Python float through float32, as a c_float argument or a float32 torch scalar holds it."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------------- reference
def step64(logits_c, logits_u, scale, temperature, exp_noise):
    """-> dict of float64 [rows, C]: ``logp`` = log p_c and ``score`` = log p_c - log q_c, and what the rounding model needs of the chain
    (``d`` = x - y, ``V`` the combined logits, ``W`` = V / T, ``t`` = W - max W).  The draw is argmax_c score (sampling.py:106-107 through
    torch.multinomial(n=1): argmax(p / q) with q ~ Exp(1))."""
    C = logits_c.shape[-1]
    x = logits_c.double().reshape(-1, C)
    s, T = f32(scale), f32(temperature)
    if logits_u is not None:
        d = x - logits_u.double().reshape(-1, C)
        d = torch.where(torch.isinf(x), x, d)                       # a forbidden class (x = -inf) stays -inf
        V = torch.where(torch.isinf(x), x, x + s * d)               # :98-99
    else:
        d, V = None, x
    W = V / T                                                       # :105
    t = W - W.max(dim=-1, keepdim=True).values
    logp = t - torch.logsumexp(t, dim=-1, keepdim=True)             # softmax, :105
    logp = logp - torch.logsumexp(logp, dim=-1, keepdim=True)       # Categorical.__init__: probs / probs.sum(-1), an identity up to float64 rounding
    score = logp - torch.log(exp_noise.double().reshape(-1, C))     # multinomial(n=1): argmax(p / q)
    return {"logp": logp, "score": score, "d": d, "V": V, "W": W, "t": t, "scale": s, "temperature": T, "guided": logits_u is not None}


def masked_counts(tokens, mask_token):
    return (tokens.reshape(tokens.shape[0], -1) == mask_token).sum(dim=1)


def mask_len32(mask_ratio, num_maskable) -> int:
    """torch.floor(mask_ratio * num_maskable) with a float32 ratio (:120-123): the product is a float32 product."""
    return int(math.floor(float(np.float32(mask_ratio) * np.float32(num_maskable))))


def k_reference(tokens, mask_token, mask_len):
    """:109 and :123-124: ONE k for the batch, clamp(mask_len, 1, num_masked - 1) with SAMPLE 0's masked count (the upper clamp wins, as in
    torch.clamp).  May be 0 or -1; the threshold is the Python index k - 1 (:126)."""
    nm0 = int(masked_counts(tokens, mask_token)[0])
    return min(max(int(mask_len), 1), nm0 - 1)


def k_edit(tokens, mask_token, mask_ratio, num_regen):
    """The edit step's rule (include/maskbit_hip.h): per sample b, nm_b >= 2: k = min(max(floor32(ratio * num_regen[b]), 1), nm_b - 1); nm_b <= 1:
    None (nothing is re-masked)."""
    out = []
    for b, nm in enumerate(masked_counts(tokens, mask_token).tolist()):
        out.append(min(max(mask_len32(mask_ratio, int(num_regen[b])), 1), nm - 1) if nm >= 2 else None)
    return out


def confidences64(ref, pred, tokens, conf_noise, mask_token):
    """float64 [B, P] confidences of a GIVEN pred: log p[pred] + noise at masked slots, +inf at known ones (:113-118)."""
    B = tokens.shape[0]
    C = ref["logp"].shape[1]
    idx = pred.reshape(-1, 1).clamp(0, C - 1)
    lp = ref["logp"].gather(1, idx).squeeze(1)
    conf = torch.where(tokens.reshape(-1) == mask_token, lp, torch.full_like(lp, math.inf)) + conf_noise.double().reshape(-1)
    return conf.reshape(B, -1)


# ------------------------------------------------------------------------------------------------------------------------------ rounding model
def sum_depth_kernel(C: int) -> int:
    """Additions a term passes through in the kernel's row sums as csrc/sampling.hip documents them: a chain over the lane's ceil(C / 64) register
    slots, then a 6-level butterfly over the 64 lanes.  A sum of non-negative terms formed by a tree of depth D has relative error <= D U."""
    cpl = next(c for c in (1, 2, 4, 8, 16, 32, 64) if C <= 64 * c)
    return cpl - 1 + 6


class RoundingModel:
    """Bounds on |float32 chain - float64 restatement|, in log units, from the operations of the chain in their order:

      d  = fl(x - y)            relative U           |
      m  = fl(s * d)            relative U           |  the three roundings of the combine: error of v0 against V <= 2 U |s d| + U |V|
      v0 = fl(x + m)            relative U           |  (no guidance: v0 = x, no error)
      v  = fl(v0 / T)           relative U: E_W = E_V / T + U |W|        (T = 1: the division is exact, E_W = E_V)
      t  = fl(v - mx)           relative U: + U |t|  (mx is the float32 maximum, one number per row: as a shift it cancels in everything below)
      e  = expf(t)              ULP_EXPF ulp = 2 U ULP_EXPF relative, and exp turns the absolute error of t into a relative one
                                => a_c = E_W(c) + U |t_c| + 2 U ULP_EXPF                                         (log error of e_c)
      S  = sum_c e_c            every term carries a_c: the p-weighted mean of a; the additions: depth * U
      p  = fl(e / S)            relative U
      ps = sum_c p_c, pn = fl(p / ps)   relative U (ps is one number per row and cancels between classes)
      r  = fl(pn / q)           relative U
    draw: argmax_c r_c.  log r_c - score_c = (terms common to the row) + err_c with |err_c| <= a_c + 3 U =: dcls_c, so the error of a score
    difference s_a - s_b is at most dcls_a + dcls_b = delta_draw.
      conf = fl(logf(p_pred) + noise): log error of p_pred = a_pred + mean_p(a) + depth U + U; logf: 2 U ULP_LOGF |log p|; the add: U |conf|.
    Classes with W = -inf have e = 0 exactly and carry no error."""

    def __init__(self, ref, sum_depth: int):
        t, W = ref["t"], ref["W"]
        dead = torch.isinf(W)
        if ref["guided"]:
            E_V = U * (2.0 * abs(ref["scale"]) * ref["d"].abs() + ref["V"].abs())        # the three roundings of the combine
        else:
            E_V = torch.zeros_like(W)
        T = ref["temperature"]
        E_W = E_V / T + (U * W.abs() if T != 1.0 else 0.0)                               # the division by the temperature
        a = E_W + U * t.abs() + 2.0 * U * ULP_EXPF                                       # v - max, expf
        a = torch.where(dead, torch.zeros_like(a), a) * SLACK
        self.a = a
        self.dcls = a + 3.0 * U * SLACK                                                  # / sum, / psum, / q
        self.sum_term = ((ref["logp"].exp() * a).sum(dim=1) + sum_depth * U * SLACK)     # error of log S
        self.ref = ref

    def delta_draw(self, rows, top, cls):
        """Bound of the error of score[row, top] - score[row, cls]."""
        return self.dcls[rows, top] + self.dcls[rows, cls]

    def delta_conf(self, pred, conf64):
        """[rows] bound of the error of a masked slot's confidence, 0 at a known slot (+inf exactly)."""
        C = self.a.shape[1]
        idx = pred.reshape(-1, 1).clamp(0, C - 1)
        lp = self.ref["logp"].gather(1, idx).squeeze(1)
        c = conf64.reshape(-1)
        d = (self.a.gather(1, idx).squeeze(1) + self.sum_term + U * SLACK                # e_pred, S, the division
             + 2.0 * U * ULP_LOGF * lp.abs() * SLACK + U * c.abs() * SLACK)              # logf, the final add
        return torch.where(torch.isinf(c), torch.zeros_like(d), d)


# ---------------------------------------------------------------------------------------------------------------------------------- checkers
LOGP_FLOOR = -80.0   # exp(-80) = 2^-115: above float32's subnormals, so the relative bounds above hold for every class the checkers look at


def draw_check(ref, model, tokens, pred, mask_token):
    """Every masked row: pred in {c : s_top - s_c <= delta_draw(top, c)}; every known row: pred == tokens.  -> (violations, stats)."""
    C = ref["score"].shape[1]
    tok, pr = tokens.reshape(-1), pred.reshape(-1)
    masked = tok == mask_token
    bad = []
    if bool(((pr < 0) | (pr >= C))[masked].any()):
        bad.append("pred outside [0, C) on a masked row")
    if not torch.equal(pr[~masked], tok[~masked]):
        bad.append(f"pred != tokens_in on {int((pr != tok)[~masked].sum())} known rows")
    score = ref["score"]
    s_top, top = score.max(dim=1)
    cand = (s_top.unsqueeze(1) - score) <= (model.dcls.gather(1, top.unsqueeze(1)) + model.dcls)
    # a class below the floor is never a candidate: its float32 ratio is at most e^-80 / q against a top ratio of at least 1 / (C q_top)
    cand &= ref["logp"] > LOGP_FLOOR
    ok = cand.gather(1, pr.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    miss = masked & ~ok
    if bool(miss.any()):
        r = int(miss.nonzero()[0])
        bad.append(f"{int(miss.sum())} masked rows drawn outside the candidate set; row {r}: pred {int(pr[r])} at "
                   f"{float(s_top[r] - score[r, pr[r].clamp(0, C - 1)]):.3e} below the top class {int(top[r])}")
    multi = (cand.sum(dim=1) > 1) & masked
    nmask = max(int(masked.sum()), 1)
    return bad, {"masked_rows": int(masked.sum()), "multi_share": float(multi.sum()) / nmask, "top": top}


def thresh_check(ref, model, tokens, conf_noise, pred, tokens_out, mask_token, k_per_sample):
    """With the implementation's OWN pred: k_per_sample[b] the count rule's k (None: sample b is not re-masked; <= 0: the Python index k - 1
    wraps).  thr64 = sorted(conf64[b])[k - 1]; band = 2 * max delta_conf of the sample.  conf64 < thr64 - band => re-masked; conf64 > thr64 +
    band => holds pred; thr64 = +inf => every slot re-masked; the re-masked count is the number of conf64 <= thr64 whenever the k-th and
    (k+1)-th smallest are more than the band apart.  -> (violations, stats)."""
    B = tokens.shape[0]
    conf = confidences64(ref, pred, tokens, conf_noise, mask_token)
    dconf = model.delta_conf(pred, conf).reshape(B, -1)
    out, pr = tokens_out.reshape(B, -1), pred.reshape(B, -1)
    P = conf.shape[1]
    bad, gaps, bands = [], [], []
    lp = ref["logp"].gather(1, pred.reshape(-1, 1).clamp(0, ref["logp"].shape[1] - 1)).squeeze(1)
    if bool((lp[tokens.reshape(-1) == mask_token] <= LOGP_FLOOR).any()):
        bad.append("a drawn class below the floor of the rounding model")
    for b in range(B):
        re = out[b] == mask_token
        keep = out[b] == pr[b]
        if not bool((re | keep).all()):
            bad.append(f"sample {b}: tokens_out is neither the mask token nor pred at {int((~(re | keep)).sum())} slots")
        k = k_per_sample[b]
        if k is None:
            if not torch.equal(out[b], pr[b]):
                bad.append(f"sample {b}: fewer than two masked slots, yet {int(re.sum())} slots re-masked")
            continue
        srt = torch.sort(conf[b]).values
        thr = float(srt[k - 1])                                                           # Python index: -1 / -2 wrap (:126)
        band = 2.0 * float(dconf[b].max())
        bands.append(band)
        if math.isinf(thr) and thr > 0:
            if not bool(re.all()):
                bad.append(f"sample {b}: threshold +inf, yet {int((~re).sum())} slots not re-masked")
            continue
        below, above = conf[b] < thr - band, conf[b] > thr + band
        if bool((below & ~re).any()):
            bad.append(f"sample {b}: {int((below & ~re).sum())} slots below the threshold not re-masked")
        if bool((above & re).any()):
            bad.append(f"sample {b}: {int((above & re).sum())} slots above the threshold re-masked")
        i = (k - 1) % P
        gap = float(srt[i + 1] - srt[i]) if i + 1 < P else math.inf
        gaps.append(gap)
        if gap > band:
            want = int((conf[b] <= thr).sum())
            if int(re.sum()) != want:
                bad.append(f"sample {b}: {int(re.sum())} slots re-masked, k = {k} asks for {want}")
    return bad, {"min_gap_over_band": min((g / bd for g, bd in zip(gaps, bands) if bd > 0), default=math.inf), "gaps": gaps, "bands": bands,
                 "conf": conf, "dconf": dconf}


# ------------------------------------------------------------------------------------------------------------------------- float32 chain, torch
def _row_sum_kernel_order(e):
    """float32 [rows, C] -> [rows]: the kernel's order (see sum_depth_kernel)."""
    rows, C = e.shape
    cpl = next(c for c in (1, 2, 4, 8, 16, 32, 64) if C <= 64 * c)
    pad = torch.zeros(rows, 64 * cpl, dtype=torch.float32)
    pad[:, :C] = e
    pad = pad.reshape(rows, cpl, 64)
    acc = torch.zeros(rows, 64, dtype=torch.float32)
    for i in range(cpl):
        acc = acc + pad[:, i]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


MUTANTS = ("fma", "no_renorm", "conf_pn", "lt", "own_count")


def step32(inp, mutant: Optional[str] = None):
    """The float32 chain of the step in torch, one rounding per line as the kernel makes them and its summation order; ``mutant`` one of MUTANTS:
    fma       -- the combine as x + fma(s, d): one rounding in the place of two,
    no_renorm -- argmax(p / q) without Categorical's renormalisation,
    conf_pn   -- the confidence from the renormalised pn instead of p,
    lt        -- conf < thr instead of <=,
    own_count -- each sample's own masked count in the place of sample 0's (plain step only).
    -> dict: pred, tokens_out [B, n, m] int64; ratio [rows, C] and conf [B, P] float32."""
    lc, lu, tokens = inp["logits_c"], inp["logits_u"], inp["tokens"]
    B = tokens.shape[0]
    C = lc.shape[-1]
    mask_token = C
    x = lc.reshape(-1, C)
    s, T = torch.tensor(inp["scale"], dtype=torch.float32), torch.tensor(inp["temperature"], dtype=torch.float32)
    if lu is not None:
        d = x - lu.reshape(-1, C)
        if mutant == "fma":
            v = (x.double() + s.double() * d.double()).float()          # the float64 product of two float32 numbers is exact: one rounding
        else:
            v = x + s * d
    else:
        v = x
    v = v / T
    tt = v - v.max(dim=1, keepdim=True).values
    e = torch.exp(tt)
    p = e / _row_sum_kernel_order(e).unsqueeze(1)
    pn = p / _row_sum_kernel_order(p).unsqueeze(1)
    ratio = (p if mutant == "no_renorm" else pn) / inp["exp_noise"].reshape(-1, C)
    pred = torch.argmax(ratio, dim=1)
    tok = tokens.reshape(-1)
    masked = tok == mask_token
    pred = torch.where(masked, pred, tok)
    pv = (pn if mutant == "conf_pn" else p).gather(1, pred.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    conf = torch.log(torch.where(masked, pv, torch.full_like(pv, math.inf))) + inp["conf_noise"].reshape(-1)
    conf = conf.reshape(B, -1)
    P = conf.shape[1]
    nm = masked.reshape(B, -1).sum(dim=1).tolist()
    out = pred.reshape(B, -1).clone()
    for b in range(B):
        if inp["edit"]:
            if nm[b] < 2:
                continue
            k = min(max(mask_len32(inp["mask_ratio"], int(inp["num_regen"][b])), 1), nm[b] - 1)
        else:
            k = min(max(int(inp["k_mask_len"]), 1), (nm[b] if mutant == "own_count" else nm[0]) - 1)
        thr = torch.sort(conf[b]).values[k - 1]
        re = conf[b] < thr if mutant == "lt" else conf[b] <= thr
        out[b] = torch.where(re, torch.full_like(out[b], mask_token), out[b])
    return {"pred": pred.reshape(tokens.shape), "tokens_out": out.reshape(tokens.shape), "ratio": ratio, "conf": conf}


# ------------------------------------------------------------------------------------------------------------------------------- random cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    C: int
    n: int
    m: int
    B: int
    sigma: float
    guided: bool
    scale: float
    temperature: float
    edit: bool
    seed: int
    mask_ratio: float = 0.3

    @property
    def P(self):
        return self.n * self.m


# A cross section of C in {8, 64, 100, 128, 200, 512, 1000, 2048, 4096} x P in {63, 512, 1025} x B in {1, 3}.  C = 200 is there because no C of the
# issue's list selects sample_rows_kernel<4> (128 < C <= 256).  The largest exp_noise: 1025 x 4096 floats = 16.8 MB.
RANDOM_CASES = (
    Case("c8_p63_b3_plain",       8,    21, 3, 3, 1.0, True,  3.0, 1.0, False, 101, 0.9),
    Case("c64_p512_b3_edit",      64,  256, 2, 3, 6.0, True,  7.1, 0.6, True,  102),
    Case("c100_p1025_b1_plain",   100, 1025, 1, 1, 1.0, False, 0.0, 1.0, False, 103),
    Case("c128_p63_b3_edit",      128,  21, 3, 3, 6.0, True,  0.0, 0.6, True,  104, 0.9),
    Case("c200_p512_b1_plain",    200, 256, 2, 1, 6.0, True,  3.0, 0.6, False, 105),
    Case("c512_p512_b1_plain",    512, 256, 2, 1, 1.0, True,  7.1, 1.0, False, 106),
    Case("c1000_p1025_b3_edit",   1000, 205, 5, 3, 6.0, True,  3.0, 0.6, True,  107),
    Case("c2048_p512_b3_plain",   2048, 256, 2, 3, 1.0, False, 0.0, 0.6, False, 108, 0.9),
    Case("c4096_p63_b3_edit",     4096, 21, 3, 3, 6.0, True,  7.1, 1.0, True,  109),
    Case("c4096_p1025_b1_plain",  4096, 1025, 1, 1, 1.0, False, 0.0, 0.6, False, 110),
)
# mask_ratio 0.3: mask_len = floor32(0.3 * P) lies below the masked count of every sample (about P / 2), every threshold is a masked slot's confidence.
# mask_ratio 0.9: mask_len lies above it, the clamp to the masked count - 1 decides: sample 0's in a plain step (a sample with fewer masked slots then
# has its threshold among the known slots, +inf, and is re-masked whole), the sample's own in an edit step.
FORBIDDEN = 3             # -inf logits per row


@functools.lru_cache(maxsize=2)
def make_case(case: Case):
    """-> dict of CPU tensors and scalars, the arguments of one step: sigma * randn logits (FORBIDDEN classes per row at -inf in logits_c, unless
    the case is guided at scale 0, where 0 * -inf has no value), Exp(1) draw noise, Gumbel * 4.5 confidence noise, a random half of the slots known."""
    g = torch.Generator().manual_seed(case.seed)
    B, n, m, C, P = case.B, case.n, case.m, case.C, case.P
    lc = case.sigma * torch.randn(B, n, m, C, generator=g)
    lu = case.sigma * torch.randn(B, n, m, C, generator=g) if case.guided else None
    if C > 2 * FORBIDDEN and not (case.guided and case.scale == 0.0):
        idx = torch.rand(B * P, C, generator=g).argsort(dim=1)[:, :FORBIDDEN] if C <= 512 else torch.randint(0, C, (B * P, FORBIDDEN), generator=g)
        lc.reshape(-1, C).scatter_(1, idx, -math.inf)
    q = torch.empty(B * P, C).exponential_(1, generator=g)
    u = torch.rand(B, n, m, generator=g).clamp_(1e-7, 1 - 1e-7)
    cn = -torch.log(-torch.log(u)) * 4.5
    known = torch.rand(B, n, m, generator=g) < 0.5
    tokens = torch.where(known, torch.randint(0, C, (B, n, m), generator=g), torch.full((B, n, m), C, dtype=torch.int64))
    nm = masked_counts(tokens, C)
    num_regen = torch.tensor([P if b % 2 == 0 else int(nm[b]) for b in range(B)], dtype=torch.int32)
    return {"case": case, "logits_c": lc, "logits_u": lu, "scale": f32(case.scale), "temperature": f32(case.temperature), "exp_noise": q,
            "conf_noise": cn, "tokens": tokens, "edit": case.edit, "mask_ratio": f32(case.mask_ratio), "num_regen": num_regen,
            "k_mask_len": mask_len32(case.mask_ratio, P)}


def reference_of(inp, sum_depth=None):
    """-> (ref, model) of a case's inputs; the kernel's summation depth unless another is given."""
    ref = step64(inp["logits_c"], inp["logits_u"], inp["scale"], inp["temperature"], inp["exp_noise"])
    return ref, RoundingModel(ref, sum_depth_kernel(inp["logits_c"].shape[-1]) if sum_depth is None else sum_depth)


def k_of(inp):
    """The count rule's k per sample for a case's inputs (see thresh_check)."""
    C = inp["logits_c"].shape[-1]
    if inp["edit"]:
        return k_edit(inp["tokens"], C, inp["mask_ratio"], inp["num_regen"])
    return [k_reference(inp["tokens"], C, inp["k_mask_len"])] * inp["tokens"].shape[0]


def check_step(inp, pred, tokens_out, sum_depth=None, refmodel=None):
    """Both checkers on one implementation's outputs -> (violations, draw stats, threshold stats)."""
    ref, model = refmodel if refmodel is not None else reference_of(inp, sum_depth)
    C = inp["logits_c"].shape[-1]
    bad_d, sd = draw_check(ref, model, inp["tokens"], pred, C)
    bad_t, st = thresh_check(ref, model, inp["tokens"], inp["conf_noise"], pred, tokens_out, C, k_of(inp))
    return bad_d + bad_t, sd, st


# ------------------------------------------------------------------------------------------------------------ exact inputs against a contraction
def fma_flip_pairs(count: int, scale: float = 7.1, seed: int = 7):
    """-> float32 [count] x, y, w: w = fl(x + fl(s * fl(x - y))), the combine in its three roundings, for which the contracted x + fma(s, x - y)
    rounds to a SMALLER number.  A row with (logits_c, logits_u) = (x, y) at class a and (w, w) at a class b > a, -inf elsewhere, q = 1, is an exact
    tie under the reference's arithmetic (pred = a, the lowest index) and no tie under the contraction (pred = b).  IEEE operations only: the
    expected value does not depend on any libm."""
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor(scale, dtype=torch.float32)
    x = 3.0 * torch.randn(64 * count, generator=g) + 8.0
    y = 3.0 * torch.randn(64 * count, generator=g)
    d = x - y
    w = x + s * d
    fused = (x.double() + s.double() * d.double()).float()
    pick = (fused < w).nonzero().squeeze(1)[:count]
    assert pick.numel() == count
    return x[pick], y[pick], w[pick]


# --------------------------------------------------------------------------------- exact inputs against a lost renormalisation / confidence from pn
def _exp32_neighbours(L: float):
    """float32 exp(L) as torch gives it and its neighbours two ulps to either side: every value an expf of 1 ulp can return, with room."""
    e = np.float32(torch.exp(torch.tensor(L, dtype=torch.float32)).item())
    out = [e]
    for towards in (np.float32(0), np.float32(2)):
        x = e
        for _ in range(2):
            x = np.nextafter(x, towards)
            out.append(x)
    return out


def renorm_flip_rows(count: int, seed: int = 11):
    """-> (logits float32 [count, 64], q float32 [count, 64], want, wrong): rows on which Categorical's renormalisation decides the draw, from IEEE
    operations alone.  Classes 1 and 33 at logit 0, class 3 at a logit L < 0, -inf elsewhere: e = (1, 1, expf(L)), S = fl(2 + e_3) (lanes 1 and 33
    meet in the first butterfly step and in one vector lane of a row sum, 1 + 1 is exact), p_1 = p_33 = fl(1 / S), sum p = fl(fl(p + p) + p_3).
    L is kept only if p and sum p come out the same for every expf(L) within two ulps and sum p != 1.  q_33 is the float32 below q_1, such that
    fl(fl(p / sum p) / q) is the same number for both (a tie: pred = 1 = ``want``) while fl(p / q_33) > fl(p / q_1) (no renormalisation: pred = 33 =
    ``wrong``).  q = 64 elsewhere."""
    f = np.float32
    rng = np.random.default_rng(seed)
    lc = torch.full((count, 64), -math.inf)
    q = torch.full((count, 64), 64.0)
    Ls = [x * 0.125 for x in range(-64, -8)]
    i = 0
    for L in Ls:
        if i == count:
            break
        res = set()
        for e3 in _exp32_neighbours(L):
            S = f(f(2) + e3)
            p, p3 = f(1) / S, e3 / S
            res.add((float(p), float(f(f(p + p) + p3))))
        if len(res) != 1:
            continue
        p, ps = (f(v) for v in res.pop())
        if ps == f(1):
            continue
        pn = p / ps
        qa = rng.uniform(0.5, 2.0, 4096).astype(f)
        qb = np.nextafter(qa, f(0))
        hit = np.nonzero(((pn / qa) == (pn / qb)) & ((p / qb) > (p / qa)))[0]
        if hit.size == 0:
            continue
        lc[i, 1] = lc[i, 33] = 0.0
        lc[i, 3] = L
        q[i, 1], q[i, 33] = float(qa[hit[0]]), float(qb[hit[0]])
        i += 1
    assert i == count
    return lc, q, [1] * count, [33] * count


def conf_pn_rows(count: int):
    """-> (logits float32 [count, 2, 1, 8], conf_noise float32 [count, 2, 1], want int64 [count, 2, 1], wrong): samples of two masked slots, C = 8, on
    which log p and log pn fall on different sides of the other slot's confidence.  Slot 0: class 1 at logit 0, class 5 at a logit L <= -8, -inf
    elsewhere: S = fl(1 + e_5), p_1 = fl(1 / S) just below 1, sum p = fl(p_1 + p_5) (two terms: no order), pn_1 = fl(p_1 / sum p); L is kept only
    if p_1 and sum p are the same for every expf(L) within two ulps and pn_1 != p_1.  log p_1 and log pn_1 are about -e_5 and differ by 2^-24
    or more, i.e. by several per cent of themselves, against a logf of 1 ulp.  Slot 1 is one-hot at class 3 (log p = 0 exactly) with the
    float64 midpoint of the two logs as its noise; slot 0 has noise 0.  With k = 1 the slot of the smaller confidence is re-masked: slot 0 iff
    log p_1 < midpoint (``want``), the other one if the confidence is taken from pn (``wrong``).  q = 1."""
    f = np.float32
    lc = torch.full((count, 2, 1, 8), -math.inf)
    cn = torch.zeros(count, 2, 1)
    want = torch.zeros(count, 2, 1, dtype=torch.int64)
    wrong = torch.zeros(count, 2, 1, dtype=torch.int64)
    i = 0
    for L in [x * 0.125 for x in range(-128, -63)]:
        if i == count:
            break
        res = set()
        for e5 in _exp32_neighbours(L):
            S = f(f(1) + e5)
            p, p5 = f(1) / S, e5 / S
            res.add((float(p), float(f(p + p5))))
        if len(res) != 1:
            continue
        p, ps = (f(v) for v in res.pop())
        pn = p / ps
        if pn == p or p >= f(1) or pn >= f(1):
            continue
        lp, lpn = math.log(float(p)), math.log(float(pn))
        mid = float(f(0.5 * (lp + lpn)))
        assert min(lp, lpn) * (1 - 1e-3) < mid < max(lp, lpn) * (1 + 1e-3) or max(lp, lpn) * (1 - 1e-3) > mid > min(lp, lpn) * (1 + 1e-3)
        lc[i, 0, 0, 1], lc[i, 0, 0, 5], lc[i, 1, 0, 3] = 0.0, L, 0.0
        cn[i, 1, 0] = mid
        a_first = lp < mid
        want[i, :, 0] = torch.tensor([8, 3] if a_first else [1, 8])
        wrong[i, :, 0] = torch.tensor([1, 8] if a_first else [8, 3])
        i += 1
    assert i == count
    return lc, cn, want, wrong
