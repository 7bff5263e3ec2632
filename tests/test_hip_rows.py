"""Per-launch GPU tests of the row kernels of norm_embed.hip -- embed_ln_kernel, embed_pair_kernel, ln_rows_kernel, ln_pair_kernel, pairify_kernel (and
transpose_f32_kernel in front of the embedding entries) -- through mb_layernorm, mb_layernorm_f4_seq, mb_layernorm_pair, mb_pairify, mb_embed_ln and
mb_embed_pair (include/maskbit_hip_diag.h): the vector paths (d = 768 / 1024), the scalar path at whole and ragged widths up to its widest row, tail
blocks with 1, 2 and 3 live waves, every combination of optional outputs, the 65 / 257 / 1025-row e2m1 scale layouts, the mask token, the drop flag,
the embedding-table path and the two-kernel fallback of the pair forward.

Every judgement is made by tests/rows_reference.py on the CPU (its check_* functions; tests/test_rows_cpu.py shows that they reject wrong kernels):
copies of a kernel's own fp32 rows are compared EXACTLY, fp32 rows and statistics against float64 within max(4 E_ref, 2 ulp) with E_ref measured per
case from a plain fp32 restatement.  Output buffers are filled with 0xA5 and carry guard rows / bytes that must survive.  Each case prints its figures
(`ROWS|case|quantity|E_ref|kernel error|bound`); profiles/rows_kernels.md records them."""
import functools
import itertools

import pytest
import torch

import rows_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12
F4_KEYS = ("x4", "xl4")


@functools.lru_cache(maxsize=None)
def _lib():
    from maskbit_amd import _lib as L
    return L.load()


def _err():
    return _lib().mb_last_error().decode()


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _outputs(rows, d, keys, nseq=0, seq_rows=0, f4_rows=None):
    """Sentinel-filled device buffers for the outputs named in keys (x32, xh, xlo: [rows, d]; stats [rows, 2]; x4 / xl4 [f4_rows or rows, 2 d] + scales)."""
    o = dict.fromkeys(("x32", "xh", "xlo", "stats", "x4", "x4s", "xl4", "xl4s"))
    for k, dt in (("x32", torch.float32), ("xh", torch.float16), ("xlo", torch.float16)):
        if k in keys:
            o[k] = R.alloc(rows, d, dt, DEV)
    if "stats" in keys:
        o["stats"] = R.alloc(rows, 2, torch.float32, DEV)
    for k in F4_KEYS:
        if k in keys:
            o[k], o[k + "s"] = R.alloc(f4_rows or rows, 2 * d, torch.uint8, DEV), R.alloc_scales(d, nseq, seq_rows, DEV)
    return o


def _cpu(o):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items() if v is not None}


def _show(label, figures):
    for k, (e_ref, err, bound) in figures.items():
        print(f"\nROWS|{label}|{k}|{e_ref:.3e}|{err:.3e}|{bound:.3e}")


def _all_sentinel(o, what):
    for k, v in _cpu(o).items():
        R.check_sentinel(v.reshape(1, -1) if v.dim() == 1 else v, f"{what}: {k} after a refused call")


# --------------------------------------------------------------------------- launches
def run_layernorm(y, g, b, M, d, keys, eps=EPS):
    o = _outputs(M, d, keys)
    rc = _lib().mb_layernorm(_p(y), _p(g), _p(b), eps, _p(o["x32"]), _p(o["xh"]), _p(o["xlo"]), _p(o["stats"]), M, d, _stream())
    assert rc == 0, _err()
    return _cpu(o)


def run_layernorm_f4(y, g, b, M, d, seq_rows, keys, eps=EPS):
    o = _outputs(M, d, keys, M // seq_rows, seq_rows)
    rc = _lib().mb_layernorm_f4_seq(_p(y), _p(g), _p(b), eps, _p(o["x32"]), _p(o["xh"]), _p(o["x4"]), _p(o["x4s"]), _p(o["xl4"]), _p(o["xl4s"]), M, d,
                                    seq_rows, _stream())
    assert rc == 0, _err()
    return _cpu(o)


def run_pair(y, g, b, P, d, seq_rows, keys, eps=EPS, expect=0):
    o = _outputs(2 * P, d, keys, P // seq_rows if seq_rows else 0, seq_rows)
    rc = _lib().mb_layernorm_pair(_p(y), _p(g), _p(b), eps, _p(o["xh"]), _p(o["stats"]), _p(o["x4"]), _p(o["x4s"]), _p(o["xl4"]), _p(o["xl4s"]), P, d,
                                  seq_rows, _stream())
    assert rc == expect, (rc, _err())
    if expect:
        _all_sentinel(o, f"mb_layernorm_pair d={d}")
    return _cpu(o)


def run_pairify(x32, P, d, seq_rows, keys, expect=0):
    o = _outputs(2 * P, d, keys, P // seq_rows if seq_rows else 0, seq_rows)
    rc = _lib().mb_pairify(_p(x32), _p(o["xh"]), _p(o["x4"]), _p(o["x4s"]), _p(o["xl4"]), _p(o["xl4s"]), P, d, seq_rows, _stream())
    assert rc == expect, (rc, _err())
    if expect:
        _all_sentinel(o, f"mb_pairify d={d}")
    return _cpu(o)


def _embed_dev(case):
    return {k: _dev(v) if torch.is_tensor(v) else v for k, v in case.items()}


def run_embed(cd, drop, keys, tokens=None, labels=None):
    """mb_embed_ln on the device copy cd of a case (tokens / labels: another batch over the same weights) -> (outputs on the CPU, the device buffers)."""
    tokens = cd["tokens"] if tokens is None else tokens
    labels = cd["labels"] if labels is None else labels
    nb, seq, m = tokens.shape
    d = cd["class_emb"].shape[1]
    o = _outputs(nb * (seq + 1), d, keys, nb, seq + 1)
    rc = _lib().mb_embed_ln(_p(tokens), _p(labels), _p(drop), _p(cd.get("w_in")), _p(cd.get("b_in")), _p(cd["class_emb"]), _p(cd["pos"]), _p(cd["gamma"]),
                            _p(cd["beta"]), _p(cd.get("tables")), _p(o["x32"]), _p(o["xh"]), _p(o["xlo"]), _p(o["x4"]), _p(o["x4s"]), _p(o["xl4"]),
                            _p(o["xl4s"]), nb, seq, m, cd["gbits"], d, cd["nclass"], _stream())
    assert rc == 0, _err()
    return _cpu(o), o


def run_embed_pair(cd, keys, expect=0):
    nb, seq, m = cd["tokens"].shape
    d = cd["class_emb"].shape[1]
    P = nb * (seq + 1)
    o = _outputs(2 * P, d, keys, nb, seq + 1)
    rc = _lib().mb_embed_pair(_p(cd["tokens"]), _p(cd["labels"]), _p(cd.get("w_in")), _p(cd.get("b_in")), _p(cd["class_emb"]), _p(cd["pos"]),
                              _p(cd["gamma"]), _p(cd["beta"]), _p(cd.get("tables")), _p(o["x32"]), _p(o["xh"]), _p(o["x4"]), _p(o["x4s"]), _p(o["xl4"]),
                              _p(o["xl4s"]), nb, seq, m, cd["gbits"], d, cd["nclass"], _stream())
    assert rc == expect, (rc, _err())
    if expect:
        _all_sentinel(o, "mb_embed_pair")
    return _cpu(o)


# --------------------------------------------------------------------------- mb_layernorm
LN_D = [1024, 768, 2048, 128, 64, 100, 36, 1]       # vector paths; scalar path: MAXS rows, whole widths, ragged widths, one column
LN_M = [258, 5, 3, 1]                               # 258 = 64 full blocks + a tail of 2 live waves; tails of 1 and 3; one wave alone
LN_ROWS = 258
FAMILIES = ["gauss", "large_mean", "channel_40_sigma", "equal_rows", "zero_rows"]


@functools.lru_cache(maxsize=None)
def _ln_case(d, family):
    """y [258, d], gamma, beta on the CPU, and E_ref of the case = the plain fp32 restatement's largest error over these 258 rows.  Launches over fewer
    rows take the first M of them and are held to the same E_ref: over one or three rows the restatement's own error is a lucky or unlucky draw
    (profiles/rows_kernels.md: 0.13 ulp of the mean on the one row of d = 2048 where the kernel, like the restatement on other rows, has 2)."""
    g = torch.Generator().manual_seed(1000 * d + FAMILIES.index(family))
    y = torch.randn(LN_ROWS, d, generator=g)
    if family == "large_mean":
        y = y + 1000.0
    elif family == "channel_40_sigma":
        y[:, min(5, d - 1)] += 40.0
    elif family == "equal_rows":
        # row k holds (k + 1) / 2 in every column: every partial sum of such a row is a multiple of 1/2 below 2^24, so ANY summation order gives the
        # mean exactly and the row normalises to beta itself.  (Values whose sum rounds leave a last-ulp offset that eps = 1e-12 blows up to +-gamma,
        # in torch's fp32 LayerNorm as in the kernel: that is the operation, not a fault.)
        y = ((torch.arange(LN_ROWS) + 1) * 0.5).unsqueeze(1).expand(LN_ROWS, d).clone()
    elif family == "zero_rows":
        y = torch.zeros(LN_ROWS, d)
    gam, bet = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2
    return y, gam, bet, R.layernorm_e_ref(y, gam, bet, EPS)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_rows(d, family):
    """ln_rows_kernel<4 / 3 / 0>, all four outputs, at every M: x_h16 and x_lo exact copies of x_f32, x_f32 exactly ln_affine(y, its own stats), x_f32
    and {mean, rstd} within the measured bound of float64, rows past M untouched; rows of equal values and zero rows give beta bit for bit."""
    y, g, b, e_ref = _ln_case(d, family)
    yd, gd, bd = _dev(y), _dev(g), _dev(b)
    for M in LN_M:
        out = run_layernorm(yd, gd, bd, M, d, ("x32", "xh", "xlo", "stats"))
        figs = R.Figures()
        try:
            R.check_layernorm(out, y, g, b, EPS, M, f"layernorm d={d} M={M} {family}", figures=figs, e_ref=e_ref)
        finally:
            _show(f"layernorm d={d} M={M} {family}", figs)
        if family in ("equal_rows", "zero_rows"):
            R.check_bits(out["x32"][:M], b.expand(M, d).contiguous(), f"layernorm d={d} M={M} {family}: x_f32 against beta")


KEYS4 = ("x32", "xh", "xlo", "stats")
SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(KEYS4, n)]


@pytest.mark.parametrize("d", LN_D)
def test_layernorm_every_combination_of_outputs(d):
    """Each of the 15 non-empty sets of {x_f32, x_h16, x_lo, stats}: what a launch writes is, bit for bit, what the launch with all four wrote (checked
    by test_layernorm_rows on the same input), and its guard rows survive -- no output depends on which others were asked for."""
    y, g, b, _ = _ln_case(d, "gauss")
    yd, gd, bd = _dev(y), _dev(g), _dev(b)
    for M in LN_M:
        full = run_layernorm(yd, gd, bd, M, d, KEYS4)
        for keys in SUBSETS:
            out = run_layernorm(yd, gd, bd, M, d, keys)
            assert set(out) == set(keys)
            R.check_guard_rows(out, M, f"layernorm d={d} M={M} outputs {keys}")
            for k in keys:
                R.check_bits(out[k][:M], full[k][:M], f"layernorm d={d} M={M} outputs {keys}: {k} against the launch with every output")


def test_layernorm_refusals():
    z = torch.zeros(4096, device=DEV)
    lib = _lib()
    assert lib.mb_layernorm(_p(z), _p(z), _p(z), EPS, _p(z), None, None, None, 1, 2049, _stream()) == -1
    assert lib.mb_layernorm(None, _p(z), _p(z), EPS, _p(z), None, None, None, 1, 64, _stream()) == -1
    assert lib.mb_layernorm(_p(z), None, _p(z), EPS, _p(z), None, None, None, 1, 64, _stream()) == -1


# --------------------------------------------------------------------------- mb_layernorm_f4_seq
U13 = 1.0 + 1.5 * 2.0 ** -13       # fp16(U13) = 1: its lo half is 1.5 * 2^-13, mantissa exactly 1.5


@functools.lru_cache(maxsize=None)
def _f4_case(d, seq_rows, nseq):
    """Gaussian rows with a 40-sigma channel in block 0; gamma = 0 on blocks 1, 2, 3 so that their normalised values are beta itself: block 1 all
    zero (scale byte 0, codes 0); block 2 with largest value 1.5 and largest lo half 1.5 * 2^-13 -- mantissa exactly 1.5, the last maximum of a
    binade under the no-saturation rule --; block 3 the same plus one fp32 ulp, the first of the next."""
    g = torch.Generator().manual_seed(d + seq_rows)
    M = seq_rows * nseq
    y = torch.randn(M, d, generator=g) * 3.0
    y[:, 5] += 40.0
    gam, bet = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2
    gam[64:256] = 0.0
    bet[64:128] = 0.0
    quiet = torch.randint(-64, 65, (64,), generator=g).float() / 64.0           # fp16 values (lo half 0) of magnitude <= 1
    bet[128:192] = quiet
    bet[128], bet[129] = 1.5, U13
    bet[192:256] = quiet
    bet[192], bet[193] = 1.5 + 2.0 ** -23, U13 + 2.0 ** -23
    return y, gam, bet


@pytest.mark.parametrize("keys", [("x4",), ("xl4",), ("x4", "xl4")], ids=["values", "lo", "both"])
@pytest.mark.parametrize("seq_rows,nseq", [(65, 3), (257, 2), (1025, 1)])
@pytest.mark.parametrize("d", [1024, 768])
def test_layernorm_e2m1_copies(d, seq_rows, nseq, keys):
    """ln_rows_kernel's e2m1 producer over 1, 4 and 16 token groups per sequence: bytes and lane-ordered scale bytes exactly those of the kernel's own
    x_f32 (and of its fp32 lo halves); class-token rows, bytes d/2 .. 2d and the guards untouched; x_f32 within the bound of float64."""
    y, g, b = _f4_case(d, seq_rows, nseq)
    M = seq_rows * nseq
    label = f"layernorm_f4 d={d} seq_rows={seq_rows} nseq={nseq} {'+'.join(keys)}"
    out = run_layernorm_f4(_dev(y), _dev(g), _dev(b), M, d, seq_rows, ("x32", "xh") + keys)
    figs = R.Figures()
    try:
        R.check_layernorm(out, y, g, b, EPS, M, label, nseq, seq_rows, figures=figs)
    finally:
        _show(label, figs)
    # the case holds what it claims: blocks 1 .. 3 of x_f32 are beta, and the reference's own scale bytes step by one between blocks 2 and 3
    R.check_bits(out["x32"][:M, 64:256], b[64:256].expand(M, 192).contiguous(), f"{label}: gamma = 0 columns against beta")
    for v in (out["x32"][:1], R.lo32_of(out["x32"][:1])):
        _, sbyte, _, _ = R.f4_expected(torch.cat([v] * seq_rows), 1, seq_rows)
        assert int(sbyte[0, 1]) == 0 and int(sbyte[0, 3]) == int(sbyte[0, 2]) + 1


def test_layernorm_f4_refusals():
    z = torch.zeros(4096, device=DEV)
    u = torch.full((4096,), R.SENT, device=DEV, dtype=torch.uint8)
    lib = _lib()
    call = lambda x4, x4s, xl4, xl4s, M, d, sr: lib.mb_layernorm_f4_seq(_p(z), _p(z), _p(z), EPS, _p(z), None, _p(x4), _p(x4s), _p(xl4), _p(xl4s), M, d, sr, _stream())
    assert call(u, None, None, None, 65, 768, 65) == -1            # values without their scales
    assert call(None, None, u, None, 65, 768, 65) == -1
    assert call(None, u, None, None, 65, 768, 65) == -1            # scales without values
    assert call(None, None, None, None, 65, 768, 65) == -1         # no e2m1 output at all
    assert call(u, u, None, None, 65, 128, 65) == -1               # scalar path widths
    assert call(u, u, None, None, 66, 768, 66) == -1               # 65 tokens: no whole 64-token groups
    assert call(u, u, None, None, 100, 768, 65) == -1              # not whole sequences
    torch.cuda.synchronize()
    assert bool((u == R.SENT).all())


# --------------------------------------------------------------------------- mb_layernorm_pair, mb_pairify
PAIR_SHAPES = [(65, 65), (514, 257), (5, 0)]         # (P, seq_rows): one sequence of 64 tokens; two of 256; a tail block alone without e2m1 outputs


@functools.lru_cache(maxsize=None)
def _pair_case(d, P):
    """y [2 P, d]: the twins are the conditional rows plus a small perturbation, equal to them on every third row and unrelated on every fifth."""
    g = torch.Generator().manual_seed(7 * d + P)
    yc = torch.randn(P, d, generator=g) * 2.0 + 0.5
    yu = yc + torch.randn(P, d, generator=g) * 0.05
    yu[4::5] = torch.randn(yu[4::5].shape, generator=g) * 2.0
    yu[0::3] = yc[0::3]
    return torch.cat([yc, yu]), torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2


def _f4_sets(seq_rows):
    return [(), ("x4",), ("xl4",), F4_KEYS] if seq_rows else [()]


@pytest.mark.parametrize("P,seq_rows", PAIR_SHAPES)
@pytest.mark.parametrize("d", [1024, 768])
def test_layernorm_pair(d, P, seq_rows):
    """ln_pair_kernel<4 / 3>: conditional rows fp16(ln_affine(y, own stats)), twin rows fp16 of the fp32 difference, the e2m1 set from the conditional
    rows alone, both rows' stats within the bound of float64; with and without stats and each part of the e2m1 set the outputs stay the same bits."""
    y, g, b = _pair_case(d, P)
    yd, gd, bd = _dev(y), _dev(g), _dev(b)
    label = f"layernorm_pair d={d} P={P}"
    full = run_pair(yd, gd, bd, P, d, seq_rows, ("xh", "stats") + _f4_sets(seq_rows)[-1])
    figs = R.Figures()
    try:
        R.check_pair(full, y, g, b, EPS, P, label, P // seq_rows if seq_rows else 0, seq_rows, figures=figs)
    finally:
        _show(label, figs)
    same = torch.arange(P)[0::3]
    assert not bool(R._bits(full["xh"][P:2 * P][same]).any()), "twins equal to their conditional rows must give all-zero difference rows"
    for stats, f4 in itertools.product((True, False), _f4_sets(seq_rows)):
        keys = ("xh",) + (("stats",) if stats else ()) + f4
        out = run_pair(yd, gd, bd, P, d, seq_rows, keys)
        R.check_guard_rows(out, 2 * P, f"{label} outputs {keys}")
        for k, v in out.items():
            R.check_bits(*(t.reshape(1, -1) if t.dim() == 1 else t for t in (v, full[k])), f"{label} outputs {keys}: {k} against the launch with every output")


@pytest.mark.parametrize("P,seq_rows", PAIR_SHAPES)
@pytest.mark.parametrize("d", [1024, 768])
def test_pairify(d, P, seq_rows):
    """pairify_kernel<4 / 3>, a pure function of its input: every output exactly, for each part of the e2m1 set; and with twins equal to the
    conditional rows the difference rows are all zero bits."""
    x32, _, _ = _pair_case(d, P)
    for f4 in _f4_sets(seq_rows):
        out = run_pairify(_dev(x32), P, d, seq_rows, ("xh",) + f4)
        R.check_pairify(out, x32, P, f"pairify d={d} P={P} {f4}", P // seq_rows if seq_rows else 0, seq_rows)
    eq = torch.cat([x32[:P], x32[:P]])
    out = run_pairify(_dev(eq), P, d, seq_rows, ("xh",) + _f4_sets(seq_rows)[-1])
    R.check_pairify(out, eq, P, f"pairify d={d} P={P} twin == conditional", P // seq_rows if seq_rows else 0, seq_rows)
    assert not bool(R._bits(out["xh"][P:2 * P]).any())


@pytest.mark.parametrize("d", [128, 64, 2048, 100])
def test_pair_forms_refuse_other_widths(d):
    """Widths other than 768 / 1024: refused (-3; with an e2m1 output, or beyond 2048, -1) and nothing written."""
    y = torch.randn(10, d, device=DEV)
    g = torch.ones(d, device=DEV)
    run_pair(y, g, g, 5, d, 0, ("xh", "stats"), expect=-3)
    run_pairify(y, 5, d, 0, ("xh",), expect=-3)
    y65 = torch.randn(130, d, device=DEV)
    run_pair(y65, g, g, 65, d, 65, ("xh", "stats", "x4"), expect=-1)
    run_pairify(y65, 65, d, 65, ("xh", "xl4"), expect=-1)
    lib = _lib()
    assert lib.mb_layernorm_pair(_p(y), _p(g), _p(g), EPS, None, None, None, None, None, None, 5, 768, 0, _stream()) == -1      # x_h16 is required
    assert lib.mb_pairify(_p(y), None, None, None, None, None, 5, 768, 0, _stream()) == -1
    assert lib.mb_pairify(_p(y), _p(y), None, None, None, None, 5, 2049, 0, _stream()) == -1


# --------------------------------------------------------------------------- mb_embed_ln
NCLASS = 10
EMBED_BITS = [(12, 2), (10, 1), (14, 2), (18, 2), (24, 2), (12, 3)]           # 24 bits = the edge of the kernels' sign masks (MAXBITS)
EMBED_D = [1024, 768, 128, 100]
EMBED_SHAPES = [(3, 4), (2, 64), (1, 256)]                                     # (nb, seq): 15 rows (tail of 3 waves), 130 (tail of 2), 257 (tail of 1)


def _edge_tokens(g, nb, seq, m, gbits, turn):
    """Random group indices with, in sequence `turn % nb`: token 0 = index 0 in every group, token 1 = 2^gbits - 1 in every group, token 2 = the mask
    token in ONE group only (the others random), token 3 = the mask token in all groups."""
    tok = torch.randint(0, 1 << gbits, (nb, seq, m), generator=g)
    s = turn % nb
    tok[s, 0] = 0
    tok[s, 1] = (1 << gbits) - 1
    tok[s, 2, turn % m] = 1 << gbits
    tok[s, 3] = 1 << gbits
    return tok


def _labels(nb, turn):
    """0, nclass - 1 and nclass, starting at a different one per case so that one-sequence batches meet all three across the cases."""
    return torch.tensor([(0, NCLASS - 1, NCLASS)[(turn + i) % 3] for i in range(nb)])


@functools.lru_cache(maxsize=None)
def _embed_case(bits, splits, d, nb, seq, family, tables=False):
    turn = bits + splits + d + nb
    g = torch.Generator().manual_seed(turn * 31 + seq + (family == "exact"))
    gbits = bits // splits
    if family == "exact":            # small multiples of 2^-8: every partial sum of the kernel's chain is exact, the pre-LayerNorm row is known exactly
        rn = lambda *s: torch.randint(-8, 9, s, generator=g).float() / 256.0
    else:
        rn = lambda *s: torch.randn(*s, generator=g) * 0.05
    c = dict(tokens=_edge_tokens(g, nb, seq, splits, gbits, turn), labels=_labels(nb, turn), gbits=gbits, nclass=NCLASS, class_emb=rn(NCLASS + 1, d),
             pos=rn(seq + 1, d), gamma=torch.rand(d, generator=g) + 0.5, beta=torch.randn(d, generator=g) * 0.2)
    if tables:
        c["tables"] = rn(splits, (1 << gbits) + 1, d)
    else:
        c.update(w_in=rn(d, bits), b_in=rn(d))
    return c


def _mixed_drop(nb, labels):
    """A drop vector with both values where there are two sequences, set on a sequence whose label is not nclass already where there is one."""
    drop = torch.zeros(nb, dtype=torch.uint8)
    live = [i for i in range(nb) if int(labels[i]) != NCLASS]
    drop[live[-1] if live else 0] = 1
    return drop


def _embed_checks(c, label):
    nb, seq, _ = c["tokens"].shape
    d = c["class_emb"].shape[1]
    cd = _embed_dev(c)
    keys = ("x32", "xh", "xlo") + (F4_KEYS if seq % 64 == 0 and d in (768, 1024) else ())
    for name, drop in (("no drop", None), ("mixed drop", _mixed_drop(nb, c["labels"])), ("all dropped", torch.ones(nb, dtype=torch.uint8))):
        out, _ = run_embed(cd, _dev(drop), keys)
        figs = R.Figures()
        try:
            R.check_embed(out, c, drop, f"{label} {name}", figures=figs)
        finally:
            _show(f"{label} {name}", figs)
    out, _ = run_embed(cd, None, ("x32", "xh"))                   # the required outputs alone: the same bits
    full, _ = run_embed(cd, None, keys)
    R.check_guard_rows(out, nb * (seq + 1), f"{label}: required outputs alone")
    for k in ("x32", "xh"):
        R.check_bits(out[k], full[k], f"{label}: {k} without the optional outputs")
    if family_is_exact(c):
        # the exact family: the float64 statement of the pre-LayerNorm row and the fp32 chain agree to the last bit, so the bound above was LayerNorm's alone
        args = {k: c.get(k) for k in ("gbits", "nclass", "class_emb", "pos", "w_in", "b_in", "tables")}
        assert torch.equal(R.embed_rows32(c["tokens"], c["labels"], None, **args).double(), R.embed_rows64(c["tokens"], c["labels"], None, **args))


def family_is_exact(c):
    return bool((c["class_emb"] * 256 == (c["class_emb"] * 256).round()).all())


@pytest.mark.parametrize("family", ["exact", "gauss"])
@pytest.mark.parametrize("nb,seq", EMBED_SHAPES)
@pytest.mark.parametrize("d", EMBED_D)
@pytest.mark.parametrize("bits,splits", EMBED_BITS)
def test_embed_ln_bit_projection(bits, splits, d, nb, seq, family):
    """embed_ln_kernel<4 / 3 / 0>, bit-projection input: index 0, all ones, the mask token in one group and in all, labels 0 / nclass - 1 / nclass,
    without drop, with a mixed drop vector and with every label dropped; x_f32 within the measured bound of float64 (an O(1) error for a wrong sign,
    bit order, position or class row), x_h16 / x_lo / the e2m1 set exactly from the kernel's own x_f32."""
    _embed_checks(_embed_case(bits, splits, d, nb, seq, family), f"embed_ln bits={bits}/{splits} d={d} nb={nb} seq={seq} {family}")


@pytest.mark.parametrize("family", ["exact", "gauss"])
@pytest.mark.parametrize("nb,seq", EMBED_SHAPES)
@pytest.mark.parametrize("d", EMBED_D)
@pytest.mark.parametrize("m,gbits", [(1, 10), (2, 6), (8, 3)])
def test_embed_ln_tables(m, gbits, d, nb, seq, family):
    """The embedding-table input (Bert): 1, 2 and the most (8) tables, row 2^gbits of each the mask token's; weight and bias NULL."""
    _embed_checks(_embed_case(m * gbits, m, d, nb, seq, family, tables=True), f"embed_ln tables={m}x{gbits} d={d} nb={nb} seq={seq} {family}")


def test_embed_refusals():
    c = _embed_dev(_embed_case(12, 2, 128, 3, 4, "gauss"))
    t = _embed_dev(_embed_case(24, 8, 128, 3, 4, "gauss", tables=True))
    o = _outputs(15, 128, ("x32", "xh", "x4"), 1, 65)
    lib = _lib()

    def call(cd, x32=o["x32"], xh=o["xh"], x4=None, x4s=None, m=2, gbits=6, d=128, seq=4, **null):
        a = {k: (None if k in null else cd.get(k)) for k in ("tokens", "labels", "w_in", "b_in", "class_emb", "pos", "gamma", "beta", "tables")}
        return lib.mb_embed_ln(_p(a["tokens"]), _p(a["labels"]), None, _p(a["w_in"]), _p(a["b_in"]), _p(a["class_emb"]), _p(a["pos"]), _p(a["gamma"]),
                               _p(a["beta"]), _p(a["tables"]), _p(x32), _p(xh), None, _p(x4), _p(x4s), None, None, 3, seq, m, gbits, d, NCLASS, _stream())
    for k in ("tokens", "labels", "w_in", "b_in", "class_emb", "pos", "gamma", "beta"):
        assert call(c, **{k: True}) == -1, k
    assert call(c, x32=None) == -1 and call(c, xh=None) == -1      # the kernel forms both addresses unconditionally: required
    assert call(c, d=2049) == -1
    assert call(c, m=5, gbits=5) == -1                             # 25 bits
    assert call(t, m=9, gbits=2) == -1                             # 9 tables
    assert call(c, x4=o["x4"], x4s=o["x4s"]) == -1                 # e2m1 at d = 128
    assert call(c, x4=o["x4"], x4s=o["x4s"], d=768, seq=4) == -1   # e2m1 at a sequence of 4 tokens
    assert call(c, x4=o["x4"], d=768, seq=64) == -1                # values without their scales
    _all_sentinel(o, "mb_embed_ln")


# --------------------------------------------------------------------------- mb_embed_pair
@pytest.mark.parametrize("bits,splits", [(12, 2), (24, 2)])
@pytest.mark.parametrize("nb,seq", [(3, 64), (2, 256)])
@pytest.mark.parametrize("d", [1024, 768])
def test_embed_pair_equals_the_two_kernel_path(d, nb, seq, bits, splits):
    """embed_pair_kernel<4 / 3> against mb_embed_ln over [conditional | twins with drop = 1] followed by mb_pairify on that launch's x_f32 -- the
    engine's fallback in front of the pair forward --: x_f32 (both halves), x_h16, the e2m1 set and the scales equal bit for bit; the twin half of
    x_h16 all zero bits on image-token rows and on the class row of a label that is nclass already, nonzero on the other class rows."""
    c = _embed_case(bits, splits, d, nb, seq, "gauss")
    cd = _embed_dev(c)
    P = nb * (seq + 1)
    label = f"embed_pair bits={bits}/{splits} d={d} nb={nb} seq={seq}"
    for f4 in [(), F4_KEYS]:
        pair = run_embed_pair(cd, ("x32", "xh") + f4)
        drop = torch.tensor([0] * nb + [1] * nb, dtype=torch.uint8, device=DEV)
        ln, ln_dev = run_embed(cd, drop, ("x32", "xh"), tokens=torch.cat([cd["tokens"]] * 2), labels=torch.cat([cd["labels"]] * 2))
        R.check_embed(ln, dict(c, tokens=torch.cat([c["tokens"]] * 2), labels=torch.cat([c["labels"]] * 2)), drop.cpu(), f"{label}: embed_ln over both halves")
        two = run_pairify(ln_dev["x32"], P, d, seq + 1, ("xh",) + f4)
        R.check_pairify(two, ln["x32"], P, f"{label}: pairify", nb, seq + 1)
        two["x32"] = ln["x32"]
        R.check_embed_pair(pair, two, c, f"{label} {f4}")


def test_embed_pair_label_nclass_gives_a_zero_class_row():
    c = dict(_embed_case(12, 2, 768, 3, 64, "gauss"))
    c["labels"] = torch.tensor([NCLASS, 3, NCLASS])
    pair = run_embed_pair(_embed_dev(c), ("x32", "xh"))
    P = 3 * 65
    R.check_guard_rows(pair, 2 * P, "embed_pair labels nclass")
    twin = pair["xh"][P:2 * P].reshape(3, 65, 768)
    assert not bool(R._bits(twin[0]).any()) and not bool(R._bits(twin[2]).any()) and bool(R._bits(twin[1, 64]).any()) and not bool(R._bits(twin[1, :64]).any())


def test_embed_pair_refusals():
    """Tables, a scalar-path width and more than 24 bits are the two-kernel path's: -3, nothing launched, every buffer still the sentinel."""
    run_embed_pair(_embed_dev(_embed_case(12, 2, 768, 3, 64, "gauss", tables=True)), ("x32", "xh"), expect=-3)
    run_embed_pair(_embed_dev(_embed_case(12, 2, 128, 3, 64, "gauss")), ("x32", "xh"), expect=-3)
    wide = dict(_embed_case(24, 2, 768, 3, 64, "gauss"))
    wide["gbits"] = 13                                             # 26 bits claimed over the same buffers: refused in front of any read
    run_embed_pair(_embed_dev(wide), ("x32", "xh"), expect=-3)
