"""CPU tests of tests/rows_reference.py, the reference of the row kernels (norm_embed.hip): its float64 statements agree with the oracle and with the
parameters of the product's modules, and its checkers accept a faithful fp32 emulation of each kernel and reject every mutated one by name."""
import pytest
import torch

import rows_reference as R
from hip_helpers import f4_codes, f4_scale_index
from oracle import maskbit_oracle as O


# --------------------------------------------------------------------------- the float64 statements
def _tiny(kind):
    return O.GenCfg(bits=12, splits=2, hidden=128, depth=1, heads=4, mlp=256, seq=16, nclass=10, kind=kind)


def _tiny_tokens(cfg, nb=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, cfg.group_codes, (nb, cfg.seq, cfg.splits), generator=g)
    tok[0, 0] = 0
    tok[0, 1] = cfg.group_codes - 1
    tok[0, 2, 0] = cfg.group_codes                                 # the mask token in one group only
    tok[0, 3] = cfg.group_codes                                    # ... and in all
    return tok, torch.tensor([0, cfg.nclass - 1, cfg.nclass])[:nb]


def _oracle_rows(sd, cfg, tokens, labels, drop):
    """The embedding rows and the first LayerNorm as the oracle's forward states them (lfq_bert_forward / bert_forward up to _trunk's first line)."""
    lab = labels.clone()
    if drop is not None:
        lab = torch.where(drop.bool(), torch.full_like(lab, cfg.nclass), lab)
    if cfg.kind == "bert":
        x = sum(sd[f"tok_emb_list.{g}.weight"][tokens[..., g]] for g in range(cfg.splits))
    else:
        x = torch.nn.functional.linear(O.token_bit_vectors(tokens, cfg).double(), sd["input_proj.weight"], sd["input_proj.bias"])
    x = torch.cat([x, sd["class_emb.weight"][lab].unsqueeze(1)], dim=1) + sd["pos_emb"]
    return x, O._ln(x, sd, "first_layer.0", 1e-12)


def _statement_args(sd, cfg):
    a = dict(gbits=cfg.group_bits, nclass=cfg.nclass, class_emb=sd["class_emb.weight"], pos=sd["pos_emb"][0])
    if cfg.kind == "bert":
        a["tables"] = torch.stack([sd[f"tok_emb_list.{g}.weight"] for g in range(cfg.splits)])
    else:
        a.update(w_in=sd["input_proj.weight"], b_in=sd["input_proj.bias"])
    return a


@pytest.mark.parametrize("kind", ["lfq", "bert"])
@pytest.mark.parametrize("drop", [None, [1, 0, 1]])
def test_statements_agree_with_the_oracle_and_the_modules(kind, drop):
    """embed_rows64 / layernorm64 against the oracle (token_bit_vectors, _ln) in float64, and fed from the parameters of maskbit_amd's own LFQBert /
    Bert (strict load, .double()) -- the modules themselves run on the device only, so it is their parameter tree and their mask_token / drop_label
    that are pinned here."""
    import maskbit_amd
    cfg = _tiny(kind)
    sd32 = O.make_generator_weights(cfg, seed=5)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    tokens, labels = _tiny_tokens(cfg)
    dr = None if drop is None else torch.tensor(drop, dtype=torch.uint8)
    want_pre, want = _oracle_rows(sd, cfg, tokens, labels, dr)
    pre = R.embed_rows64(tokens, labels, dr, **_statement_args(sd, cfg))
    assert float((pre - want_pre).abs().max()) < 1e-14
    got, mean, rstd = R.layernorm64(pre, sd["first_layer.0.weight"], sd["first_layer.0.bias"])
    assert float((got - want).abs().max()) < 1e-12
    assert float((mean - pre.mean(-1)).abs().max()) < 1e-15 and float((rstd * torch.sqrt(pre.var(-1, unbiased=False) + 1e-12) - 1).abs().max()) < 1e-12
    cls = maskbit_amd.Bert if kind == "bert" else maskbit_amd.LFQBert
    m = cls(img_size=64, hidden_dim=cfg.hidden, codebook_size=2 ** cfg.bits, codebook_splits=cfg.splits, depth=cfg.depth, heads=cfg.heads,
            mlp_dim=cfg.mlp, nclass=cfg.nclass, input_stride=16)
    m.load_state_dict(sd32, strict=True)
    assert (m.mask_token, m.drop_label, m.seq_len) == (cfg.group_codes, cfg.nclass, cfg.seq)
    msd = m.double().state_dict()
    pre_m = R.embed_rows64(tokens, labels, dr, **{**_statement_args(msd, cfg), "gbits": m.bits // m.splits, "nclass": m.drop_label})
    got_m, _, _ = R.layernorm64(pre_m, msd["first_layer.0.weight"], msd["first_layer.0.bias"])
    assert torch.equal(got_m, got)
    # and the fp32 chain in the kernel's order is the same function
    pre32 = R.embed_rows32(tokens, labels, dr, **_statement_args(sd32, cfg))
    assert float((pre32.double() - pre).abs().max()) < 1e-6


def test_rows_from_stats_decides_midpoints_exactly():
    """The fma of ln_affine: u * g + b lands exactly on an fp32 rounding midpoint, or a hair to either side of it -- float64 alone would round the sum to
    the midpoint and then to even."""
    u, gm, big = 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, 2.0 ** 24 + 2.0            # u * gm = 1 - 2^-46: 70 bits wide next to 2^24
    y = torch.tensor([[u, u, 3.0]])
    g = torch.tensor([gm, gm, 0.5])
    b = torch.tensor([big, -big, 1.0])                 # exact sums 2^24 + 3 - 2^-46 and -(2^24 + 1 + 2^-46); float64 rounds both onto the midpoint
    out = R.rows_from_stats(y, torch.zeros(1), torch.ones(1), g, b)
    assert out[0].tolist() == [big, -big, 2.5]         # (midpoint, then to even, would give 2^24 + 4 and -2^24)
    y2 = torch.tensor([[1.0, 1.0, 3.0]])               # exact ties go to even
    b2 = torch.tensor([2.0 ** 24, big, 1.0])
    assert R.rows_from_stats(y2, torch.zeros(1), torch.ones(1), torch.tensor([1.0, 1.0, 0.5]), b2)[0].tolist() == [2.0 ** 24, 2.0 ** 24 + 4.0, 2.5]


# --------------------------------------------------------------------------- fp32 emulations of the kernels
def _ln_core(y, g, b, eps, mean_cols=None):
    """Two-pass fp32 statistics, then ln_affine -> (x32, stats [R, 2])."""
    y = y.float()
    d = y.shape[1]
    mean = (y[:, :mean_cols].sum(-1) / d) if mean_cols else y.mean(-1)
    rstd = torch.rsqrt(((y - mean.unsqueeze(-1)) ** 2).mean(-1) + eps)
    return R.rows_from_stats(y, mean, rstd, g, b), torch.stack([mean, rstd], dim=1)


def _emu_f4(x4, x4s, v32, nseq, seq_rows, rule="nosat", class_rows=False):
    """fp4_row_store on the CPU: per 64-column block the biased exponent of the largest element (`nosat`: one more when its mantissa exceeds 1.5;
    `sat`: mb_common.h fp4_scale_byte, which lets the largest elements clip), codes of v * 2^(129 - E), the scale byte E - 2 at its lane-ordered index."""
    R_, d = v32.shape
    bits = v32.float().abs().reshape(R_, d // 64, 64).amax(-1).view(torch.int32).long()
    E = (bits >> 23) & 0xFF
    if rule == "nosat":
        E = E + ((bits & 0x7FFFFF) > 0x400000).long()
    mul = torch.where((E >= 2) & (E <= 254), 2.0 ** (129 - E).double(), torch.zeros(E.shape, dtype=torch.float64))
    codes = f4_codes(v32.double().reshape(R_, d // 64, 64) * mul.unsqueeze(-1)).reshape(R_, d)
    groups = (seq_rows - 1) // 64
    for r in range(R_):
        seq, tok = divmod(r, seq_rows)
        if tok == seq_rows - 1 and not class_rows:
            continue
        x4[r, : d // 2] = (codes[r, 0::2] | (codes[r, 1::2] << 4)).to(torch.uint8)
        if tok < seq_rows - 1:
            for blk in range(d // 64):
                x4s[f4_scale_index(blk, nseq, seq, tok, groups)] = int((E[r, blk] - 2).clamp(min=0))


def _emu_store(x32, keys, nseq=0, seq_rows=0, stats=None, **f4kw):
    M, d = x32.shape
    out = {}
    if "x32" in keys:
        out["x32"] = R.alloc(M, d, torch.float32); out["x32"][:M] = x32
    if "xh" in keys:
        out["xh"] = R.alloc(M, d, torch.float16); out["xh"][:M] = R.h16_of(x32)
    if "xlo" in keys:
        out["xlo"] = R.alloc(M, d, torch.float16); out["xlo"][:M] = R.lo_of(x32)
    if stats is not None:
        out["stats"] = R.alloc(M, 2, torch.float32); out["stats"][:M] = stats
    for k, v in (("x4", x32), ("xl4", R.lo32_of(x32))):
        if k in keys:
            out[k], out[k + "s"] = R.alloc(M, 2 * d, torch.uint8), R.alloc_scales(d, nseq, seq_rows)
            _emu_f4(out[k], out[k + "s"], v, nseq, seq_rows, **f4kw)
    return out


ALL = ("x32", "xh", "xlo", "x4", "xl4")


def _emu_layernorm(y, g, b, eps, nseq=0, seq_rows=0, keys=ALL, mean_cols=None, **f4kw):
    x32, st = _ln_core(y, g, b, eps, mean_cols)
    return _emu_store(x32, keys, nseq, seq_rows, stats=st, **f4kw)


def _emu_pairify(x32, P, nseq=0, seq_rows=0, f4=True, twin_of=lambda xc, xu: R.h16_of(xu - xc)):
    d = x32.shape[1]
    out = {"xh": R.alloc(2 * P, d, torch.float16)}
    out["xh"][:P] = R.h16_of(x32[:P])
    out["xh"][P:2 * P] = twin_of(x32[:P].float(), x32[P:2 * P].float())
    if f4:
        for k, v in (("x4", x32[:P].float()), ("xl4", R.lo32_of(x32[:P]))):
            out[k], out[k + "s"] = R.alloc(2 * P, 2 * d, torch.uint8), R.alloc_scales(d, nseq, seq_rows)
            _emu_f4(out[k], out[k + "s"], v, nseq, seq_rows)
    return out


def _emu_pair(y, g, b, eps, P, nseq=0, seq_rows=0, f4=True, **kw):
    x32, st = _ln_core(y[:2 * P], g, b, eps)
    out = _emu_pairify(x32, P, nseq, seq_rows, f4, **kw)
    out["stats"] = R.alloc(2 * P, 2, torch.float32); out["stats"][:2 * P] = st
    return out


def _emu_embed(case, drop, keys=ALL, mask_as_zero=False, msb_first=False):
    c = dict(case)
    gb = c["gbits"]
    if mask_as_zero:
        c["tokens"] = torch.where(c["tokens"] == (1 << gb), torch.zeros_like(c["tokens"]), c["tokens"])
    if msb_first:
        m = c["tokens"].shape[2]
        c["w_in"] = c["w_in"].reshape(-1, m, gb).flip(-1).reshape(-1, m * gb)
    args = {k: c.get(k) for k in ("gbits", "nclass", "class_emb", "pos", "w_in", "b_in", "tables")}
    nb, seq, _ = c["tokens"].shape
    pre = R.embed_rows32(c["tokens"], c["labels"], drop, **args).reshape(nb * (seq + 1), -1)
    x32, _ = _ln_core(pre, c["gamma"], c["beta"], R.LN_EPS)
    f4 = seq % 64 == 0 and x32.shape[1] in (768, 1024)
    return _emu_store(x32, [k for k in keys if f4 or k not in ("x4", "xl4")], nb, seq + 1)


def _emu_embed_two_kernels(case):
    """embed_ln over [conditional | twins with drop = 1] followed by pairify -> {x32, xh, e2m1 set} as embed_pair must write them."""
    nb, seq, _ = case["tokens"].shape
    both = dict(case, tokens=torch.cat([case["tokens"]] * 2), labels=torch.cat([case["labels"]] * 2))
    drop = torch.tensor([0] * nb + [1] * nb, dtype=torch.uint8)
    e = _emu_embed(both, drop, keys=("x32",))
    P = nb * (seq + 1)
    out = _emu_pairify(e["x32"][:2 * P], P, nb, seq + 1)
    out["x32"] = e["x32"]
    return out


def _ln_inputs(M, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, d, generator=g) * 1.5 + 0.25
    return y, torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2


def _embed_case(nb=2, seq=64, d=768, bits=12, splits=2, tables=False, seed=3):
    g = torch.Generator().manual_seed(seed)
    gb, nclass = bits // splits, 10
    tok = torch.randint(0, 1 << gb, (nb, seq, splits), generator=g)
    tok[0, 0] = 0; tok[0, 1] = (1 << gb) - 1; tok[0, 2, 0] = 1 << gb; tok[0, 3] = 1 << gb
    rn = lambda *s: torch.randn(*s, generator=g) * 0.05
    c = dict(tokens=tok, labels=torch.tensor([nclass - 1, 0, nclass])[:nb], gbits=gb, nclass=nclass, class_emb=rn(nclass + 1, d), pos=rn(seq + 1, d),
             gamma=torch.rand(d, generator=g) + 0.5, beta=rn(d))
    if tables:
        c["tables"] = rn(splits, (1 << gb) + 1, d)
    else:
        c.update(w_in=rn(d, bits), b_in=rn(d))
    return c


# --------------------------------------------------------------------------- the faithful emulations pass
def test_faithful_emulations_pass_every_checker():
    y, g, b = _ln_inputs(2 * 65, 768)
    R.check_layernorm(_emu_layernorm(y, g, b, 1e-12, 2, 65), y, g, b, 1e-12, 130, "layernorm", 2, 65, R.Figures())
    y2, g2, b2 = _ln_inputs(7, 100, seed=1)
    R.check_layernorm(_emu_layernorm(y2, g2, b2, 1e-12, keys=("x32", "xh", "xlo")), y2, g2, b2, 1e-12, 7, "scalar layernorm")
    R.check_pair(_emu_pair(y, g, b, 1e-12, 65, 1, 65), y, g, b, 1e-12, 65, "pair", 1, 65)
    R.check_pair(_emu_pair(y[:10], g, b, 1e-12, 5, f4=False), y[:10], g, b, 1e-12, 5, "pair tail")
    R.check_pairify(_emu_pairify(y, 65, 1, 65), y, 65, "pairify", 1, 65)
    for tables in (False, True):
        c = _embed_case(tables=tables)
        for drop in (None, torch.tensor([1, 0], dtype=torch.uint8)):
            R.check_embed(_emu_embed(c, drop), c, drop, "embed")
    c = _embed_case()
    two = _emu_embed_two_kernels(c)
    R.check_embed_pair({k: v.clone() for k, v in two.items()}, two, c, "embed_pair")


# --------------------------------------------------------------------------- every mutation is rejected by name
def _mut_lane_swap():
    y, g, b = _ln_inputs(5, 1024)
    x32, st = _ln_core(y, g, b, 1e-12)
    x32[:, 4:8], x32[:, 8:12] = x32[:, 8:12].clone(), x32[:, 4:8].clone()          # lanes 1 and 2 store each other's float4
    R.check_layernorm(_emu_store(x32, ("x32", "xh", "xlo"), stats=st), y, g, b, 1e-12, 5, "m")


def _mut_lane_swap_pairify():
    y, _, _ = _ln_inputs(10, 768)
    out = _emu_pairify(y, 5, f4=False)
    out["xh"][:10, 4:8], out["xh"][:10, 8:12] = out["xh"][:10, 8:12].clone(), out["xh"][:10, 4:8].clone()
    R.check_pairify(out, y, 5, "m")


def _mut_lane_swap_e2m1():
    y, g, b = _ln_inputs(65, 768)
    out = _emu_layernorm(y, g, b, 1e-12, 1, 65)
    out["x4"][:65, 2:4], out["x4"][:65, 4:6] = out["x4"][:65, 4:6].clone(), out["x4"][:65, 2:4].clone()
    R.check_layernorm(out, y, g, b, 1e-12, 65, "m", 1, 65)


def _mut_mean_512_of_768():
    y, g, b = _ln_inputs(5, 768)
    R.check_layernorm(_emu_layernorm(y, g, b, 1e-12, keys=("x32", "xh"), mean_cols=512), y, g, b, 1e-12, 5, "m")


def _mut_scale_groups_4_of_16():
    y, g, b = _ln_inputs(1025, 768)
    out = _emu_layernorm(y, g, b, 1e-12, 1, 1025, keys=("x32", "xh", "x4"))
    right, wrong = f4_scale_index(3, 1, 0, 700, 16), f4_scale_index(3, 1, 0, 700, 4)
    assert right != wrong
    out["x4s"][wrong], out["x4s"][right] = out["x4s"][right].clone(), R.SENT
    R.check_layernorm(out, y, g, b, 1e-12, 1025, "m", 1, 1025)


def _mut_saturating_scale():
    y, g, b = _ln_inputs(65, 768)
    R.check_layernorm(_emu_layernorm(y, g, b, 1e-12, 1, 65, rule="sat"), y, g, b, 1e-12, 65, "m", 1, 65)


def _mut_class_row_e2m1():
    y, g, b = _ln_inputs(65, 768)
    R.check_layernorm(_emu_layernorm(y, g, b, 1e-12, 1, 65, class_rows=True), y, g, b, 1e-12, 65, "m", 1, 65)


def _mut_twin_is_xu():
    y, g, b = _ln_inputs(10, 768)
    R.check_pair(_emu_pair(y, g, b, 1e-12, 5, f4=False, twin_of=lambda xc, xu: R.h16_of(xu)), y, g, b, 1e-12, 5, "m")


def _mut_twin_token_row_nonzero():
    c = _embed_case()
    two = _emu_embed_two_kernels(c)
    out = {k: v.clone() for k, v in two.items()}
    P = 2 * 65
    out["xh"][P + 7] = R.h16_of(out["x32"][P + 7])                 # an image-token twin row holding fp16(x_u) instead of the zero difference
    R.check_embed_pair(out, two, c, "m")


def _mut_mask_token_as_zero():
    c = _embed_case()
    R.check_embed(_emu_embed(c, None, mask_as_zero=True), c, None, "m")


def _mut_bits_msb_first():
    c = _embed_case()
    R.check_embed(_emu_embed(c, None, msb_first=True), c, None, "m")


def _mut_drop_ignored():
    c = _embed_case()
    R.check_embed(_emu_embed(c, None), c, torch.tensor([1, 0], dtype=torch.uint8), "m")


def _mut_row_past_M_written():
    y, g, b = _ln_inputs(5, 128)
    out = _emu_layernorm(y, g, b, 1e-12, keys=("x32", "xh"))
    out["xh"][5] = out["xh"][4]
    R.check_layernorm(out, y, g, b, 1e-12, 5, "m")


def _mut_rstd_eps_1e5():
    y, g, b = _ln_inputs(5, 1024)
    R.check_layernorm(_emu_layernorm(y, g, b, 1e-5, keys=("x32", "xh")), y, g, b, 1e-12, 5, "m")


MUTATIONS = {
    "lanes_swapped": (_mut_lane_swap, "ln_affine"),
    "lanes_swapped_pairify": (_mut_lane_swap_pairify, "conditional rows"),
    "lanes_swapped_e2m1": (_mut_lane_swap_e2m1, "e2m1 bytes"),
    "mean_over_512_of_768": (_mut_mean_512_of_768, "mean row"),
    "scale_index_groups_4_of_16": (_mut_scale_groups_4_of_16, "scale bytes"),
    "saturating_scale_rule": (_mut_saturating_scale, "e2m1 bytes"),
    "class_row_e2m1": (_mut_class_row_e2m1, "class-token rows"),
    "twin_is_fp16_xu": (_mut_twin_is_xu, "twin rows"),
    "embed_pair_twin_token_row_nonzero": (_mut_twin_token_row_nonzero, "xh against embed_ln"),
    "mask_token_as_index_0": (_mut_mask_token_as_zero, "x row 2,"),
    "bits_msb_first": (_mut_bits_msb_first, "x row"),
    "drop_ignored": (_mut_drop_ignored, "x row 64,"),
    "row_past_M_written": (_mut_row_past_M_written, "rows past 5 of xh"),
    "rstd_eps_1e-5": (_mut_rstd_eps_1e5, "rstd row"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_checkers_reject_the_mutated_kernel(name):
    fn, where = MUTATIONS[name]
    with pytest.raises(R.RowsMismatch) as e:
        fn()
    assert where in str(e.value), str(e.value)


def test_embed_pair_structure_check_stands_alone():
    """The twin-row rule of check_embed_pair does not lean on the two-kernel outputs: a path that wrote the same wrong twin row in BOTH is caught too."""
    c = _embed_case()
    two = _emu_embed_two_kernels(c)
    two["xh"][2 * 65 + 7] = R.h16_of(two["x32"][2 * 65 + 7])
    with pytest.raises(R.RowsMismatch, match="image-token rows"):
        R.check_embed_pair({k: v.clone() for k, v in two.items()}, two, c, "m")
