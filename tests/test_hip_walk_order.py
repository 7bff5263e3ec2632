"""Walk order (mb_kernels.h walk_tile / walk_seq / walk_row): direction 1 visits the same tiles, workgroups and rows as direction 0 in the opposite
order, so every output is bit-identical -- per launch through mb_diag_set_walk (the direction the diagnostic entries hand to their kernel), and for a
whole guided forward through mb_gen_set_walk (0 = every launch in direction 0, 1 = alternating along the launch chain: the product's default)."""
import ctypes as C
from dataclasses import replace

import pytest
import torch

import gemm_reference as R
from hip_helpers import attention_pair, gemm_mini
from oracle import maskbit_oracle as O
from test_hip_rows import run_layernorm, run_layernorm_f4, run_pair, run_pairify

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEQS, SQ = 3, 257


def _lib():
    from maskbit_amd import _lib as L
    return L.load()


def _both_directions(lib, run):
    """-> [run() in direction 0, run() in direction 1]; the direction is restored whatever happens."""
    out = []
    try:
        for rev in (0, 1):
            assert lib.mb_diag_set_walk(rev) == 0
            out.append(run())
            torch.cuda.synchronize()
    finally:
        lib.mb_diag_set_walk(0)
    return out


def _same(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        same = torch.equal(x.view(torch.uint8), y.view(torch.uint8)) if x.dtype != torch.uint8 else torch.equal(x, y)
        assert same, f"{label}: output {k} differs between direction 0 and direction 1"


def test_setter_refuses_other_values():
    lib = _lib()
    assert lib.mb_diag_set_walk(2) == -1 and lib.mb_diag_set_walk(-1) == -1 and lib.mb_diag_set_walk(0) == 0


@pytest.mark.parametrize("nlo", [0, 1])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("pair", [True, False])
def test_sequence_gemm_tiles_all_epilogues(pair, K, N, nlo):
    """Pair tiles and plain sequence tiles, 3 x 257 rows, with and without the mini-tile operand set; fp16, GELU (+ the e2m1 copy with mini-tiles) and the
    fp32 residual in place over LayerNorm statistics; the device's own grid (one tile per workgroup at these sizes) and a grid of 2 workgroups (several
    tiles each: the has_next prologue runs in both directions)."""
    from maskbit_amd import _lib as L
    lib = _lib()
    rows = SEQS * SQ
    base = R.make_case(0, rows, N, K, seq_rows=SQ, pair=pair, nlo=nlo, seed=K + N + nlo, dev=DEV)
    lo = [s.tensors() for s in base.lo]
    torch.manual_seed(N + K)
    y = torch.randn(base.M, N, device=DEV) * 1.7 + 0.3
    g, b = torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV) * 0.2
    stats = torch.empty(base.M, 2, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.mb_layernorm(y.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-12, None, None, None, stats.data_ptr(), base.M, N, st), "mb_layernorm")
    flat = [t.data_ptr() for s in lo for t in s]
    arr = (C.c_void_p * max(1, len(flat)))(*flat)

    def launch(epi):
        c = replace(base, epi=epi)
        if epi == 2:
            out = y.clone()
            L.check(lib.mb_gemm_mini_ln(c.A.data_ptr(), c.W.data_ptr(), c.bias.data_ptr(), out.data_ptr(), stats.data_ptr(), g.data_ptr(), b.data_ptr(),
                                        rows, int(pair), SQ, N, K, nlo, arr, st), "mb_gemm_mini_ln")
            return {"out": out}
        o = {"out": torch.full((c.M, N), float("nan"), device=DEV, dtype=torch.float16)}
        if epi == 1 and nlo:
            o["out4"] = torch.full((c.M, 2 * N), 0xA5, device=DEV, dtype=torch.uint8)
            o["out4s"] = torch.full(((N // 64) * SEQS * (SQ - 1) + 256,), 0xA5, device=DEV, dtype=torch.uint8)
        gemm_mini(lib, epi, c.A, c.W, c.bias, None, None, o["out"], rows, pair, N, K, lo, o.get("out4"), o.get("out4s"), SQ)
        return o

    tiles = SEQS * (2 if pair else 1) * (N // 256)
    try:
        for cus in (0, 2):
            assert lib.mb_set_cu_count(cus) == 0
            for epi in (0, 1, 2):
                fwd, rev = _both_directions(lib, lambda: launch(epi))
                assert not bool(torch.isnan(fwd["out"]).any())
                _same(fwd, rev, f"{'pair' if pair else 'plain'} K {K} N {N} nlo {nlo} epi {epi}, {tiles} tiles on {cus or 'all'} CUs")
    finally:
        lib.mb_set_cu_count(0)


def test_attention_pair_with_e2m1_copies():
    lib = _lib()
    pairs, heads, d = SEQS, 2, 128
    torch.manual_seed(5)
    qc = torch.randn(pairs * SQ, 3 * d, device=DEV) * 0.7
    qkv = torch.cat([qc, qc + torch.randn_like(qc) * 0.02]).half().contiguous()

    def launch(f4):
        o = {"out": torch.full((2 * pairs * SQ, d), float("nan"), device=DEV, dtype=torch.float16)}
        if f4:
            for k in ("out4", "out4l"):
                o[k] = torch.zeros(2 * pairs * SQ, 2 * d, device=DEV, dtype=torch.uint8)
                o[k + "s"] = torch.zeros(heads * pairs * 256 + 256, device=DEV, dtype=torch.uint8)
        attention_pair(lib, qkv, o["out"], pairs, SQ, d, heads, o.get("out4"), o.get("out4s"), o.get("out4l"), o.get("out4ls"))
        return o

    for f4 in (True, False):
        fwd, rev = _both_directions(lib, lambda: launch(f4))
        assert not bool(torch.isnan(fwd["out"]).any())
        _same(fwd, rev, f"attention_pair, e2m1 copies {f4}")


@pytest.mark.parametrize("d", [1024, 768])
def test_row_kernels(d):
    """layernorm_pair, pairify and layernorm_rows over P = 3 x 257 rows (a row count that is no multiple of the 4 rows of a workgroup): with the sequence
    length known (the e2m1 entries: sequences follow walk_seq) and without it (mb_layernorm: one run of rows, mirrored)."""
    lib = _lib()
    P = SEQS * SQ
    torch.manual_seed(d)
    y = torch.randn(2 * P, d, device=DEV) * 1.3 + 0.1
    g, b = torch.rand(d, device=DEV) + 0.5, torch.randn(d, device=DEV) * 0.2
    runs = {
        "layernorm_pair": lambda: run_pair(y, g, b, P, d, SQ, ("xh", "stats", "x4", "xl4")),
        "layernorm_pair, no e2m1": lambda: run_pair(y, g, b, P, d, 0, ("xh", "stats")),
        "pairify": lambda: run_pairify(y, P, d, SQ, ("xh", "x4", "xl4")),
        "layernorm_rows": lambda: run_layernorm(y, g, b, P, d, ("x32", "xh", "xlo", "stats")),
        "layernorm_rows, e2m1": lambda: run_layernorm_f4(y, g, b, P, d, SQ, ("x32", "xh", "x4", "xl4")),
    }
    for label, run in runs.items():
        fwd, rev = _both_directions(lib, run)
        _same(fwd, rev, f"{label} d {d}")


@pytest.mark.parametrize("hidden,heads,mlp,prenorm", [(256, 4, 512, False), (256, 4, 512, True), (768, 12, 1024, False), (768, 12, 1024, True)])
def test_guided_forward_walk_modes(hidden, heads, mlp, prenorm):
    """A depth-2 generator, 2 pairs, strict mode (the product's default precision): the logits of walk mode 0 and walk mode 1 are the same bits.  Hidden 256
    takes the plain forward over [conditional | twins]; hidden 768 the differential pair forward with the weight-correction mini-tiles."""
    from maskbit_amd import LFQBert, _lib as L
    lib = _lib()
    cfg = O.GenCfg(bits=12, splits=2, hidden=hidden, depth=2, heads=heads, mlp=mlp, prenorm=prenorm)
    sd = O.make_generator_weights(cfg, seed=41, head_gain=12.0)
    m = LFQBert(img_size=256, hidden_dim=hidden, codebook_size=2 ** cfg.bits, codebook_splits=cfg.splits, depth=cfg.depth, heads=heads, mlp_dim=mlp,
                dropout=0.1, nclass=cfg.nclass, input_stride=16, use_prenorm=prenorm)
    m.load_state_dict(sd, strict=True)
    m = m.eval().requires_grad_(False).to(DEV)
    g = torch.Generator().manual_seed(hidden)
    t = torch.randint(0, 65, (2, 256, 2), generator=g).to(DEV)
    y = torch.tensor([5, 321], device=DEV)
    out = {}
    try:
        for mode in (1, 0, 1):
            L.check(lib.mb_gen_set_walk(m.engine(4), mode), "mb_gen_set_walk")
            lg = m.forward_cfg(t, y).clone()
            assert bool(torch.isfinite(lg).all())
            out.setdefault(mode, lg)
            assert torch.equal(out[mode], lg)
        assert torch.equal(out[0], out[1]), f"logits differ between the walk modes in {int((out[0] != out[1]).sum())} places"
        assert lib.mb_gen_set_walk(m.engine(4), 2) == -1
    finally:
        lib.mb_gen_set_walk(m.engine(4), 1)
