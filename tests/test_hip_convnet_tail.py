"""The fp32 tail of the Conv+BatchNorm feature networks (maskbit_amd/csrc/inception.hip; mb_inception and mb_resnet both run it), one launch at a
time through the diagnostic entries of include/maskbit_hip_diag.h: ``bn_fold_kernel`` (the loaders' BatchNorm fold), ``spatial_mean_kernel``,
``fc_head_kernel`` and ``channel_tap_kernel``; and the fold as the two product handles hold it, for every BatchNorm, under any load order and
after a reload.  The whole-network tests allow these kernels the error of an fp16 model (3e-4 .. 1.4e-3); here the unit is 2^-24.

Criteria, none tuned to what the kernels give (references and cases: tests/convnet_reference.py, checked on the CPU in test_convnet_tail_cpu.py):

* fold: bit-equal to the five correctly rounded fp32 operations (``bn_fold32``).
* spatial mean: bit-equal to the kernel's stated order in numpy float32 (``spatial_mean32``); integer inputs bit-equal to fp32(S) / fp32(HW);
  independently within (ceil(HW / 256) + 9) 2^-24 mean|x| of float64 -- a thread's chain, eight tree levels, the division.
* head: integer operands bit-equal to exact arithmetic; seeded within (D / 64 + 7) 2^-24 (sum |p w| + |bias|) of float64 -- a lane's fma
  chain, six butterfly levels, the bias add; biased == fp32(unbiased + bias) bit for bit; a row's bits do not depend on its batch.
* channel tap: the widened fp16 values, bit-equal.
* every output buffer keeps a NaN sentinel outside what the kernel is to write.

Worst error / bound of the seeded cases measured on an MI355X: spatial mean 0.26 (HW 255), head 0.09 (D 256, N 1008, B 9); the networks' own
logits against the head of their own pool 0.011 (profiles/inception.md, profiles/perceptual.md).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import convnet_reference as CR
import inception_reference as RI
import resnet_reference as RR
from convnet_helpers import (DEV, _lib, _stream, bits32, folded_bns, run_bn_fold, run_channel_tap, run_fc_head, run_spatial_mean)
from maskbit_amd.synth import inception_convs, resnet50_convs

pytestmark = pytest.mark.gpu
EPS = {"inception": float(np.float32(CR.INCEPTION_EPS)), "resnet": float(np.float32(CR.RESNET_EPS))}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits32(a), bits32(b))


# ------------------------------------------------------------------------------------------------ the fold, per launch
@pytest.mark.parametrize("net", list(EPS))
@pytest.mark.parametrize("cout", CR.FOLD_COUTS)
def test_fold_is_the_five_rounded_operations(cout, net):
    bn = CR.fold_case(cout)
    scale, shift, untouched = run_bn_fold(bn, EPS[net])
    want_scale, want_shift = CR.bn_fold32(*bn, EPS[net])
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all())
    off = int((bits32(scale) != bits32(want_scale)).sum()), int((bits32(shift) != bits32(want_shift)).sum())
    print(f"fold cout {cout} eps {EPS[net]:g}: {off[0]} scales and {off[1]} shifts of {cout} differ from the rounded expression")
    assert same_bits(scale, want_scale) and same_bits(shift, want_shift)
    assert untouched


def test_fold_refuses_what_it_does_not_take():
    L, lib = _lib()
    bn, sc, sh = torch.ones(4, 8, device=DEV), torch.full((8,), float("nan"), device=DEV), torch.full((8,), float("nan"), device=DEV)
    call = lambda b, s, t, cout, eps: lib.mb_bn_fold(b, s, t, cout, eps, _stream())
    p, q, r = bn.data_ptr(), sc.data_ptr(), sh.data_ptr()
    assert call(None, q, r, 8, 1e-3) == -1 and call(p, None, r, 8, 1e-3) == -1 and call(p, q, None, 8, 1e-3) == -1
    assert call(p, q, r, 0, 1e-3) == -1 and call(p, q, r, 8, -1e-3) == -1 and call(p, q, r, 8, float("nan")) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(sc).all()) and bool(torch.isnan(sh).all())          # nothing was launched
    assert call(p, q, r, 8, 0.0) == 0
    torch.cuda.synchronize()
    assert bool((sc == 1).all()) and bool((sh == 0).all())


# ------------------------------------------------------------------------------------------------ every BatchNorm of the two products
def _inception(style):
    from maskbit_amd import InceptionV3
    m = InceptionV3(["2048", "logits_unbiased", "logits"])
    m.load_weights(RI.weights(style))
    m.max_images_per_call = 1
    return m.to(DEV)


def _resnet():
    from maskbit_amd import PerceptualLoss
    m = PerceptualLoss()
    m.load_resnet50(RR.weights())
    m.max_pairs_per_call = 1
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _probe_inputs():
    g = torch.Generator().manual_seed(6400)
    u8 = torch.randint(0, 256, (1, 3, 8, 8), generator=g, dtype=torch.uint8).to(DEV)
    img = torch.zeros(1, 32, 32, 4, dtype=torch.float16)
    img[..., :3] = torch.randn(1, 32, 32, 3, generator=g).to(torch.float16)
    a = torch.rand(1, 3, 32, 32, generator=g)
    return u8, img.to(DEV), a.to(DEV), (a + 0.1 * torch.rand(1, 3, 32, 32, generator=g)).clamp(0, 1).to(DEV)


def _inception_probe(h):
    """one forward of the raw handle -> its fp32 outputs on the CPU"""
    L, lib = _lib()
    u8 = _probe_inputs()[0]
    outs = [torch.full((1, n), float("nan"), device=DEV) for n in (2048, 1008, 1008)]
    L.check(lib.mb_inception_forward(h, u8.data_ptr(), 1, 8, 8, *[t.data_ptr() for t in outs], _stream()), "mb_inception_forward")
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


def _resnet_probe(h):
    L, lib = _lib()
    img = _probe_inputs()[1]
    outs = [torch.full((1, n), float("nan"), device=DEV) for n in (2048, 1000)]
    L.check(lib.mb_resnet_taps(h, img.data_ptr(), 1, 32, None, None, None, None, *[t.data_ptr() for t in outs], _stream()), "mb_resnet_taps")
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


# name -> (abi, fresh product model, [(BatchNorm prefix as the model names it, cout)], the source weights by that prefix, eps, probe, the layer
# whose running_var the reload test changes, the product's own forward)
def _net(name):
    if name.startswith("inception"):
        style = name.split()[1]
        sd = RI.weights(style)
        layers = [(n + ".bn", cout) for n, _cin, cout, *_ in inception_convs()]
        forward = lambda m: [v.cpu() for v in m(_probe_inputs()[0]).values()]
        return "inception", (lambda: _inception(style)), layers, (lambda p: CR.bn_parts(sd, p)), EPS["inception"], _inception_probe, "Mixed_6b.branch7x7_2.bn", forward
    sd = RR.weights()
    layers = [("model." + bn, cout) for _conv, bn, _cin, cout, *_ in resnet50_convs()]
    forward = lambda m: [m.per_image(*_probe_inputs()[2:]).cpu()]
    return "resnet", _resnet, layers, (lambda p: CR.bn_parts(sd, p[len("model."):])), EPS["resnet"], _resnet_probe, "model.layer2.1.bn2", forward


NETS = ("inception he", "inception tf", "resnet")


def _want(layers, parts, eps):
    return {p: CR.bn_fold32(*parts(p), eps) for p, _c in layers}


def _assert_folds(tag, got, want):
    assert list(got) == list(want)
    for p in want:
        assert same_bits(got[p][0], want[p][0]) and same_bits(got[p][1], want[p][1]), (tag, p)


def test_the_layer_lists_are_the_networks():
    assert [len(_net(n)[2]) for n in NETS] == [94, 94, 53]


@pytest.mark.parametrize("name", NETS)
def test_every_folded_bn_is_the_fp32_expression(name):
    abi, make, layers, parts, eps, _probe, _layer, _forward = _net(name)
    L, lib = _lib()
    m = make()
    h = m.engine(1)
    want = _want(layers, parts, eps)
    _assert_folds(name, folded_bns(abi, h, layers), want)
    entry = getattr(lib, f"mb_{abi}_folded_bn")
    prefix, cout = layers[len(layers) // 2]
    buf = torch.full((2, cout + 1), float("nan"), device=DEV)
    call = lambda p, c: entry(h, p.encode(), buf[0].data_ptr(), buf[1].data_ptr(), c, _stream())
    if abi == "resnet":                                            # the loader takes torchvision's names too: so does this
        bare = [(p[len("model."):], c) for p, c in layers]
        got = folded_bns(abi, h, bare)
        _assert_folds(name, {"model." + p: v for p, v in got.items()}, want)
        assert call("model.model.bn1", 64) == -2
    for bad, code in (("no.such.bn", -2), ("fc", -2), (prefix + ".weight", -2), (prefix[:-1], -2)):
        assert call(bad, cout) == code, bad
        assert f"mb_{abi}_folded_bn" in lib.mb_last_error().decode() and bad in lib.mb_last_error().decode()
    assert call(prefix, cout + 1) == -4 and call(prefix, cout - 1) == -4
    assert entry(None, prefix.encode(), buf[0].data_ptr(), buf[1].data_ptr(), cout, _stream()) == -1
    assert entry(h, prefix.encode(), None, buf[1].data_ptr(), cout, _stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                            # a refused call copies nothing


@pytest.mark.parametrize("name", NETS)
def test_the_load_order_changes_no_bit(name):
    """load_entry refolds after each of a BatchNorm's four parts; whatever order they arrive in, among whatever other entries, the last fold sees
    all four.  Reversed: a layer's parts arrive variance first.  Shuffled: they arrive apart"""
    abi, make, layers, parts, eps, probe, _layer, _forward = _net(name)
    L, lib = _lib()
    m = make()
    want = _want(layers, parts, eps)
    reference = probe(m.engine(1))
    assert all(bool(torch.isfinite(t).all()) for t in reference)
    sd = {k: t for k, t in m.state_dict().items() if t.is_floating_point()}
    keys = list(sd)
    perm = torch.randperm(len(keys), generator=torch.Generator().manual_seed(6500)).tolist()
    shuffled = [keys[i] for i in perm]
    where = {k: i for i, k in enumerate(shuffled)}
    for p, _c in layers:                                           # no layer's four parts stayed together
        at = sorted(where[p + s] for s in (".weight", ".bias", ".running_mean", ".running_var"))
        assert at[3] - at[0] > 3, p
    for tag, order in (("reversed", keys[::-1]), ("shuffled", shuffled)):
        h = C.c_void_p()
        L.check(getattr(lib, f"mb_{abi}_create")(1, C.byref(h)), f"mb_{abi}_create")
        try:
            for k in order:
                t = sd[k]
                L.check(getattr(lib, f"mb_{abi}_load")(h, k.encode(), t.data_ptr(), (C.c_int64 * t.dim())(*t.shape), t.dim(), _stream()), f"mb_{abi}_load({k})")
            _assert_folds(f"{name} {tag}", folded_bns(abi, h, layers), want)
            got = probe(h)
            assert all(same_bits(a, b) for a, b in zip(got, reference)), tag
        finally:
            torch.cuda.synchronize()
            getattr(lib, f"mb_{abi}_destroy")(h)


@pytest.mark.parametrize("name", NETS)
def test_a_reload_refolds_the_changed_layer_and_no_other(name):
    """the model's own reload path: a parameter's version changes, the next forward loads every entry again onto the handle it has"""
    abi, make, layers, parts, eps, _probe, layer, forward = _net(name)
    m = make()
    before_out = forward(m)
    h = m._engine
    want = _want(layers, parts, eps)
    _assert_folds(name, folded_bns(abi, h, layers), want)
    var = m.get_buffer(layer + ".running_var")
    var.mul_(1.5)
    g, b, mean, _v = parts(layer)
    changed = CR.bn_fold32(g, b, mean, var.cpu(), eps)
    assert not torch.equal(changed[0], want[layer][0])
    after_out = forward(m)
    assert m._engine is h                                          # reloaded, not rebuilt
    want[layer] = changed
    _assert_folds(f"{name} reloaded", folded_bns(abi, h, layers), want)
    assert len(after_out) == len(before_out) and all(bool(torch.isfinite(t).all()) for t in after_out)
    assert all(not torch.equal(a, b) for a, b in zip(after_out, before_out))


# ------------------------------------------------------------------------------------------------ spatial mean
@pytest.mark.parametrize("HW", CR.MEAN_HW)
def test_spatial_mean_bits_and_bound(HW):
    worst = 0.0
    for C_ in CR.MEAN_C:
        for B in CR.MEAN_B:
            x16 = CR.mean_case("integer", B, HW, C_)
            got, untouched = run_spatial_mean(x16)
            want = torch.from_numpy(x16.double().sum(1).float().numpy() / np.float32(HW))
            assert same_bits(got, want) and untouched, ("integer", B, HW, C_)
            x16 = CR.mean_case("seeded", B, HW, C_)
            got, untouched = run_spatial_mean(x16)
            assert same_bits(got, CR.spatial_mean32(x16)) and untouched, ("seeded", B, HW, C_)
            exact, mag = CR.spatial_mean64(x16)
            err, bound = (got.double() - exact).abs(), CR.mean_bound(HW, mag)
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()) and bool((got[:, 1] < 0).all())
            for b in range(B):                                     # an image alone gives the bits it has in the batch
                one, _ = run_spatial_mean(x16[b:b + 1])
                assert same_bits(one, got[b:b + 1]), (b, B, HW, C_)
    print(f"spatial mean HW {HW}: worst err / bound {worst:.3f}")


def test_spatial_mean_refuses_what_it_does_not_take():
    L, lib = _lib()
    x = torch.zeros(2, 4, 16, dtype=torch.float16, device=DEV)
    out = torch.zeros(2, 16, device=DEV)
    call = lambda B, HW, C_, xp=x.data_ptr(), op=out.data_ptr(): lib.mb_spatial_mean(xp, op, B, HW, C_, _stream())
    assert call(2, 4, 16) == 0
    for bad in ((2, 4, 12), (2, 4, 4), (2, 4, 0), (2, 0, 16), (0, 4, 16), (-1, 4, 16)):
        assert call(*bad) == -1, bad
    assert call(2, 4, 16, xp=None) == -1 and call(2, 4, 16, op=None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("D,N,B", CR.HEAD_CASES)
def test_head_integer_operands_are_exact(D, N, B):
    pool, w, bias = CR.head_case("integer", B, D, N)
    exact_u, exact_b, _S = CR.fc_head64(pool, w, bias)
    unbiased, biased, untouched = run_fc_head(pool, w, bias)
    assert same_bits(unbiased, exact_u.float()) and same_bits(biased, exact_b.float()) and untouched


@pytest.mark.parametrize("D,N,B", CR.HEAD_CASES)
def test_head_vs_fp64_and_its_output_forms(D, N, B):
    pool, w, bias = CR.head_case("seeded", B, D, N)
    exact_u, exact_b, S = CR.fc_head64(pool, w, bias)
    unbiased, biased, untouched = run_fc_head(pool, w, bias)
    assert untouched and bool(torch.isfinite(unbiased).all()) and bool(torch.isfinite(biased).all())
    bound = CR.head_bound(D, S)
    eu, eb = (unbiased.double() - exact_u).abs(), (biased.double() - exact_b).abs()
    print(f"head D {D} N {N} B {B}: worst err / bound {max(float((eu / bound).max()), float((eb / bound).max())):.3f}")
    assert bool((eu <= bound).all()) and bool((eb <= bound).all())
    assert same_bits(biased, unbiased + bias)                      # one fp32 add of the bias
    # the same values whichever outputs are asked for
    only_u, none_b, ok1 = run_fc_head(pool, w, bias, biased=False)
    none_u, only_b, ok2 = run_fc_head(pool, w, bias, unbiased=False)
    assert none_b is None and none_u is None and ok1 and ok2
    assert same_bits(only_u, unbiased) and same_bits(only_b, biased)
    nb_u, nb_b, ok3 = run_fc_head(pool, w, None)                   # no bias: both outputs are the products' sum
    assert ok3 and same_bits(nb_u, unbiased) and same_bits(nb_b, unbiased)
    # a row's bits do not depend on the batch or its place in it: alone, and rotated by 3 rows, which moves rows across the 8-image groups
    for b in sorted({0, B // 2, B - 1}):
        one_u, one_b, _ = run_fc_head(pool[b:b + 1], w, bias)
        assert same_bits(one_u, unbiased[b:b + 1]) and same_bits(one_b, biased[b:b + 1]), b
    if B > 1:
        rolled = torch.roll(pool, 3, 0)
        r_u, r_b, _ = run_fc_head(rolled, w, bias)
        assert same_bits(r_u, torch.roll(unbiased, 3, 0)) and same_bits(r_b, torch.roll(biased, 3, 0))


def test_head_refuses_what_it_does_not_take():
    L, lib = _lib()
    pool, w, bias, out = torch.zeros(2, 2304, device=DEV), torch.zeros(4, 2304, device=DEV), torch.zeros(4, device=DEV), torch.full((2, 4), float("nan"), device=DEV)

    def call(B=2, D=256, N=4, p=pool.data_ptr(), wp=w.data_ptr(), u=out.data_ptr(), b=None):
        return lib.mb_fc_head(p, wp, bias.data_ptr(), u, b, B, D, N, _stream())

    for bad in (dict(D=2047), dict(D=2304), dict(D=0), dict(D=128), dict(D=257), dict(u=None, b=None), dict(B=0), dict(N=0), dict(p=None), dict(wp=None)):
        assert call(**bad) == -1, bad
        assert b"mb_fc_head" in lib.mb_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ channel tap
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 289])
@pytest.mark.parametrize("C_,off,cs", [(7, 0, 768), (8, 8, 24), (1, 23, 24)])
def test_channel_tap_is_the_slice_widened(C_, off, cs, HW, B):
    g = torch.Generator().manual_seed(6600 + cs + HW + B)
    buf = torch.full((B, HW, cs), float("nan"), dtype=torch.float16)
    buf[..., off:off + C_] = (torch.randn(B, HW, C_, generator=g) * 8).to(torch.float16)
    buf[0, 0, off] = 65504.0
    buf[B - 1, HW - 1, off + C_ - 1] = -65504.0
    got, untouched = run_channel_tap(buf, C_, off)
    assert bool(torch.isfinite(got).all()) and same_bits(got, buf[..., off:off + C_].float()) and untouched


def test_channel_tap_second_pass_of_the_grid_stride_loop():
    """16 384 blocks of 256 threads are the grid's cap: 5 elements more than that make the loop's second pass, at the far end of both buffers"""
    B, HW, C_, cs = 3, 199729, 7, 8
    assert 0 < B * HW * C_ - 16384 * 256 < 256
    g = torch.Generator().manual_seed(6700)
    buf = torch.randint(-2048, 2049, (B, HW, cs), generator=g).to(torch.float16)
    buf[..., C_:] = float("nan")
    got, untouched = run_channel_tap(buf, C_, 0)
    assert same_bits(got, buf[..., :C_].float()) and untouched


def test_channel_tap_refuses_what_it_does_not_take():
    L, lib = _lib()
    x = torch.zeros(2, 4, 24, dtype=torch.float16, device=DEV)
    out = torch.full((2, 4, 24), float("nan"), device=DEV)
    call = lambda B=2, HW=4, C_=8, off=8, cs=24, xp=x.data_ptr(), op=out.data_ptr(): lib.mb_channel_tap(xp, op, B, HW, C_, off, cs, _stream())
    for bad in (dict(off=17), dict(C_=25, off=0), dict(off=-1), dict(C_=0), dict(HW=0), dict(B=0), dict(xp=None), dict(op=None)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(off=16) == 0
    torch.cuda.synchronize()
