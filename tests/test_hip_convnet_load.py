"""GPU checks of the feature networks' checkpoint loaders (mb_inception_load, mb_resnet_load) called directly on the product models' handles: what
they refuse, with which code and message, that a refused entry leaves the handle as it was, and that a handle runs only once every entry it
needs is there.  Codes (include/maskbit_hip.h): -2 an entry the handle has no slot for, -4 an entry of the wrong shape or size, 0 for the
``num_batches_tracked`` counters, which are accepted and ignored.  Nothing larger than one image or one pair is run."""
import ctypes as C

import pytest
import torch

import inception_reference as RI
import resnet_reference as RR
from maskbit_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
ANY = (4,)

# (entry, the shape handed over -- None: one element short of its size in the state dict --, the code)
INCEPTION_REFUSALS = [
    ("Mixed_5b.branch1x1.conv.weight", (64, 191, 1, 1), -4),
    ("Mixed_5b.branch1x1.conv.weight", (64, 192, 1), -4),
    ("Mixed_5b.branch1x1.conv.weight", (192, 64, 1, 1), -4),
    ("Mixed_6b.branch7x7_2.conv.weight", (128, 128, 7, 1), -4),          # a 1x7: the element count is right, only the shape check can tell
    ("Mixed_7c.branch_pool.bn.running_var", None, -4),
    ("fc.weight", None, -4),
    ("AuxLogits.conv0.conv.weight", ANY, -2),
    ("Conv2d_1a_3x3.bn.num_batches_tracked", ANY, 0),
]
RESNET_REFUSALS = [
    ("conv1.weight", (64, 147, 1, 1), -4),                                # the folded stem's run shape: the checkpoint's is [64, 3, 7, 7]
    ("model.conv1.weight", (64, 147, 1, 1), -4),
    ("layer1.0.downsample.1.running_var", None, -4),
    ("mean", (4,), -4),
    ("fc.bias", (999,), -4),
    ("layer1.1.downsample.0.weight", ANY, -2),                            # only block 0 of a layer has a downsample branch
    ("model.mean", ANY, -2),
    ("bn1.num_batches_tracked", ANY, 0),
    ("model.layer4.2.bn3.num_batches_tracked", ANY, 0),
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def inception():
    from maskbit_amd import InceptionV3
    m = InceptionV3()
    m.load_weights(RI.weights("he"))
    m.max_images_per_call = 1
    u8 = torch.randint(0, 256, (2, 3, 8, 8), generator=torch.Generator().manual_seed(61), dtype=torch.uint8).to(DEV)

    def run():
        out = m(u8)
        torch.cuda.synchronize()
        return [v.clone() for v in out.values()], m.saturation_count()

    def forward(h):
        pool = torch.zeros(1, 2048, device=DEV)
        return _lib.load().mb_inception_forward(h, u8.data_ptr(), 1, 8, 8, pool.data_ptr(), None, None, _stream())

    return m.to(DEV), run, forward, lambda name: RI.weights("he")[name].numel()


def resnet():
    from maskbit_amd import PerceptualLoss
    m = PerceptualLoss()
    m.load_resnet50(RR.weights())
    m.max_pairs_per_call = 1
    g = torch.Generator().manual_seed(62)
    a, b = torch.rand(1, 3, 32, 32, generator=g).to(DEV), torch.rand(1, 3, 32, 32, generator=g).to(DEV)

    def run():
        out = []
        for on_logits in (True, False):
            m.compute_perceptual_loss_on_logits = on_logits
            out.append(m.per_image(a, b).clone())
        torch.cuda.synchronize()
        return out, m.saturation_count()

    def forward(h):
        out = torch.zeros(1, dtype=torch.float64, device=DEV)
        return _lib.load().mb_resnet_forward(h, a.data_ptr(), b.data_ptr(), 1, 32, 32, 0, 1, out.data_ptr(), None, _stream())

    def numel(name):
        sd = RR.reference_layout(RR.weights())
        return sd[name if name in sd else "model." + name].numel()

    return m.to(DEV), run, forward, numel


NETS = {"inception": (inception, "mb_inception", INCEPTION_REFUSALS,
                      ["Mixed_6b.branch7x7_2.conv.weight", "Mixed_7c.branch_pool.bn.running_var", "fc.bias"]),
        "resnet": (resnet, "mb_resnet", RESNET_REFUSALS,
                   ["model.layer3.0.downsample.0.weight", "model.layer2.1.bn2.running_mean", "model.fc.weight", "std"])}


@pytest.mark.parametrize("which", list(NETS))
def test_loader_refusals_leave_the_handle_intact(which):
    make, abi, refusals, _ = NETS[which]
    m, run, _forward, numel = make()
    before = run()
    h = m._engine
    assert h is not None and m._engine_key[1] == 1
    lib = _lib.load()
    entry = abi + "_load"
    load = getattr(lib, entry)
    data = torch.zeros(1 << 22, device=DEV)                # more floats than any shape below names: a loader that took one would stay inside it
    for name, shape, code in refusals:
        if shape is None:
            shape = (numel(name) - 1,)
        n = 1
        for v in shape:
            n *= v
        assert n <= data.numel()
        rc = load(h, name.encode(), data.data_ptr(), (C.c_int64 * len(shape))(*shape), len(shape), _stream())
        msg = lib.mb_last_error().decode()
        assert rc == code, (name, shape, rc, msg)
        if code:
            assert entry in msg and name in msg, (name, rc, msg)
        if code == -2:
            assert "unknown checkpoint entry" in msg, (name, msg)
    after = run()
    assert m._engine is h                                  # the same handle, not a reloaded one
    assert len(after[0]) == len(before[0]) and all(torch.equal(x, y) for x, y in zip(after[0], before[0])) and after[1] == before[1]
    assert all(bool(torch.isfinite(x).all()) for x in after[0])


@pytest.mark.parametrize("which,omit", [(which, omit) for which, v in NETS.items() for omit in v[3]])
def test_a_handle_runs_only_when_every_entry_is_loaded(which, omit):
    make, abi, _, _ = NETS[which]
    m, _run, forward, _numel = make()
    sd = {k: t for k, t in m.state_dict().items() if t.is_floating_point()}
    assert omit in sd and all(t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cuda" for t in sd.values())
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(getattr(lib, abi + "_create")(1, C.byref(h)), abi + "_create")

    def load(k):
        t = sd[k]
        _lib.check(getattr(lib, abi + "_load")(h, k.encode(), t.data_ptr(), (C.c_int64 * t.dim())(*t.shape), t.dim(), _stream()), f"{abi}_load({k})")

    try:
        for k in sd:
            if k != omit:
                load(k)
        assert forward(h) != 0
        assert "not complete" in lib.mb_last_error().decode()
        load(omit)
        assert forward(h) == 0
    finally:
        torch.cuda.synchronize()
        getattr(lib, abi + "_destroy")(h)
        torch.cuda.synchronize()
