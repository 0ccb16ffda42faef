"""Colour augmentation on the device (nunet_color_aug_u8, nunet_preprocess_u8_color, nunet_plan_stage_u8_color,
TrainStep(color_aug=True)) against the numpy restatement of the project's definition in tests/color_cases.py.

Criteria. The kernels evaluate the definition's operations one by one in fp32, as the fp32 oracle does, so their bytes must
EQUAL the fp32 oracle's. Against the fp64 oracle an HSV byte may differ by one level (a product that lands next to a rounding
boundary of rint(x * 255)), and at most 0.5 % of the bytes of the HSV samples may differ at all: the fp32 restatement itself
differs from fp64 in 0.04 - 0.10 % of bytes on random colours, so a kernel above the cap evaluates something else (a
contracted multiply-add, a reciprocal). The cap is taken over all bytes of the HSV samples together. Per sample the fp32
restatement ITSELF (numpy on the CPU, tests/test_color_aug_cpu.py prints it) differs from fp64 in 0.96 % of the bytes of image 0
(b = 0 with a zero shift), 0.27 %, 0.06 % and 0.10 % of images 1 - 3, 0.35 % of the four together. The high figures belong to
s' = 255 with v' = 255 (image 0's saturated colours; the clamps of a (20, 30, 20) shift, 0.82 % on random colours): there
t * 255 = 8.5 * (h' mod 30) is an exact tie for every odd h' mod 30, and the last bits of fp32 and fp64 decide it differently.
Random colours stay at 0.02 - 0.10 % under the other three codes. Since the kernels' bytes equal the fp32 oracle's, their figure
is the definition's own. The fused loaders and the captured step are compared bit for bit with the unfused composition."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import dataset as D  # noqa: E402
import color_cases as CC  # noqa: E402

DEV = "cuda:0"
NUNET_EINVAL = -1


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


def dev(a):
    """a numpy array or host tensor -> a device tensor allocated through a guarded factory"""
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = torch.empty(a.shape, dtype=a.dtype, device=DEV)
    t.copy_(a)
    return t


def codes_dev(codes):
    return dev(D.color_codes([c[0] for c in codes], [c[1:] for c in codes]))


def color_aug_u8(u8, codes, inplace=False):
    """nunet_color_aug_u8 through ctypes (dataset.color_augment always allocates; this one can run in place)"""
    n, h, w, c = u8.shape
    out = u8 if inplace else torch.empty(u8.shape, dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_color_aug_u8(L.ptr(u8), n, h, w, c, L.ptr(codes), L.ptr(out), L.stream()), "nunet_color_aug_u8")
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def byte_case():
    """the 7 x 256 x 256 batch and its oracles for both code tables, computed once"""
    u = CC.byte_batch()
    ref = {}
    for name, codes in (("in_range", CC.BYTE_CODES), ("out_of_range", CC.OUT_OF_RANGE_CODES)):
        ref[name] = (CC.apply_batch(u, codes, np.float32), CC.apply_batch(u, codes, np.float64))
    return u, ref


# -- 1. bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["in_range", "out_of_range"])
def test_bytes_equal_the_fp32_oracle(byte_case, table):
    u, ref = byte_case
    codes = CC.BYTE_CODES if table == "in_range" else CC.OUT_OF_RANGE_CODES
    r32, r64 = ref[table]
    got = D.color_augment(dev(u), codes_dev(codes)).cpu().numpy()
    for i, code in enumerate(codes):
        bad = int((got[i] != r32[i]).sum())
        d64 = np.abs(got[i].astype(int) - r64[i].astype(int))
        print("sample %d code %s: bytes != fp32 oracle %d, != fp64 oracle %.4f %%, max |d64| %d" % (i, code, bad, 100.0 * (d64 != 0).mean(), d64.max()))
    for i, code in enumerate(codes):
        assert np.array_equal(got[i], r32[i]), "sample %d %s: %d bytes differ from the fp32 oracle" % (i, code, int((got[i] != r32[i]).sum()))
        d64 = np.abs(got[i].astype(int) - r64[i].astype(int))
        if code[0] == CC.HSV:
            assert d64.max() <= 1, "sample %d %s: %d levels from the fp64 oracle" % (i, code, d64.max())
        else:
            assert d64.max() == 0       # the LUT ops and NONE are one fp32 operation on an integer: the same in fp64 up to the fp32 parameter
    hsv = [i for i, code in enumerate(codes) if code[0] == CC.HSV]
    if hsv:
        frac = float((got[hsv] != r64[hsv]).mean())
        print("HSV samples %s: %.4f %% of bytes differ from the fp64 oracle" % (hsv, 100.0 * frac))
        assert frac <= 0.005, "%.3f %% of the HSV samples' bytes differ from the fp64 oracle" % (100.0 * frac)
    if table == "in_range":
        assert hsv == [0, 1, 2, 3]
        assert np.array_equal(got[6], u[6]) and not np.array_equal(got[0], u[0])


# -- 2. small and odd shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,inplace", CC.SMALL_SHAPES)
def test_small_and_odd_shapes(n, h, w, inplace):
    u = np.random.default_rng(n * 1000 + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    codes = CC.SMALL_CODES[:n]
    src = dev(u)
    got = color_aug_u8(src, codes_dev(codes), inplace)
    assert (got.data_ptr() == src.data_ptr()) == inplace
    assert np.array_equal(got.cpu().numpy(), CC.apply_batch(u, codes))
    if not inplace:
        assert np.array_equal(src.cpu().numpy(), u)


# -- 3. fused loaders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,aug", [(12, 12, [0, 1, 2 | 4, 3 | 8, 1 | 12]), (6, 10, [0, 2, 2 | 4, 8, 2 | 12])])
def test_preprocess_color_equals_color_then_preprocess(h, w, aug):
    n = len(aug)
    u = dev(np.random.default_rng(h).integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    a = dev(torch.tensor(aug, dtype=torch.int32))
    codes = [CC.BYTE_CODES[3], CC.BYTE_CODES[4], CC.BYTE_CODES[5], CC.BYTE_CODES[6], CC.BYTE_CODES[1]]
    col = codes_dev(codes)
    fused = D.preprocess_images(u, a, color=col)
    two = D.preprocess_images(D.color_augment(u, col), a)
    assert torch.equal(fused, two)
    assert not torch.equal(fused, D.preprocess_images(u, a)), "the colour ops did something"
    # against the oracle as well: the composition is the numpy colour op followed by the existing entry
    assert torch.equal(fused, D.preprocess_images(dev(CC.apply_batch(u.cpu().numpy(), codes)), a))
    # all NONE, and color == NULL, give the existing entry's output
    none = codes_dev([(CC.NONE, 1.0, 2.0, 3.0)] * n)
    plain = D.preprocess_images(u, a)
    assert torch.equal(D.preprocess_images(u, a, color=none), plain)
    assert torch.equal(D.preprocess_images(u, None, color=none), D.preprocess_images(u, None))
    m, s = dev(np.asarray(D.MEAN, np.float32)), dev(np.asarray(D.STD, np.float32))
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    L.check(L.lib().nunet_preprocess_u8_color(L.ptr(u), n, h, w, 3, L.ptr(m), L.ptr(s), L.ptr(a), None, 1.0 / 255.0, L.ptr(out), L.stream()), "null color")
    assert torch.equal(out, plain)


# -- 4. the captured step ------------------------------------------------------------------------------------------------------------
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor: its node count is the step's launch count


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_with_colour_codes(dtype, synth):
    """Three captured step_u8 calls with changing aug and colour codes equal three steps of a float TrainStep fed
    preprocess_images(color_augment(raw, color), aug): losses, parameters and BatchNorm buffers bit for bit. color_aug=True with
    color=None equals color_aug=False, and the graph has as many nodes either way."""
    from nunet_amd.trainer import TrainStep
    n, hw = 4, 32
    torch.manual_seed(9)
    sd = {k: v.clone() for k, v in nunet_amd.archs.NestedUNet(1, 3, False).state_dict().items()}
    raw, m8 = synth.synth_blob_pairs_u8(3 * n, hw, hw, seed=77)
    raw, m8 = dev(raw), dev(m8)
    gen = torch.Generator().manual_seed(2)
    augs = [None, torch.tensor([1, 2 | 4, 3 | 8, 12], dtype=torch.int32, device=DEV), D.draw_augmentation(n, gen, DEV)]
    cols = [codes_dev(CC.BYTE_CODES[:4]), D.draw_color_augmentation(n, gen, DEV), codes_dev(CC.BYTE_CODES[3:7])]

    def run(mode):
        m = nunet_amd.archs.NestedUNet(1, 3, False, dtype=dtype)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        u8 = mode != "float"
        ts = TrainStep(m, (n, 3, hw, hw), lr=1e-2, input_u8=u8, color_aug=mode in ("color", "color_none"), **GRAPH)
        if u8:
            ts.capture(raw[:n], m8[:n])
        else:
            ts.capture(D.preprocess_images(raw[:n]), D.preprocess_masks(m8[:n]))
        losses = []
        for k in range(3):
            xb, tb = raw[k * n:(k + 1) * n], m8[k * n:(k + 1) * n]
            ts.reset_meters()
            if mode == "color":
                ts.step_u8(xb, tb, augs[k], cols[k])
            elif mode == "float":
                ts.step(D.preprocess_images(D.color_augment(xb.contiguous(), cols[k]), augs[k]), D.preprocess_masks(tb, augs[k]))
            else:                                   # "color_none": built with the colour loader, no codes; "plain": today's step
                ts.step_u8(xb, tb, augs[k])
            losses.append(ts.epoch_stats())
        torch.cuda.synchronize()
        return losses, ts.eng.flat_params.clone(), ts.eng.bnbuf.clone(), ts.g_fb.info()["nodes"], ts

    col, flt, none, plain = run("color"), run("float"), run("color_none"), run("plain")
    print("losses", col[0], "graph nodes with / without the colour loader: %d / %d" % (col[3], plain[3]))
    assert col[0] == flt[0], (col[0], flt[0])
    assert torch.equal(col[1], flt[1]) and torch.equal(col[2], flt[2])
    assert none[0] == plain[0] and torch.equal(none[1], plain[1]) and torch.equal(none[2], plain[2])
    assert col[0] != plain[0], "the colour ops changed the batch"
    assert col[3] == plain[3] == none[3]
    # a step that had colour codes runs without them afterwards: the static buffer is cleared
    ts = col[4]
    ts.step_u8(raw[:n], m8[:n], None, cols[0])
    ts.step_u8(raw[:n], m8[:n])
    assert int(ts.color.abs().sum()) == 0


# -- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_before_launching():
    lib = L.lib()
    u = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    u1 = torch.zeros((2, 4, 4, 1), dtype=torch.uint8, device=DEV)
    col = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    out = torch.full((2, 4, 4, 3), 7, dtype=torch.uint8, device=DEV)
    fo = torch.full((2, 3, 4, 4), 7.0, dtype=torch.float32, device=DEV)
    m, s = dev(np.asarray(D.MEAN, np.float32)), dev(np.asarray(D.STD, np.float32))
    st = L.stream()

    def refused(rc, *words):
        assert rc == NUNET_EINVAL
        msg = lib.nunet_last_error().decode()
        assert msg and all(w in msg for w in words), msg

    refused(lib.nunet_color_aug_u8(L.ptr(u1), 2, 4, 4, 1, L.ptr(col), L.ptr(out), st), "color_aug_u8", "C=1")
    refused(lib.nunet_color_aug_u8(None, 2, 4, 4, 3, L.ptr(col), L.ptr(out), st), "color_aug_u8", "null")
    refused(lib.nunet_color_aug_u8(L.ptr(u), 2, 4, 4, 3, None, L.ptr(out), st), "color_aug_u8", "null")
    refused(lib.nunet_color_aug_u8(L.ptr(u), 2, 4, 4, 3, L.ptr(col), None, st), "color_aug_u8", "null")
    refused(lib.nunet_color_aug_u8(L.ptr(u), 0, 4, 4, 3, L.ptr(col), L.ptr(out), st), "color_aug_u8", "positive")
    refused(lib.nunet_color_aug_u8(L.ptr(u), 2, -4, 4, 3, L.ptr(col), L.ptr(out), st), "color_aug_u8", "positive")
    refused(lib.nunet_preprocess_u8_color(L.ptr(u1), 2, 4, 4, 1, L.ptr(m), L.ptr(s), None, L.ptr(col), 1.0, L.ptr(fo), st), "preprocess_u8_color", "C=1")
    refused(lib.nunet_preprocess_u8_color(L.ptr(u), 2, 4, 4, 3, None, None, None, L.ptr(col), 1.0, L.ptr(fo), st), "preprocess_u8_color", "mean")
    refused(lib.nunet_preprocess_u8_color(None, 2, 4, 4, 3, L.ptr(m), L.ptr(s), None, L.ptr(col), 1.0, L.ptr(fo), st), "preprocess_u8_color")
    refused(lib.nunet_preprocess_u8_color(L.ptr(u), 2, 4, 4, 3, L.ptr(m), L.ptr(s), None, L.ptr(col), 1.0, None, st), "preprocess_u8_color")
    # the plan entry: null pointers, and a one-channel plan
    cfg = L.PlanCfg(2, 32, 32, 1, 1, 0, L.F32, 0)
    p = lib.nunet_plan_create(C.byref(cfg))
    assert p
    try:
        arena = torch.zeros(lib.nunet_plan_arena_bytes(p), dtype=torch.uint8, device=DEV)
        x1 = torch.zeros((2, 32, 32, 1), dtype=torch.uint8, device=DEV)
        c2 = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
        refused(lib.nunet_plan_stage_u8_color(p, L.ptr(x1), L.ptr(m), L.ptr(s), None, L.ptr(c2), 1.0, L.ptr(arena), L.nbytes(arena), st),
                "plan_stage_u8_color", "input_channels=1")
        refused(lib.nunet_plan_stage_u8_color(p, None, L.ptr(m), L.ptr(s), None, L.ptr(c2), 1.0, L.ptr(arena), L.nbytes(arena), st),
                "plan_stage_u8_color", "null")
        refused(lib.nunet_plan_stage_u8_color(None, L.ptr(x1), L.ptr(m), L.ptr(s), None, L.ptr(c2), 1.0, L.ptr(arena), L.nbytes(arena), st),
                "plan_stage_u8_color", "null")
        torch.cuda.synchronize()
        assert int(arena.max()) == 0
    finally:
        lib.nunet_plan_destroy(p)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((fo == 7.0).all()), "a refused call launched nothing"


def test_python_misuse_raises():
    from nunet_amd.trainer import TrainStep
    n, hw = 2, 32
    m3 = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).train()
    with pytest.raises(L.NunetError, match="input_u8"):
        TrainStep(m3, (n, 3, hw, hw), color_aug=True)                       # without the uint8 loader
    m1 = nunet_amd.archs.NestedUNet(1, 1, False).to(DEV).train()
    with pytest.raises(L.NunetError, match="input_channels == 3"):
        TrainStep(m1, (n, 1, hw, hw), input_u8=True, color_aug=True)        # not RGB
    ts = TrainStep(m3, (n, 3, hw, hw), input_u8=True, use_graph=False)
    x, t = torch.zeros((n, hw, hw, 3), dtype=torch.uint8, device=DEV), torch.zeros((n, hw, hw, 1), dtype=torch.uint8, device=DEV)
    steps = ts.steps
    with pytest.raises(L.NunetError, match="color_aug=True"):
        ts.step_u8(x, t, None, D.draw_color_augmentation(n, torch.Generator().manual_seed(0), DEV))   # codes into a step built without
    assert ts.steps == steps
    tc = TrainStep(m3, (n, 3, hw, hw), input_u8=True, color_aug=True, use_graph=False)
    with pytest.raises(L.NunetError, match="int32"):
        tc.step_u8(x, t, None, torch.zeros((n, 3), dtype=torch.int32, device=DEV))                    # not [n,4]
    assert tc.steps == 0
    with pytest.raises(L.NunetError):
        D.color_augment(torch.zeros((n, 4, 4, 1), dtype=torch.uint8, device=DEV), torch.zeros((n, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(L.NunetError):
        D.preprocess_images(torch.zeros((n, 4, 4, 3), dtype=torch.uint8, device=DEV), color=torch.zeros((n, 3), dtype=torch.int32, device=DEV))
