"""The device-side input pipeline (nunet_preprocess_u8, nunet_preprocess_u8_color, nunet_color_aug_u8, nunet_plan_stage_u8,
nunet_plan_stage_u8_color, TrainStep.step_u8) against the numpy oracle of tests/pipeline_cases.py - never against one another.

Geometry is compared EXACTLY on tagged images whose bytes say where they came from (all 16 codes on square shapes, the 8
even-rot90 codes on the others; tests/test_input_pipeline_cpu.py shows these tables catch every plausible mutation of the
index map): in the NULL mean / std, post_scale = 1 configuration every output value is the fp32 quotient u/255 (rounded to
nearest-even into a 16-bit storage type), 256 distinct values that decode back to bytes, and a wrong pixel is reported as
the source (n, y, x) found and expected. Values are compared with the fp64 evaluation within the per-element bound
B = 2^-24 (|u/255| / std * post_scale + 3 |ref|) derived in pipeline_cases.py (a faithful fp32 evaluation reaches 0.90 B on
the CPU), and 16-bit staged values bit for bit with the fp32 restatement rounded to nearest-even. The staged image is read
through Plan.image() from an arena pre-filled with a non-zero pattern: padding channels must be zero bits and nothing
outside the image may change. The capped-grid cases push each one-pixel-per-thread kernel past 4096 x 256 pixels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import dataset as D  # noqa: E402
from nunet_amd.engine import Plan  # noqa: E402
import color_cases as CC  # noqa: E402
import pipeline_cases as PC  # noqa: E402

DEV = "cuda:0"
KINDS = {"fp32": L.F32, "bf16": L.BF16, "fp16": L.F16}
FILL = 0xA5
# two or three codes per colour op (color_cases.BYTE_CODES and its neighbours), cycled over the samples of a batch
COLOR_CODES = [CC.BYTE_CODES[1], CC.BYTE_CODES[4], CC.BYTE_CODES[5], CC.BYTE_CODES[2], CC.SMALL_CODES[2], CC.OUT_OF_RANGE_CODES[0],
               CC.BYTE_CODES[3]]
ZERO3, ONE3 = np.zeros(3, np.float32), np.ones(3, np.float32)


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


def dev(a):
    """a numpy array or host tensor -> a device tensor allocated through a guarded factory; None stays None (a NULL argument)"""
    if a is None:
        return None
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = torch.empty(a.shape, dtype=a.dtype, device=DEV)
    t.copy_(a)
    return t


def aug_dev(codes):
    return None if codes is None else dev(np.asarray(codes, np.int32))


def color_dev(codes):
    return dev(D.color_codes([c[0] for c in codes], [c[1:] for c in codes]))


def color_codes_for(n):
    return [COLOR_CODES[i % len(COLOR_CODES)] for i in range(n)]


def preprocess_u8(u, codes, mean, std, post_scale, color=None):
    """nunet_preprocess_u8 / _color through ctypes on a numpy uint8 [N,H,W,C] batch -> numpy fp32 [N,H,W,C] (the entry writes
    NCHW; the transpose is numpy's)"""
    n, h, w, c = u.shape
    out = torch.full((n, c, h, w), 7.0, dtype=torch.float32, device=DEV)
    ud, a, m, s = dev(u), aug_dev(codes), dev(None if mean is None else np.resize(np.asarray(mean, np.float32), c)), \
        dev(None if std is None else np.resize(np.asarray(std, np.float32), c))
    if color is None:
        L.check(L.lib().nunet_preprocess_u8(L.ptr(ud), n, h, w, c, L.ptr(m), L.ptr(s), L.ptr(a), post_scale, L.ptr(out), L.stream()), "nunet_preprocess_u8")
    else:
        col = color_dev(color)
        L.check(L.lib().nunet_preprocess_u8_color(L.ptr(ud), n, h, w, c, L.ptr(m), L.ptr(s), L.ptr(a), L.ptr(col), post_scale, L.ptr(out), L.stream()),
                "nunet_preprocess_u8_color")
    torch.cuda.synchronize()
    assert np.array_equal(ud.cpu().numpy(), u), "the source batch was written"
    return np.ascontiguousarray(out.cpu().numpy().transpose(0, 2, 3, 1))


def color_aug_u8(u, color):
    n, h, w, c = u.shape
    ud, col = dev(u), color_dev(color)
    out = torch.full(u.shape, 7, dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_color_aug_u8(L.ptr(ud), n, h, w, c, L.ptr(col), L.ptr(out), L.stream()), "nunet_color_aug_u8")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def make_plan(n, h, w, cin, kind, depth=None):
    return Plan(n, h, w, cin, 1, depth is not None, KINDS[kind], False, DEV, depth=depth)


def stage(pl, u, codes, mean, std, post_scale, color=None, check_rest=True):
    """nunet_plan_stage_u8(_color) into an arena filled with FILL bytes -> (fp32 numpy [N,H,W,32] of Plan.image(), its raw bits).
    check_rest: no byte of the arena outside the image changed."""
    lib, c = L.lib(), u.shape[-1]
    pl.arena.fill_(FILL)
    ud, a = dev(u), aug_dev(codes)
    m = dev(None if mean is None else np.resize(np.asarray(mean, np.float32), c))
    s = dev(None if std is None else np.resize(np.asarray(std, np.float32), c))
    if color is None:
        L.check(lib.nunet_plan_stage_u8(pl.handle, L.ptr(ud), L.ptr(m), L.ptr(s), L.ptr(a), post_scale, L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()),
                "nunet_plan_stage_u8")
    else:
        col = color_dev(color)
        L.check(lib.nunet_plan_stage_u8_color(pl.handle, L.ptr(ud), L.ptr(m), L.ptr(s), L.ptr(a), L.ptr(col), post_scale, L.ptr(pl.arena),
                                              L.nbytes(pl.arena), L.stream()), "nunet_plan_stage_u8_color")
    torch.cuda.synchronize()
    img = pl.image()
    assert tuple(img.shape) == (pl.n, pl.h, pl.w, 32) and img.dtype == L.TORCH_DTYPE[pl.dtype]
    host = img.cpu().contiguous()
    bits = host.view(torch.int32 if pl.dtype == L.F32 else torch.int16).numpy()
    if check_rest:
        off = lib.nunet_plan_image(pl.handle, None, None)
        size = pl.n * pl.h * pl.w * 32 * host.element_size()
        assert off >= 0 and off % 16 == 0 and off + size <= pl.arena_bytes
        assert bool((pl.arena[:off] == FILL).all()) and bool((pl.arena[off + size:] == FILL).all()), "the staging launch wrote outside the image"
    return host.float().numpy(), bits


def assert_bytes(got_values, kind, exp_bytes, what, decode=None):
    """the output, decoded to the bytes it is the exact quotient image of, equals the oracle's bytes"""
    got = PC.decode_bytes(got_values, kind)
    msg = PC.first_mismatch(got, exp_bytes, decode)
    assert not msg, "%s: %s" % (what, msg)


def assert_within_bound(got, ref, B, what):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / B).max())
    print("%s: max err %.3e, max err/B %.3f" % (what, err.max(), ratio))
    assert np.all(err <= B), "%s: %d elements past B, worst err/B %.3f" % (what, int((err > B).sum()), ratio)
    return ratio


# -- 1. preprocess_u8 geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PC.CHANNELS)
def test_preprocess_u8_geometry(c):
    for h, w in PC.U8_SHAPES:
        codes = PC.codes_for(h, w)
        u = PC.tagged(len(codes), h, w, c, codes)
        got = preprocess_u8(u, codes, None, None, 1.0)
        assert_bytes(got, "fp32", PC.ref_batch(u, codes), "%dx%d C=%d" % (h, w, c))
        for name, ident in (("aug NULL", None), ("aug all zero", [0] * len(codes))):
            assert_bytes(preprocess_u8(u, ident, None, None, 1.0), "fp32", u, "%dx%d C=%d %s" % (h, w, c, name))


# -- 2. preprocess_u8 values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 4])
def test_preprocess_u8_values(c):
    u = PC.all_bytes_image(c)
    ref, B = PC.ref_values(u, PC.MEAN, PC.STD, 1.0 / 255.0)
    got = preprocess_u8(u, None, PC.MEAN, PC.STD, 1.0 / 255.0)
    assert_within_bound(got, ref, B, "preprocess_u8 C=%d, ImageNet mean/std, post_scale 1/255" % c)
    print("bit-equal to the fp32 restatement: %s" % np.array_equal(got, PC.f32_values(u, PC.MEAN, PC.STD, 1.0 / 255.0)))
    # the entry the package calls gives the same numbers
    pk = D.preprocess_images(dev(u)).cpu().numpy().transpose(0, 2, 3, 1)
    assert_within_bound(pk, ref, B, "dataset.preprocess_images C=%d" % c)


def test_masks_come_out_as_zero_and_one():
    m8 = (np.random.default_rng(11).random((3, 7, 5, 2)) > 0.5).astype(np.uint8) * 255
    got = preprocess_u8(m8, [2, 8, 2 | 4], None, None, 1.0)
    assert np.array_equal(got, PC.ref_batch(m8 // 255, [2, 8, 2 | 4]).astype(np.float32))
    pk = D.preprocess_masks(dev(m8), aug_dev([2, 8, 2 | 4])).cpu().numpy().transpose(0, 2, 3, 1)
    assert np.array_equal(pk, got) and set(np.unique(pk)) == {0.0, 1.0}


# -- 3. preprocess_u8_color and color_aug_u8 -------------------------------------------------------------------------------------
def test_preprocess_u8_color_geometry_with_no_colour_op():
    for h, w in PC.U8_SHAPES:
        codes = PC.codes_for(h, w)
        u = PC.tagged(len(codes), h, w, 3, codes)
        none = [(CC.NONE, 1.0, 2.0, 3.0)] * len(codes)
        got = preprocess_u8(u, codes, ZERO3, ONE3, 1.0, color=none)
        assert_bytes(got, "fp32", PC.ref_batch(u, codes), "%dx%d colour NONE" % (h, w))
        assert np.array_equal(got, preprocess_u8(u, codes, None, None, 1.0)), "%dx%d: differs from nunet_preprocess_u8" % (h, w)


@pytest.mark.parametrize("h,w", [(1, 6), (7, 3), (5, 5), (16, 16), (33, 31)])
def test_preprocess_u8_color_against_the_colour_and_geometry_oracles(h, w):
    codes = PC.codes_for(h, w)
    n = len(codes)
    u = np.random.default_rng(100 * h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    col = color_codes_for(n)
    exp_bytes = PC.ref_batch(CC.apply_batch(u, col), codes)
    assert not np.array_equal(exp_bytes, PC.ref_batch(u, codes)), "the colour ops did something"
    # bytes, exactly: mean 0, std 1 (given, as the entry demands), post_scale 1
    assert_bytes(preprocess_u8(u, codes, ZERO3, ONE3, 1.0, color=col), "fp32", exp_bytes, "%dx%d colour bytes" % (h, w))
    # values: ImageNet mean / std, post_scale 1/255, within B of fp64
    ref, B = PC.ref_values(exp_bytes, PC.MEAN, PC.STD, 1.0 / 255.0)
    assert_within_bound(preprocess_u8(u, codes, PC.MEAN, PC.STD, 1.0 / 255.0, color=col), ref, B, "preprocess_u8_color %dx%d" % (h, w))
    # the stand-alone pass: sample n through color[n], no geometry
    assert np.array_equal(color_aug_u8(u, col), CC.apply_batch(u, col))


# -- 4. stage_u8 geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("c", PC.PLAN_CHANNELS)
def test_stage_u8_geometry(kind, c):
    for h, w in PC.PLAN_SHAPES:
        codes = PC.codes_for(h, w)
        u = PC.tagged(len(codes), h, w, c, codes)
        pl = make_plan(len(codes), h, w, c, kind)
        what = "%s %dx%d C=%d" % (kind, h, w, c)
        img, bits = stage(pl, u, codes, None, None, 1.0)
        assert_bytes(img[..., :c], kind, PC.ref_batch(u, codes), what)
        assert not bits[..., c:].any(), "%s: %d padding elements are not zero" % (what, int((bits[..., c:] != 0).sum()))
        img, bits = stage(pl, u, None, None, None, 1.0)
        assert_bytes(img[..., :c], kind, u, what + " aug NULL")
        assert not bits[..., c:].any()


# -- 5. stage_u8 values ----------------------------------------------------------------------------------------------------------
def storage_bits(f32, kind):
    return {"fp32": lambda f: f.view(np.int32), "bf16": lambda f: PC.round_bf16_bits(f).view(np.int16),
            "fp16": lambda f: PC.round_fp16_bits(f).view(np.int16)}[kind](np.ascontiguousarray(f32, np.float32))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage_u8_values(kind):
    u = PC.all_bytes_image(3)
    pl = make_plan(1, 16, 16, 3, kind)
    img, bits = stage(pl, u, None, PC.MEAN, PC.STD, 1.0 / 255.0)
    f32 = PC.f32_values(u, PC.MEAN, PC.STD, 1.0 / 255.0)
    if kind == "fp32":
        ref, B = PC.ref_values(u, PC.MEAN, PC.STD, 1.0 / 255.0)
        assert_within_bound(img[..., :3], ref, B, "stage_u8 fp32")
        print("bit-equal to the fp32 restatement: %s" % np.array_equal(bits[..., :3], storage_bits(f32, kind)))
    else:
        exp = storage_bits(f32, kind)
        assert np.array_equal(bits[..., :3], exp), "%s: %d of 768 staged values differ from round-to-nearest-even of the fp32 result" % (
            kind, int((bits[..., :3] != exp).sum()))
    assert not bits[..., 3:].any()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage_u8_color_values(kind):
    n, hw = 7, 16
    codes = [0, 1, 2 | 4, 3 | 8, 12, 3, 2]
    u = np.random.default_rng(21).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    col = color_codes_for(n)
    exp_bytes = PC.ref_batch(CC.apply_batch(u, col), codes)
    pl = make_plan(n, hw, hw, 3, kind)
    img, bits = stage(pl, u, codes, PC.MEAN, PC.STD, 1.0 / 255.0, color=col)
    f32 = PC.f32_values(exp_bytes, PC.MEAN, PC.STD, 1.0 / 255.0)
    if kind == "fp32":
        ref, B = PC.ref_values(exp_bytes, PC.MEAN, PC.STD, 1.0 / 255.0)
        assert_within_bound(img[..., :3], ref, B, "stage_u8_color fp32")
    else:
        exp = storage_bits(f32, kind)
        assert np.array_equal(bits[..., :3], exp), "%s: %d staged values differ" % (kind, int((bits[..., :3] != exp).sum()))
    assert not bits[..., 3:].any()
    # bytes exactly, through the quotient configuration
    img, bits = stage(pl, u, codes, ZERO3, ONE3, 1.0, color=col)
    assert_bytes(img[..., :3], kind, exp_bytes, "stage_u8_color %s bytes" % kind)


# -- 6. capped grids -------------------------------------------------------------------------------------------------------------
LARGE_COLOR = [CC.BYTE_CODES[3], CC.BYTE_CODES[6], CC.BYTE_CODES[4], CC.BYTE_CODES[6], CC.BYTE_CODES[5]]    # samples 1 and 3 NONE


@pytest.fixture(scope="module")
def large_free():
    n, h, w = PC.LARGE_SHAPES["free"]
    u = PC.tagged_large(n, h, w)
    return u, CC.apply_batch(u, LARGE_COLOR)


def test_capped_grid_color_aug_u8(large_free):
    """5 x 460 x 457 = 1,051,100 pixels against the 1,048,576 the grid holds: the last 2,524 pixels are a thread's second
    trip, and that trip ends inside a block (the count is no multiple of 256). The plan entries below cannot show a partial
    final block - their shapes are multiples of 16, so their pixel counts are multiples of 256; this case and the
    preprocess_u8_color one are the only ones that do."""
    u, colored = large_free
    assert u.shape[0] * u.shape[1] * u.shape[2] > PC.GRID_CAP_PIXELS and (u.shape[0] * u.shape[1] * u.shape[2]) % 256
    msg = PC.first_mismatch(color_aug_u8(u, LARGE_COLOR), colored, PC.decode_large)
    assert not msg, msg


def test_capped_grid_preprocess_u8_color(large_free):
    u, colored = large_free
    got = preprocess_u8(u, PC.LARGE_CODES, ZERO3, ONE3, 1.0, color=LARGE_COLOR)
    assert_bytes(got, "fp32", PC.ref_batch(colored, PC.LARGE_CODES), "preprocess_u8_color 5x460x457", PC.decode_large)


def test_capped_grid_preprocess_u8():
    """one thread per destination pixel under the pipeline's one grid cap, 4096 blocks of 256 threads: 5 x 460 x 457 = 1,051,100
    pixels of four channels each are more than the 1,048,576 the grid holds, so the last 2,524 pixels are a thread's second
    trip and that trip ends inside a block"""
    n, h, w = PC.LARGE_SHAPES["free"]
    u = PC.tagged_large(n, h, w, 4)
    assert n * h * w > PC.GRID_CAP_PIXELS and (n * h * w) % 256
    got = preprocess_u8(u, PC.LARGE_CODES, None, None, 1.0)
    assert_bytes(got, "fp32", PC.ref_batch(u, PC.LARGE_CODES), "preprocess_u8 5x460x457x4", PC.decode_large)


def test_capped_grid_stage_u8_and_stage_u8_color():
    """N = 5, 464 x 464, bf16 on a plan pruned to depth 1 (a small arena): 1,076,480 pixels, 27,904 of them a second trip.
    Both staging kernels, tagged content, a different code per sample; the padding channels of every pixel are zero bits."""
    n, h, w = PC.LARGE_SHAPES["plan"]
    u = PC.tagged_large(n, h, w)
    assert n * h * w > PC.GRID_CAP_PIXELS
    pl = make_plan(n, h, w, 3, "bf16", depth=1)
    print("capped-grid plan (N=%d, %dx%d, bf16, depth 1): arena_bytes = %d (%.1f MiB)" % (n, h, w, pl.arena_bytes, pl.arena_bytes / 2.0 ** 20))
    img, bits = stage(pl, u, PC.LARGE_CODES, None, None, 1.0, check_rest=False)
    assert_bytes(img[..., :3], "bf16", PC.ref_batch(u, PC.LARGE_CODES), "stage_u8 5x464x464", PC.decode_large)
    assert not bits[..., 3:].any()
    del img, bits
    img, bits = stage(pl, u, PC.LARGE_CODES, ZERO3, ONE3, 1.0, color=LARGE_COLOR, check_rest=False)
    exp = PC.ref_batch(CC.apply_batch(u, LARGE_COLOR), PC.LARGE_CODES)
    assert_bytes(img[..., :3], "bf16", exp, "stage_u8_color 5x464x464", PC.decode_large)
    assert not bits[..., 3:].any()


# -- 7. the captured step keeps image and mask paired ----------------------------------------------------------------------------
def test_image_and_mask_stay_paired_inside_the_captured_step(synth):
    from nunet_amd.trainer import TrainStep
    n, hw = 16, 32
    raw, m8 = synth.synth_blob_pairs_u8(n, hw, hw, seed=5)
    raw[..., 0] = m8[..., 0]                                   # channel 0 is 255 where the mask is set and 0 elsewhere
    src = m8[..., 0] > 127
    assert 0.05 < src.mean() < 0.95 and all(0 < src[i].sum() < hw * hw for i in range(n))
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="bf16").to(DEV).train()
    ts = TrainStep(m, (n, 3, hw, hw), lr=1e-3, input_u8=True, segmented=False, schedule="lanes")
    rd, md = dev(raw), dev(m8)
    ts.capture(rd, md)
    assert ts.g_fb is not None, "the step was captured"
    lo, hi = ((0.0 - D.MEAN[0]) / D.STD[0]) / 255.0, ((1.0 - D.MEAN[0]) / D.STD[0]) / 255.0
    mid = 0.5 * (lo + hi)

    def pair():
        torch.cuda.synchronize()
        ch0 = ts.pl.image()[..., 0].float().cpu().numpy()
        assert np.all(np.abs(ch0 - np.where(ch0 > mid, hi, lo)) < 2.0 ** -8 * abs(hi)), "channel 0 holds the two bf16 levels only"
        return ch0 > mid, ts.t[:, 0].cpu().numpy() > 0.5

    codes, steps0 = list(range(16)), ts.steps
    ts.step_u8(rd, md, aug_dev(codes))
    img, tgt = pair()
    exp = PC.ref_batch(src[..., None], codes)[..., 0]
    for i in range(n):
        assert np.array_equal(img[i], tgt[i]), "sample %d (code %d): image and mask were transformed differently" % (i, codes[i])
        assert np.array_equal(tgt[i], exp[i]), "sample %d (code %d): not rot90 / flip of the source" % (i, codes[i])
    assert sum(not np.array_equal(exp[i], src[i]) for i in range(n)) >= 14, "the codes moved the blobs"
    ts.step_u8(rd, md)                                           # aug=None: the static code buffer is cleared
    img, tgt = pair()
    assert int(ts.aug.abs().sum()) == 0
    assert np.array_equal(img, src) and np.array_equal(tgt, src)
    assert ts.steps == steps0 + 2


# -- 8. refusals -----------------------------------------------------------------------------------------------------------------
BAD_AUG = [("short", lambda n: torch.zeros(n - 1, dtype=torch.int32, device=DEV)),
           ("long", lambda n: torch.zeros(n + 1, dtype=torch.int32, device=DEV)),
           ("two-dimensional", lambda n: torch.zeros((n, 1), dtype=torch.int32, device=DEV)),
           ("scalar", lambda n: torch.zeros((), dtype=torch.int32, device=DEV)),
           ("int64", lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)),
           ("host", lambda n: torch.zeros(n, dtype=torch.int32))]


@pytest.fixture
def no_launch(monkeypatch):
    """A refusal is shown without letting the launch go ahead: while this is active the library's pipeline entries are
    replaced by a recorder, so even a missing check launches nothing."""
    calls = []
    lib = L.lib()
    for name in ("nunet_preprocess_u8", "nunet_preprocess_u8_color", "nunet_plan_stage_u8", "nunet_plan_stage_u8_color"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append(_n) or 0, raising=True)
    return calls


def test_preprocess_entries_refuse_bad_codes_before_a_launch(no_launch):
    n = 4
    img = torch.zeros((n, 16, 32, 3), dtype=torch.uint8, device=DEV)
    msk = torch.zeros((n, 16, 32, 1), dtype=torch.uint8, device=DEV)
    odd = torch.tensor([0, 2, 1, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(L.NunetError, match="square"):
        D.preprocess_masks(msk, odd)
    with pytest.raises(L.NunetError, match="square"):
        D.preprocess_images(img, odd)
    for name, make in BAD_AUG:
        for fn, x in ((D.preprocess_images, img), (D.preprocess_masks, msk)):
            with pytest.raises(L.NunetError, match="aug"):
                fn(x, make(n))
        with pytest.raises(L.NunetError, match="aug"):
            D.preprocess_images(img, make(n), color=torch.zeros((n, 4), dtype=torch.int32, device=DEV))
    assert no_launch == [], "a refused call reached the library: %s" % no_launch
    # what is allowed still goes through (to the recorder)
    D.preprocess_masks(msk, torch.tensor([0, 2, 6, 12], dtype=torch.int32, device=DEV))
    D.preprocess_masks(msk[:, :, :16].contiguous(), torch.tensor([0, 1, 3, 15], dtype=torch.int32, device=DEV))
    D.preprocess_images(img, None)
    assert no_launch == ["nunet_preprocess_u8"] * 3


def test_step_u8_refuses_bad_codes_before_a_launch(no_launch, monkeypatch):
    from nunet_amd.trainer import TrainStep
    n = 2
    m = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).train()
    ts = TrainStep(m, (n, 3, 16, 32), input_u8=True, use_graph=False)
    ran = []
    monkeypatch.setattr(ts, "_run", lambda: ran.append(1))
    ts.t.fill_(7.0)
    ts.pl.arena.fill_(FILL)
    ts.x_u8.fill_(9)
    x = torch.zeros((n, 16, 32, 3), dtype=torch.uint8, device=DEV)
    t = torch.zeros((n, 16, 32, 1), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.NunetError, match="square"):
        ts.step_u8(x, t, torch.tensor([2, 3], dtype=torch.int32, device=DEV))
    for name, make in BAD_AUG:
        with pytest.raises(L.NunetError, match="aug"):
            ts.step_u8(x, t, make(n))
    torch.cuda.synchronize()
    assert ran == [] and no_launch == [] and ts.steps == 0
    assert bool((ts.t == 7.0).all()) and bool((ts.pl.arena == FILL).all()) and bool((ts.x_u8 == 9).all()), "a refused step touched its static buffers"
    ts.step_u8(x, t, torch.tensor([2, 12], dtype=torch.int32, device=DEV))
    assert ran == [1]
