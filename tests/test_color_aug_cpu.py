"""Colour augmentation, host side (no GPU): dataset.draw_color_augmentation draws what OneOf([HueSaturationValue(),
RandomBrightness(), RandomContrast()], p=1) draws (trains.py:260-264), and the numpy oracle of tests/color_cases.py - the
project's own definition of the three ops - has the properties the definition promises."""
import numpy as np
import torch

import nunet_amd
from nunet_amd import _lib as L
from nunet_amd import dataset as D

import color_cases as CC


def _decode(codes):
    w = codes.numpy()
    return w[:, 0], np.ascontiguousarray(w[:, 1:]).view(np.float32)


def test_draw_shape_dtype_and_ops():
    c = D.draw_color_augmentation(300, torch.Generator().manual_seed(5), "cpu")
    assert c.shape == (300, L.COLOR_WORDS) and c.dtype == torch.int32 and c.is_contiguous()
    op, _ = _decode(c)
    assert set(op.tolist()) == {L.COLOR_HSV, L.COLOR_BRIGHTNESS, L.COLOR_CONTRAST}, "each op is present in 300 draws, and nothing else"
    assert (L.COLOR_NONE, L.COLOR_HSV, L.COLOR_BRIGHTNESS, L.COLOR_CONTRAST) == (CC.NONE, CC.HSV, CC.BRIGHTNESS, CC.CONTRAST)


def test_draw_parameter_ranges():
    op, par = _decode(D.draw_color_augmentation(3000, torch.Generator().manual_seed(6), "cpu"))
    assert par.dtype == np.float32 and np.all(np.isfinite(par))
    hsv, bri, con = par[op == CC.HSV], par[op == CC.BRIGHTNESS], par[op == CC.CONTRAST]
    for k, lim in enumerate((20.0, 30.0, 20.0)):
        assert np.all(np.abs(hsv[:, k]) <= lim)
        assert hsv[:, k].min() < -0.8 * lim and hsv[:, k].max() > 0.8 * lim, "the range is used"
    assert np.all(np.abs(bri[:, 0]) <= np.float32(0.2 * 255.0)) and np.all(bri[:, 1:] == 0)
    assert bri[:, 0].min() < -0.8 * 51 and bri[:, 0].max() > 0.8 * 51
    assert np.all(con[:, 0] >= np.float32(0.8)) and np.all(con[:, 0] <= np.float32(1.2)) and np.all(con[:, 1:] == 0)
    assert con[:, 0].min() < 0.84 and con[:, 0].max() > 1.16


def test_draw_is_deterministic_under_a_seed():
    a = D.draw_color_augmentation(64, torch.Generator().manual_seed(11), "cpu")
    b = D.draw_color_augmentation(64, torch.Generator().manual_seed(11), "cpu")
    c = D.draw_color_augmentation(64, torch.Generator().manual_seed(12), "cpu")
    assert torch.equal(a, b) and not torch.equal(a, c)
    g = torch.Generator().manual_seed(11)           # a stream: the second draw differs from the first
    assert torch.equal(D.draw_color_augmentation(64, g, "cpu"), a) and not torch.equal(D.draw_color_augmentation(64, g, "cpu"), a)


def test_color_codes_pack_the_struct():
    w = D.color_codes([1, 3], [[13.7, -22.4, 9.2], [1.2, 0, 0]])
    assert w.dtype == torch.int32 and w.shape == (2, 4)
    op, par = _decode(w)
    assert op.tolist() == [1, 3]
    assert np.array_equal(par, np.array([[13.7, -22.4, 9.2], [1.2, 0, 0]], np.float32))


def test_division_tables():
    assert CC.SDIV[0] == 0 and CC.HDIV[0] == 0 and CC.SDIV[255] == 4096 and CC.SDIV[1] == 255 << 12 and CC.HDIV[1] == 30 << 12
    i = np.arange(1, 256)
    # neither quotient has a fraction of one half, so the integer rounding the kernels' table uses gives the same values
    assert np.array_equal(CC.SDIV[1:], (2 * (255 << 12) + i) // (2 * i))
    assert np.array_equal(CC.HDIV[1:], (2 * (180 << 12) + 6 * i) // (12 * i))


def test_oracle_primaries_and_greys_survive_a_zero_shift():
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for ft in (np.float32, np.float64):
        assert np.array_equal(CC.hsv_op(prim, 0, 0, 0, ft), prim)
        assert np.array_equal(CC.hsv_op(grey, 0, 0, 0, ft), grey)
        for hue in (-20.0, 7.3, 20.0):           # s = 0: the hue does not matter
            assert np.array_equal(CC.hsv_op(grey, hue, 0, 0, ft), grey)


def test_oracle_hue_range_and_round_trip():
    rgb = np.random.default_rng(0).integers(0, 256, (1 << 18, 3), dtype=np.uint8)
    h, s, v = CC.rgb_to_hsv(rgb)
    assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
    assert np.array_equal(v, rgb.max(axis=1))
    a32, a64 = CC.hsv_op(rgb, 0, 0, 0, np.float32), CC.hsv_op(rgb, 0, 0, 0, np.float64)
    err = np.abs(a32.astype(int) - rgb.astype(int))
    assert err.max() <= 5 and err.mean() < 0.5, "the zero-shift round trip is close to, but not, the identity"
    assert err.max() > 0
    d = np.abs(a32.astype(int) - a64.astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 0.005
    b32, b64 = CC.hsv_op(rgb, 13.7, -22.4, 9.2, np.float32), CC.hsv_op(rgb, 13.7, -22.4, 9.2, np.float64)
    d = np.abs(b32.astype(int) - b64.astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 0.005


def test_oracle_fp32_against_fp64_on_the_byte_test_batch():
    """The GPU test's batch and codes through both oracles: what the fp32 definition itself differs from fp64 by, per sample and
    over the HSV samples together (the figure the GPU test caps at 0.5 %), and on random colours under every HSV code."""
    u = CC.byte_batch()
    hsv = [i for i, c in enumerate(CC.BYTE_CODES) if c[0] == CC.HSV]
    assert hsv == [0, 1, 2, 3]
    a32, a64 = CC.apply_batch(u[:4], CC.BYTE_CODES[:4], np.float32), CC.apply_batch(u[:4], CC.BYTE_CODES[:4], np.float64)
    d = np.abs(a32.astype(int) - a64.astype(int))
    for i in hsv:
        print("image %d code %s: fp32 != fp64 in %.4f %% of bytes" % (i, CC.BYTE_CODES[i], 100.0 * (d[i] != 0).mean()))
    print("HSV samples together: %.4f %%" % (100.0 * (d != 0).mean()))
    assert d.max() <= 1 and (d != 0).mean() <= 0.005
    for c in CC.BYTE_CODES[:4]:
        dr = np.abs(CC.apply(u[6], *c, ft=np.float32).astype(int) - CC.apply(u[6], *c, ft=np.float64).astype(int))
        print("random colours, code %s: fp32 != fp64 in %.4f %% of bytes" % (c, 100.0 * (dr != 0).mean()))
        assert dr.max() <= 1


def test_oracle_lut_ops():
    u = np.arange(256, dtype=np.uint8).reshape(-1, 1).repeat(3, axis=1)
    assert np.array_equal(CC.apply(u, CC.BRIGHTNESS, 0.0), u) and np.array_equal(CC.apply(u, CC.CONTRAST, 1.0), u)
    assert np.array_equal(CC.apply(u, CC.NONE, 5.0, 5.0, 5.0), u) and np.array_equal(CC.apply(u, 9, 5.0, 5.0, 5.0), u)
    dark = CC.apply(u, CC.BRIGHTNESS, CC.b255(-0.2))
    assert dark[0, 0] == 0 and dark[51, 0] == 0 and dark[52, 0] == 1 and dark[255, 0] == 204
    hi = CC.apply(u, CC.CONTRAST, 1.2)
    assert hi[255, 0] == 255 and hi[213, 0] == 255 and hi[10, 0] == 12 and hi[1, 0] == 1      # 1.2f * 1 = 1.2000000477 -> 1
    assert np.array_equal(CC.apply(u, CC.CONTRAST, 2.0)[:, 0], np.minimum(2 * np.arange(256), 255))
    assert not CC.apply(u, CC.BRIGHTNESS, CC.b255(-1.0)).any()


def test_package_exports_the_surface():
    assert callable(nunet_amd.dataset.color_augment) and callable(nunet_amd.dataset.draw_color_augmentation)
    import inspect
    assert "color" in inspect.signature(nunet_amd.dataset.preprocess_images).parameters
    from nunet_amd.trainer import TrainStep
    assert "color_aug" in inspect.signature(TrainStep.__init__).parameters
    assert "color" in inspect.signature(TrainStep.step_u8).parameters
