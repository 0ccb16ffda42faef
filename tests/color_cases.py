"""numpy restatement of the colour augmentation the device pipeline runs (include/nunet.h, nunet_color_aug; DESIGN.md, input
pipeline): OneOf([HueSaturationValue(), RandomBrightness(), RandomContrast()], p=1) of the reference's train transform
(trains.py:260-264). The definition is the project's own - modelled on albumentations' uint8 paths and OpenCV's 8-bit RGB2HSV /
HSV2RGB with hue range 180, not captured from them - so this file is the oracle of tests/test_color_aug_cpu.py and
tests/test_color_aug_gpu.py, not a copy of a library's output.

The forward conversion is integer. The inverse is written twice: in np.float32 with one ufunc per operation (every operation
rounded on its own, no fused multiply-add: the bytes the kernels must produce) and in np.float64 (what the fp32 bytes may differ
from by at most one level)."""
import numpy as np

NONE, HSV, BRIGHTNESS, CONTRAST = 0, 1, 2, 3

_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint((255 << 12) / _I)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint((180 << 12) / (6.0 * _I))]).astype(np.int64)


def rgb_to_hsv(rgb):
    """uint8 [..., 3] -> (h, s, v) int64, h in [0, 179]"""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * SDIV[v] + 2048) >> 12
    hn = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (hn * HDIV[diff] + 2048) >> 12            # arithmetic shift
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def shift_hsv(h, s, v, p0, p1, p2):
    """the three shifts in double (p0, p1, p2 are fp32 values); truncated to integers"""
    p0, p1, p2 = (np.float64(np.float32(p)) for p in (p0, p1, p2))
    x = h.astype(np.float64) + p0
    h2 = np.trunc(np.where(x < 0, x + 180.0, np.where(x >= 180.0, x - 180.0, x))).astype(np.int64)
    s2 = np.trunc(np.clip(s.astype(np.float64) + p1, 0.0, 255.0)).astype(np.int64)
    v2 = np.trunc(np.clip(v.astype(np.float64) + p2, 0.0, 255.0)).astype(np.int64)
    return h2, s2, v2


def hsv_to_rgb(h, s, v, ft):
    """(h, s, v) integers -> uint8 [..., 3]; ft = np.float32 (one ufunc per operation) or np.float64"""
    one, six = ft(1), ft(6)
    H = np.multiply(h.astype(ft), np.divide(six, ft(180)))
    H = np.where(H >= six, np.subtract(H, six), H)
    S = np.multiply(s.astype(ft), np.divide(one, ft(255)))
    V = np.multiply(v.astype(ft), np.divide(one, ft(255)))
    sec = np.floor(H)
    fr = np.subtract(H, sec)
    inside = (sec >= 0) & (sec <= 5)
    sec = np.where(inside, sec, 0).astype(np.int64)
    fr = np.where(inside, fr, ft(0))
    p = np.multiply(V, np.subtract(one, S))
    q = np.multiply(V, np.subtract(one, np.multiply(S, fr)))
    t = np.multiply(V, np.subtract(one, np.multiply(S, np.subtract(one, fr))))
    assert all(a.dtype == ft for a in (H, S, V, fr, p, q, t))
    table = (((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)))
    out = np.zeros(h.shape + (3,), np.uint8)
    for c in range(3):
        x = np.choose(sec, [table[k][c] for k in range(6)])
        out[..., c] = np.clip(np.rint(np.multiply(x, ft(255))), 0, 255).astype(np.uint8)      # ties to even
    return out


def hsv_op(rgb, p0, p1, p2, ft=np.float32):
    return hsv_to_rgb(*shift_hsv(*rgb_to_hsv(rgb), p0, p1, p2), ft)


def lut_op(rgb, alpha, b255):
    """albumentations brightness_contrast_adjust, uint8 LUT, beta_by_max=True: alpha and b255 = float(beta * 255.0) are fp32"""
    f = rgb.astype(np.float32)
    if np.float32(alpha) != 1:
        f = np.multiply(f, np.float32(alpha))
    if np.float32(b255) != 0:
        f = np.add(f, np.float32(b255))
    assert f.dtype == np.float32
    return np.clip(f, 0, 255).astype(np.uint8)              # truncation


def apply(rgb, op, p0=0.0, p1=0.0, p2=0.0, ft=np.float32):
    """one sample [H, W, 3] through one code; any op outside 1..3 is NONE"""
    if op == HSV:
        return hsv_op(rgb, p0, p1, p2, ft)
    if op == BRIGHTNESS:
        return lut_op(rgb, 1.0, p0)
    if op == CONTRAST:
        return lut_op(rgb, p0, 0.0)
    return rgb.copy()


def apply_batch(u8, codes, ft=np.float32):
    return np.stack([apply(u8[i], *codes[i], ft=ft) for i in range(len(codes))])


def b255(beta):
    """the BRIGHTNESS parameter of a beta: formed in double, rounded to fp32 once"""
    return float(np.float32(np.float64(beta) * 255.0))


# -- case tables -----------------------------------------------------------------------------------------------------------------
# one code per sample of the 7-image byte test: (op, p0, p1, p2)
BYTE_CODES = [(HSV, 0.0, 0.0, 0.0), (HSV, 20.0, 30.0, 20.0), (HSV, -20.0, -30.0, -20.0), (HSV, 13.7, -22.4, 9.2),
              (BRIGHTNESS, b255(-0.2), 0.0, 0.0), (CONTRAST, 1.2, 0.0, 0.0), (NONE, 0.0, 0.0, 0.0)]
# second pass: parameters outside what draw_color_augmentation draws, and an op that is none of the three
OUT_OF_RANGE_CODES = [(CONTRAST, 2.0, 0.0, 0.0), (BRIGHTNESS, b255(-1.0), 0.0, 0.0), (9, 5.0, 5.0, 5.0), (CONTRAST, 2.0, 0.0, 0.0),
                      (BRIGHTNESS, b255(-1.0), 0.0, 0.0), (9, 5.0, 5.0, 5.0), (CONTRAST, 2.0, 0.0, 0.0)]
# small and odd shapes: (N, H, W, in place)
SMALL_SHAPES = [(3, 5, 7, False), (2, 33, 31, False), (2, 33, 31, True)]
SMALL_CODES = [(HSV, 13.7, -22.4, 9.2), (CONTRAST, 1.2, 0.0, 0.0), (BRIGHTNESS, b255(0.15), 0.0, 0.0)]
BLUES = (0, 51, 102, 153, 204, 255)


def byte_batch(seed=3):
    """7 x 256 x 256 x 3: images 0-5 have r = x, g = y and a constant b (every v and every diff occurs), image 6 is random"""
    u = np.zeros((7, 256, 256, 3), np.uint8)
    ramp = np.arange(256, dtype=np.uint8)
    for i, bl in enumerate(BLUES):
        u[i, :, :, 0] = ramp[None, :]
        u[i, :, :, 1] = ramp[:, None]
        u[i, :, :, 2] = bl
    u[6] = np.random.default_rng(seed).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    return u
