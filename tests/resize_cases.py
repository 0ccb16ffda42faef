"""numpy oracle and case tables of the device-side Resize on ragged uint8 sources (nunet_resize_u8, nunet_preprocess_u8_resize,
nunet_plan_stage_u8_resize; include/nunet.h). The definition is the project's own (input pipeline) - modelled on
OpenCV's 8-bit INTER_LINEAR (two passes, 11-bit coefficients) and INTER_NEAREST, not captured from a cv2 run - so this file is
the oracle of tests/test_resize_cpu.py and tests/test_resize_gpu.py, not a copy of a library's output.

Order. The reference augments the source, then resizes (trains.py:257-267). reference() states that FORWARD with library
calls: pipeline_cases.ref_geometry on the source, color_cases' oracle, then the resize. The kernels are destination-driven
(destination pixel -> four taps in the augmented view -> inverse index map -> source bytes, the colour op on every fetched
tap); restate() is a numpy copy of that path, kept apart and used to show that it equals reference() and that the listed
mutations are detected on the tables."""
import numpy as np

import color_cases as CC
import pipeline_cases as PC

LINEAR, NEAREST = 0, 1
MAX_EXTENT = 16384

TAP_MUTATIONS = ("no_half_pixel", "swap_a", "s_for_d")
ORDER_MUTATIONS = ("resize_first", "hs_for_ws")


# -- the definition ------------------------------------------------------------------------------------------------------------
def taps(S, D, mutate=None):
    """one axis: (s0, s1, a0, a1) int64 arrays over the D destination indices"""
    assert mutate is None or mutate in TAP_MUTATIONS, mutate
    d = np.arange(D, dtype=np.int64)
    if mutate == "s_for_d":
        num, den = (2 * d + 1) * D - S, 2 * S
    elif mutate == "no_half_pixel":
        num, den = 2 * d * S, 2 * D
    else:
        num, den = (2 * d + 1) * S - D, 2 * D
    neg = num < 0
    pos = np.where(neg, 0, num)
    s, r = pos // den, pos % den
    edge = s >= S - 1
    s = np.where(edge, S - 1, s)
    a1 = np.where(neg | edge, 0, (r * 4096 + den) // (2 * den))
    a0 = 2048 - a1
    if mutate == "swap_a":
        a0, a1 = a1, a0
    return s, np.minimum(s + 1, S - 1), a0, a1


def bilinear(src, Hd, Wd, mutate=None):
    """uint8 [H,W,C] -> uint8 [Hd,Wd,C]: horizontal pass, then the vertical one"""
    H, W, _ = src.shape
    y0, y1, b0, b1 = taps(H, Hd, mutate)
    x0, x1, a0, a1 = taps(W, Wd, mutate)
    s = src.astype(np.int64)
    R = (s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]) >> 4
    out = (((b0[:, None, None] * R[y0]) >> 16) + ((b1[:, None, None] * R[y1]) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def bilinear_f64(src, Hd, Wd):
    """fp64 bilinear of the SAME taps with the exact weights a1 / 2048: what the integer form may differ from by < 1 byte"""
    H, W, _ = src.shape
    y0, y1, b0, b1 = taps(H, Hd)
    x0, x1, a0, a1 = taps(W, Wd)
    s = src.astype(np.float64)
    R = s[:, x0] * (a0 / 2048.0)[None, :, None] + s[:, x1] * (a1 / 2048.0)[None, :, None]
    return R[y0] * (b0 / 2048.0)[:, None, None] + R[y1] * (b1 / 2048.0)[:, None, None]


def nearest_index(S, D):
    return np.minimum(np.arange(D, dtype=np.int64) * S // D, S - 1)


def nearest(src, Hd, Wd):
    H, W, _ = src.shape
    return np.ascontiguousarray(src[nearest_index(H, Hd)][:, nearest_index(W, Wd)])


def resize(src, Hd, Wd, mode=LINEAR, mutate=None):
    return nearest(src, Hd, Wd) if mode == NEAREST else bilinear(src, Hd, Wd, mutate)


def reference(src, Hd, Wd, mode=LINEAR, code=0, color=None, mutate=None):
    """FORWARD: augment the source (any shape, any code), colour op, resize. mutate 'resize_first': the other order."""
    assert mutate is None or mutate == "resize_first" or mutate in TAP_MUTATIONS
    if mutate == "resize_first":
        k_odd = code & 1
        out = resize(src, Wd if k_odd else Hd, Hd if k_odd else Wd, mode)      # so that the augmented result is Hd x Wd
        out = PC.ref_geometry(out, code)
        return out if color is None else CC.apply(out, *color)
    v = PC.ref_geometry(src, code)
    if color is not None:
        v = CC.apply(v, *color)
    return resize(v, Hd, Wd, mode, mutate)


def restate(src, Hd, Wd, mode=LINEAR, code=0, color=None, mutate=None):
    """The kernels' destination-driven path: taps in the augmented view, each through the inverse index map (as
    pipeline_cases.restate_batch states it, with the view's extents where the source is not square) to a flat source address,
    the colour op on the fetched taps. mutate 'hs_for_ws': the view of an odd rot90 count keeps the source's extents; its
    addresses may leave the sample and are wrapped (any value would do: the pixel is wrong)."""
    assert mutate is None or mutate == "hs_for_ws"
    Hs, Ws, C = src.shape
    k = code & 3
    Hv, Wv = (Ws, Hs) if (k & 1) and mutate != "hs_for_ws" else (Hs, Ws)
    flat = src.reshape(Hs * Ws, C)

    def fetch(vy, vx):
        sy, sx = np.meshgrid(vy, vx, indexing="ij")
        if code & 8:
            sy = Hv - 1 - sy
        if code & 4:
            sx = Wv - 1 - sx
        if k == 1:
            ry, rx = sx, Ws - 1 - sy
        elif k == 2:
            ry, rx = Hs - 1 - sy, Ws - 1 - sx
        elif k == 3:
            ry, rx = Hs - 1 - sx, sy
        else:
            ry, rx = sy, sx
        px = flat[np.mod(ry * Ws + rx, Hs * Ws)]
        return px if color is None else CC.apply(px, *color)

    if mode == NEAREST:
        return np.ascontiguousarray(fetch(nearest_index(Hv, Hd), nearest_index(Wv, Wd)))
    y0, y1, b0, b1 = taps(Hv, Hd)
    x0, x1, a0, a1 = taps(Wv, Wd)
    a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
    p = [[fetch(vy, vx).astype(np.int64) for vx in (x0, x1)] for vy in (y0, y1)]
    r0 = (p[0][0] * a0 + p[0][1] * a1) >> 4
    r1 = (p[1][0] * a0 + p[1][1] * a1) >> 4
    return ((((b0 * r0) >> 16) + ((b1 * r1) >> 16) + 2) >> 2).astype(np.uint8)


# -- ragged batches ------------------------------------------------------------------------------------------------------------
def pack(samples):
    """list of [H,W,C] uint8 -> (pool uint8 [bytes], descriptors int32 [N,4]: offset as two little-endian words, H, W), tight"""
    desc = np.zeros((len(samples), 4), np.int32)
    off = 0
    for i, s in enumerate(samples):
        desc[i:i + 1].view(np.int64)[0, 0] = off
        desc[i, 2], desc[i, 3] = s.shape[0], s.shape[1]
        off += s.size
    return np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in samples]), desc


def reference_batch(samples, Hd, Wd, mode=LINEAR, codes=None, colors=None):
    return np.stack([reference(s, Hd, Wd, mode, 0 if codes is None else int(codes[i]), None if colors is None else colors[i])
                     for i, s in enumerate(samples)])


# -- case tables ---------------------------------------------------------------------------------------------------------------
DST_SHAPES = [(16, 16), (32, 32), (16, 48), (48, 16)]              # what a plan takes (multiples of 16)
SRC_SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (16, 16), (32, 32), (37, 53), (100, 75), (255, 3)]
UPSCALE = ((8, 8), (32, 32))
# one batch of 16 ragged samples, none square: sample n has code n, so every one of the 16 codes meets a non-square source
BATCH_SHAPES = [(7, 5), (37, 53), (100, 75), (255, 3), (1, 9), (9, 1), (53, 37), (5, 7),
                (75, 100), (3, 255), (37, 53), (7, 5), (9, 1), (100, 75), (1, 9), (53, 37)]
BATCH_CODES = list(range(16))
# a second, shorter batch that mixes every source shape of the table, the upscale source included
MIXED_SHAPES = SRC_SHAPES + [UPSCALE[0]]
MIXED_CODES = [0, 1 | 4, 3 | 8, 1, 2 | 4, 12, 3, 1 | 12, 3 | 4, 2]
# the capped grid: N * Hd * Wd just over pipeline_cases.GRID_CAP_PIXELS (4096 blocks x 256 threads), so threads take a second trip
LARGE_DST = PC.LARGE_SHAPES["plan"]                                # (5, 464, 464)
LARGE_SRC = [(100, 75), (37, 53), (464, 464), (255, 3), (75, 100)]
LARGE_CODES = [1 | 4, 0, 8, 3, 2 | 4 | 8]
# colour codes of the batches (color_cases): every op, NONE among them
COLOR_CODES = [CC.BYTE_CODES[i % len(CC.BYTE_CODES)] for i in range(16)]


def sources(shapes, c, seed=5):
    """random uint8 [H,W,c] per shape; masks (binary=True) in {0, 255}"""
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in shapes]


def binary_sources(shapes, c, seed=6):
    g = np.random.default_rng(seed)
    return [(g.integers(0, 2, (h, w, c), dtype=np.uint8) * 255).astype(np.uint8) for h, w in shapes]
