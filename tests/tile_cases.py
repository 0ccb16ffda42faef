"""numpy oracle of the tiled-inference geometry (nunet_amd.tiled, include/nunet.h: nunet_tile / nunet_tile_grid): tile origins,
BORDER_REFLECT_101, the uint8 crop, the fp64 stitch - written from the definitions, not from tiled.py - and the case lists the
CPU and GPU tests share."""
import numpy as np

import resize_cases as RC

TENT, UNIFORM = "tent", "uniform"


def origins(S, T, O):
    """walk from 0 in steps of T - O while a whole tile still fits before the last, flush one"""
    if S <= T:
        return [0]
    out, o = [], 0
    while o < S - T:
        out.append(o)
        o += T - O
    return out + [S - T]


def reflect_loop(i, S):
    """index i >= 0 of an axis of extent S under BORDER_REFLECT_101, repeated: walk i steps, turning at both ends"""
    pos, step = 0, 1
    for _ in range(i):
        if S == 1:
            break
        if pos + step < 0 or pos + step >= S:
            step = -step
        pos += step
    return pos


def crop(src, y0, x0, Th, Tw):
    """the Th x Tw window of src [H,W,C] at (y0, x0); rows / columns at or past the extent through the reflection"""
    H, W = src.shape[:2]
    ys = [y if y < H else reflect_loop(y, H) for y in range(y0, y0 + Th)]
    xs = [x if x < W else reflect_loop(x, W) for x in range(x0, x0 + Tw)]
    return np.ascontiguousarray(src[np.ix_(ys, xs)])


def window(T, kind):
    return np.asarray([min(i + 1, T - i) if kind == TENT else 1 for i in range(T)], np.float64)


def tables(shapes, Th, Tw, O, K):
    """(tiles int32 [n,4], grids int32 [n_samples,8], out_elems): the layout nunet_amd.tiled.build_tables documents"""
    tiles, grids, off = [], np.zeros((len(shapes), 8), np.int32), 0
    for n, (H, W) in enumerate(shapes):
        oy, ox = origins(H, Th, O), origins(W, Tw, O)
        grids[n:n + 1].view(np.int64)[0, 0] = off
        grids[n, 2:7] = (len(tiles), len(oy), len(ox), Th - O, Tw - O)
        for y0 in oy:
            for x0 in ox:
                tiles.append((n, y0, x0, 0))
        off += -(-K * H * W // 4) * 4          # every block starts at a multiple of 4 elements
    return np.asarray(tiles, np.int32).reshape(-1, 4), grids, off


def stitch(tile_logits, tiles, n, H, W, kind):
    """fp64 blend of sample n: tile_logits [n_tiles,K,Th,Tw], tiles as tables() lists them -> (blend [K,H,W], cover [H,W])"""
    _, K, Th, Tw = tile_logits.shape
    wy, wx = window(Th, kind), window(Tw, kind)
    num, den, cover = np.zeros((K, H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
    for t, (s, y0, x0, _) in enumerate(tiles):
        if s != n:
            continue
        h, w = min(Th, H - y0), min(Tw, W - x0)
        wt = np.outer(wy[:h], wx[:w])
        num[:, y0:y0 + h, x0:x0 + w] += wt * tile_logits[t, :, :h, :w].astype(np.float64)
        den[y0:y0 + h, x0:x0 + w] += wt
        cover[y0:y0 + h, x0:x0 + w] += 1
    assert cover.min() >= 1
    return num / den, cover


def single_cover_values(tile_logits, tiles, n, H, W):
    """fp32 [K,H,W]: where exactly one tile covers a pixel, that tile's own logit (elsewhere whatever tile came last)"""
    _, K, Th, Tw = tile_logits.shape
    out = np.zeros((K, H, W), np.float32)
    for t, (s, y0, x0, _) in enumerate(tiles):
        if s == n:
            h, w = min(Th, H - y0), min(Tw, W - x0)
            out[:, y0:y0 + h, x0:x0 + w] = tile_logits[t, :, :h, :w]
    return out


# -- case tables ---------------------------------------------------------------------------------------------------------------
SRC_SHAPES = [(1, 1), (5, 40), (16, 16), (17, 16), (33, 70), (40, 56)]
C1_SHAPES = [(5, 40), (33, 70)]                       # the C = 1 case
TILE_CASES = [(16, 16, 0), (16, 16, 4), (16, 16, 8), (32, 32, 0), (32, 32, 8), (32, 32, 16), (16, 32, 8)]     # (Th, Tw, overlap)
TILE_IDS = ["%dx%d-o%d" % c for c in TILE_CASES]
# one sample whose K * H * W is past the stitch launch's 2048 workgroups x 256 threads: threads take a second trip
LARGE_SHAPE, LARGE_K, LARGE_TILE = (420, 421), 3, (32, 32, 8)
STITCH_GRID_THREADS = 2048 * 256


def sources(shapes=SRC_SHAPES, c=3, seed=31):
    return RC.sources(shapes, c, seed)


def logit_tolerance(tile_logits):
    """16 * 2^-24 * max|logit|: a 9-term fp32 weighted mean plus one division is within 11 * 2^-24 * max|logit| of the exact
    value; the rest is margin for fused versus separately rounded multiply-adds"""
    return 16.0 * 2.0 ** -24 * float(np.abs(tile_logits).max())
