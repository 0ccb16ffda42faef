"""Full-resolution tiled inference on the device (nunet_crop_tiles_u8, nunet_plan_stage_u8_tiles, nunet_stitch_tiles,
nunet_amd.tiled.TiledPredictor) against the numpy oracle of tests/tile_cases.py.

Criteria. The crop is a byte copy: its bytes must EQUAL the oracle's, and tiles that may read nothing are zeros. The fused
staging launch is compared bit for bit with crop + nunet_plan_stage_u8, and must write nothing outside the image. The stitch is
compared with the fp64 blend within 16 * 2^-24 * max|logit| (tile_cases.logit_tolerance: the bound of a 9-term fp32 weighted
mean and one division is 11 * 2^-24 * max|logit|), bit for bit where one tile covers a pixel, its bytes with nunet_sigmoid_u8 of
its own logits, and two runs with each other. One stitched sample is past the launch's 2048 x 256 threads. The whole path is
compared bit for bit with EvalStep where source == tile, and with oracle crop -> module forward -> fp64 stitch on ragged sources."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import dataset as D  # noqa: E402
from nunet_amd import tiled as T  # noqa: E402
from nunet_amd.engine import Plan  # noqa: E402
from nunet_amd.metrics import iou_logit_threshold, sigmoid_masks_u8, sigmoid_u8_thresholds  # noqa: E402
from nunet_amd.trainer import EvalStep  # noqa: E402
import pipeline_cases as PC  # noqa: E402
import resize_cases as RC  # noqa: E402
import tile_cases as TC  # noqa: E402

DEV = "cuda:0"
KINDS = {"fp32": L.F32, "bf16": L.BF16}
FILL = 0xA5
MEAN3, STD3 = np.asarray(D.MEAN, np.float32), np.asarray(D.STD, np.float32)


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


def dev(a):
    if a is None:
        return None
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = torch.empty(a.shape, dtype=a.dtype, device=DEV)
    t.copy_(a)
    return t


class Ragged:
    """a packed batch on the device: the pool sits in a guarded buffer of exactly its size"""

    def __init__(self, samples):
        pool, desc = RC.pack(samples)
        self.samples, self.pool_host, self.desc_host = samples, pool, desc
        self.n, self.c = len(samples), samples[0].shape[2]
        self.pool, self.desc, self.bytes = dev(pool), dev(desc), int(pool.size)
        self.shapes = [s.shape[:2] for s in samples]


def crop(r, desc_dev, tiles, th, tw):
    out = torch.full((tiles.shape[0], th, tw, r.c), 7, dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_crop_tiles_u8(L.ptr(r.pool), r.bytes, L.ptr(desc_dev), desc_dev.shape[0], L.ptr(dev(tiles)), tiles.shape[0], r.c, th, tw,
                                        L.ptr(out), L.stream()), "nunet_crop_tiles_u8")
    torch.cuda.synchronize()
    assert np.array_equal(r.pool.cpu().numpy(), r.pool_host), "the pool was written"
    return out


def oracle_crops(samples, tiles, th, tw):
    c = samples[0].shape[2]
    return np.stack([np.zeros((th, tw, c), np.uint8) if s < 0 else TC.crop(samples[s], y0, x0, th, tw) for s, y0, x0, _ in tiles])


def assert_tiles_equal(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for t in range(exp.shape[0]):
        bad = got[t] != exp[t]
        if bad.any():
            y, x, c = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: tile %d: %d of %d bytes differ; first at (y, x, c) = (%d, %d, %d): found %d, expected %d"
                                 % (what, t, int(bad.sum()), bad.size, y, x, c, int(got[t, y, x, c]), int(exp[t, y, x, c])))


NULL_TILE = np.asarray([[-1, 0, 0, 0]], np.int32)


# -- 1. nunet_crop_tiles_u8 against the oracle, byte for byte -----------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.TILE_CASES, ids=TC.TILE_IDS)
def test_crop_tiles_u8_equals_the_oracle(case):
    th, tw, o = case
    for c, shapes in ((3, TC.SRC_SHAPES), (1, TC.C1_SHAPES)):
        samples = TC.sources(shapes, c)
        r = Ragged(samples)
        tiles = TC.tables(shapes, th, tw, o, 1)[0]
        tiles = np.concatenate([tiles[:2], NULL_TILE, tiles[2:], NULL_TILE])        # null tiles inside and at the end
        assert_tiles_equal(crop(r, r.desc, tiles, th, tw), oracle_crops(samples, tiles, th, tw), "crop %s C=%d" % (case, c))


def test_crop_tiles_that_may_read_nothing_are_zeros():
    """a bad sample descriptor (an extent of 0, an offset past the pool, a negative offset, a sample that leaves the pool), a
    sample index at or past n_samples and an origin outside the source: zero tiles, and their neighbours are untouched"""
    shapes = [(17, 16), (5, 40), (16, 16), (33, 70), (40, 56), (5, 40)]
    samples = TC.sources(shapes, 3)
    r = Ragged(samples)
    desc = r.desc_host.copy()
    desc[1, 2] = 0                                           # H = 0
    desc[2:3].view(np.int64)[0, 0] = r.bytes                 # offset past the pool
    desc[3:4].view(np.int64)[0, 0] = -1                      # negative offset
    desc[5:6].view(np.int64)[0, 0] = r.bytes - 5 * 40 * 3 + 1      # the last byte lies outside
    tiles = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [3, 1, 38, 0], [4, 8, 24, 0], [5, 0, 0, 0], [6, 0, 0, 0], [2 ** 31 - 1, 0, 0, 0],
                        [0, 17, 0, 0], [0, 0, 16, 0], [4, -1, 0, 0], [4, 0, -2 ** 31, 0], [4, 2 ** 31 - 1, 0, 0], [0, 16, 15, 0]], np.int32)
    good = {0, 4, 13}
    exp = np.stack([TC.crop(samples[s], y0, x0, 16, 16) if t in good else np.zeros((16, 16, 3), np.uint8) for t, (s, y0, x0, _) in enumerate(tiles)])
    assert_tiles_equal(crop(r, dev(desc), tiles, 16, 16), exp, "bad descriptors")


# -- 2. the fused staging launch = crop + stage, bit for bit -------------------------------------------------------------------
def _image_bits(pl):
    torch.cuda.synchronize()
    host = pl.image().cpu().contiguous()
    return host.view(torch.int32 if pl.dtype == L.F32 else torch.int16).numpy()


def _image_region_only(pl):
    off = L.lib().nunet_plan_image(pl.handle, None, None)
    size = pl.n * pl.h * pl.w * 32 * (4 if pl.dtype == L.F32 else 2)
    assert off >= 0 and off + size <= pl.arena_bytes
    assert bool((pl.arena[:off] == FILL).all()) and bool((pl.arena[off + size:] == FILL).all()), "the staging launch wrote outside the image"


@pytest.mark.parametrize("case", [(16, 16, 4), (32, 32, 8), (16, 32, 8)], ids=lambda c: "%dx%d-o%d" % c)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stage_u8_tiles_equals_crop_then_stage(kind, case):
    th, tw, o = case
    samples = TC.sources(TC.SRC_SHAPES, 3)
    r = Ragged(samples)
    desc = r.desc_host.copy()
    desc[2, 3] = 0                                           # sample 2 (16 x 16) has a bad descriptor: its tiles stage the byte 0
    tiles = np.concatenate([TC.tables(TC.SRC_SHAPES, th, tw, o, 1)[0], NULL_TILE, np.asarray([[len(samples), 0, 0, 0]], np.int32)])
    n = tiles.shape[0]
    pl = Plan(n, th, tw, 3, 1, True, KINDS[kind], False, DEV, depth=1)         # pruned to depth 1: the full plan's image, a small arena
    d_desc, d_tiles, m, s = dev(desc), dev(tiles), dev(MEAN3), dev(STD3)
    pl.arena.fill_(FILL)
    L.check(L.lib().nunet_plan_stage_u8_tiles(pl.handle, L.ptr(r.pool), r.bytes, L.ptr(d_desc), r.n, L.ptr(d_tiles), L.ptr(m), L.ptr(s), 1.0 / 255.0,
                                              L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()), "nunet_plan_stage_u8_tiles")
    fused = _image_bits(pl)
    _image_region_only(pl)
    u8 = crop(r, d_desc, tiles, th, tw)
    pl.arena.fill_(FILL)
    L.check(L.lib().nunet_plan_stage_u8(pl.handle, L.ptr(u8), L.ptr(m), L.ptr(s), None, 1.0 / 255.0, L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()),
            "nunet_plan_stage_u8")
    two = _image_bits(pl)
    assert np.array_equal(fused, two), (kind, case)
    assert not fused[..., 3:].any(), "padding channels are zero bits"
    # and against the oracle's bytes through the existing staging entry
    exp = oracle_crops(samples, np.asarray([t if t[0] not in (2, len(samples)) else (-1, 0, 0, 0) for t in tiles.tolist()], np.int32), th, tw)
    pl.arena.fill_(FILL)
    L.check(L.lib().nunet_plan_stage_u8(pl.handle, L.ptr(dev(exp)), L.ptr(m), L.ptr(s), None, 1.0 / 255.0, L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()),
            "nunet_plan_stage_u8")
    assert np.array_equal(fused, _image_bits(pl))


# -- 2b. past the pipeline's grid cap (4096 workgroups x 256 threads, one thread per tile pixel) ----------------------------------
def test_capped_grid_crop_tiles_u8():
    """5 tiles of 460 x 457 = 1,051,100 pixels against the 1,048,576 the grid holds: the last 2,524 pixels are a thread's second
    trip, which ends inside a block. Every source is smaller than the tile, so the reflection turns many times along both axes;
    tile 2 is null and tile 4's origin lies outside its source."""
    n, th, tw = PC.LARGE_SHAPES["free"]
    assert n * th * tw > PC.GRID_CAP_PIXELS and (n * th * tw) % 256
    samples = TC.sources([(33, 70), (1, 1), (17, 16)], 3)
    tiles = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [-1, 0, 0, 0], [2, 16, 15, 0], [0, 33, 0, 0]], np.int32)
    exp = oracle_crops(samples, np.concatenate([tiles[:4], NULL_TILE]), th, tw)
    r = Ragged(samples)
    assert_tiles_equal(crop(r, r.desc, tiles, th, tw), exp, "crop 5x460x457")


def test_capped_grid_stage_u8_tiles():
    """the plan of test_input_pipeline_gpu's capped-grid staging case (N = 5, 464 x 464, bf16, pruned to depth 1): 1,076,480
    pixels, 27,904 of them a second trip. Five windows of two small sources; the staged image decodes to the oracle's crop
    (NULL mean / std, post_scale = 1) and the padding channels of every pixel are zero bits."""
    n, h, w = PC.LARGE_SHAPES["plan"]
    assert n * h * w > PC.GRID_CAP_PIXELS
    samples = TC.sources([(40, 56), (17, 16)], 3)
    tiles = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [0, 39, 55, 0], [1, 5, 9, 0], [0, 8, 24, 0]], np.int32)
    r = Ragged(samples)
    pl = Plan(n, h, w, 3, 1, True, L.BF16, False, DEV, depth=1)
    L.check(L.lib().nunet_plan_stage_u8_tiles(pl.handle, L.ptr(r.pool), r.bytes, L.ptr(r.desc), r.n, L.ptr(dev(tiles)), None, None, 1.0,
                                              L.ptr(pl.arena), L.nbytes(pl.arena), L.stream()), "nunet_plan_stage_u8_tiles")
    torch.cuda.synchronize()
    host = pl.image().cpu().contiguous()
    assert tuple(host.shape) == (n, h, w, 32)
    got = PC.decode_bytes(host.float().numpy()[..., :3], "bf16")
    assert_tiles_equal(got, oracle_crops(samples, tiles, h, w).astype(got.dtype), "stage_u8_tiles 5x464x464")
    assert not host.view(torch.int16).numpy()[..., 3:].any(), "padding channels are zero bits"


# -- 3. nunet_stitch_tiles against the fp64 oracle ------------------------------------------------------------------------------
def shape_desc(shapes):
    """descriptors that carry the extents only (the stitch reads no pool)"""
    d = np.zeros((len(shapes), 4), np.int32)
    d[:, 2:4] = np.asarray(shapes, np.int32)
    return d


def stitch(logits_dev, desc, grids, out_elems, kind, want_logits=True, want_u8=True, fill=7):
    nt, k, th, tw = logits_dev.shape
    lo = torch.full((out_elems,), float(fill), dtype=torch.float32, device=DEV) if want_logits else None
    u8 = torch.full((out_elems,), fill, dtype=torch.uint8, device=DEV) if want_u8 else None
    L.check(L.lib().nunet_stitch_tiles(L.ptr(logits_dev), nt, k, th, tw, L.ptr(dev(desc)), L.ptr(dev(grids)), desc.shape[0], T.WINDOWS[kind],
                                       L.ptr(sigmoid_u8_thresholds(torch.device(DEV))), L.ptr(lo), L.ptr(u8), out_elems, L.stream()), "nunet_stitch_tiles")
    torch.cuda.synchronize()
    return lo, u8


def sigmoid_u8_of(flat):
    out = torch.empty(flat.numel(), dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_sigmoid_u8(L.ptr(flat), L.ptr(sigmoid_u8_thresholds(flat.device)), L.ptr(out), flat.numel(), L.stream()), "sigmoid_u8")
    return out


def in_blocks(grids, shapes, K, out_elems):
    """bool [out_elems]: the elements that belong to a sample's [K][H][W] block (blocks start at multiples of 4 elements)"""
    m = np.zeros(out_elems, bool)
    for off, (h, w) in zip(grids.view(np.int64)[:, 0], shapes):
        m[off:off + K * h * w] = True
    return m


def check_stitch(got, logits, tiles, grids, shapes, K, kind, what):
    """got: flat fp32 host array; every sample's block against the fp64 blend, single-cover pixels bit for bit"""
    tol = TC.logit_tolerance(logits)
    offs = grids.view(np.int64)[:, 0]
    worst = 0.0
    for n, (h, w) in enumerate(shapes):
        blk = got[offs[n]:offs[n] + K * h * w].reshape(K, h, w)
        exp, cover = TC.stitch(logits, tiles, n, h, w, kind)
        err = float(np.abs(blk.astype(np.float64) - exp).max())
        worst = max(worst, err)
        assert err <= tol, "%s: sample %d (%d x %d): max error %.3g > %.3g" % (what, n, h, w, err, tol)
        m = np.broadcast_to(cover == 1, blk.shape)
        one = TC.single_cover_values(logits, tiles, n, h, w)
        assert np.array_equal(blk[m].view(np.int32), one[m].view(np.int32)), "%s: sample %d: a single-cover pixel is not its tile's logit" % (what, n)
    print("%s: max error %.3g, tolerance %.3g" % (what, worst, tol))


@pytest.mark.parametrize("kind", [TC.TENT, TC.UNIFORM])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("case", TC.TILE_CASES, ids=TC.TILE_IDS)
def test_stitch_tiles_equals_the_fp64_blend(case, K, kind):
    th, tw, o = case
    shapes = TC.SRC_SHAPES
    tiles, grids, n = TC.tables(shapes, th, tw, o, K)
    logits = np.random.default_rng(th + 7 * o + K).uniform(-8, 8, (tiles.shape[0], K, th, tw)).astype(np.float32)
    ld, desc = dev(logits), shape_desc(shapes)
    lo, u8 = stitch(ld, desc, grids, n, kind)
    check_stitch(lo.cpu().numpy(), logits, tiles, grids, shapes, K, kind, "stitch %s K=%d %s" % (case, K, kind))
    inside = dev(in_blocks(grids, shapes, K, n))
    assert torch.equal(u8[inside], sigmoid_u8_of(lo)[inside]), "out_u8 is nunet_sigmoid_u8 of the kernel's own logits"
    assert bool((lo[~inside] == 7).all()) and bool((u8[~inside] == 7).all()), "the elements between the samples' blocks were written"
    lo2, u82 = stitch(ld, desc, grids, n, kind)
    assert torch.equal(lo.view(torch.int32), lo2.view(torch.int32)) and torch.equal(u8, u82), "two runs differ"
    only_lo = stitch(ld, desc, grids, n, kind, want_u8=False)[0]
    only_u8 = stitch(ld, desc, grids, n, kind, want_logits=False)[1]
    assert torch.equal(only_lo.view(torch.int32), lo.view(torch.int32)) and torch.equal(only_u8, u8)


def test_stitch_source_of_the_tiles_size_is_the_networks_output():
    tiles, grids, n = TC.tables([(16, 32), (16, 32)], 16, 32, 8, 2)
    logits = np.random.default_rng(1).uniform(-8, 8, (2, 2, 16, 32)).astype(np.float32)
    lo, _ = stitch(dev(logits), shape_desc([(16, 32)] * 2), grids, n, TC.TENT)
    assert np.array_equal(lo.cpu().numpy().view(np.int32), logits.reshape(-1).view(np.int32))


def test_stitch_bad_grids_write_zeros_for_their_sample_only():
    th, tw, o, K = 16, 16, 4, 2
    shapes = [(33, 70), (17, 16), (5, 40), (40, 56), (16, 16), (17, 16), (1, 1)]
    tiles, grids, n = TC.tables(shapes, th, tw, o, K)
    nt = tiles.shape[0]
    logits = np.random.default_rng(2).uniform(-8, 8, (nt, K, th, tw)).astype(np.float32)
    ld, desc = dev(logits), shape_desc(shapes)
    good_lo, good_u8 = (v.cpu().numpy() for v in stitch(ld, desc, grids, n, TC.TENT))
    bad = grids.copy()
    bad[0, 3] = 0                      # ny < 1
    bad[1, 5] = 0                      # stride_y < 1
    bad[2, 2] = nt                     # tiles past the store
    bad[3, 2] = -1                     # tiles before the store
    bad[4, 4] = 2 ** 31 - 1            # nx such that ny * nx leaves the store (and would overflow 32 bits with a larger ny)
    d2 = desc.copy()
    d2[6, 2] = 0                       # a sample without extents writes nothing
    lo, u8 = (v.cpu().numpy() for v in stitch(ld, d2, bad, n, TC.TENT))
    offs = grids.view(np.int64)[:, 0]
    for i, (h, w) in enumerate(shapes):
        a, b = offs[i], offs[i] + K * h * w
        if i < 5:
            assert not lo[a:b].any() and not u8[a:b].any(), "sample %d: a bad grid writes zeros" % i
        elif i == 6:
            assert (lo[a:b] == 7).all() and (u8[a:b] == 7).all(), "a sample without extents writes nothing"
        else:
            assert np.array_equal(lo[a:b].view(np.int32), good_lo[a:b].view(np.int32)) and np.array_equal(u8[a:b], good_u8[a:b])
    # an output block that leaves 0 .. out_elems is not written (the guard bands around `lo` and `u8` would show it)
    bad = grids.copy()
    bad.view(np.int64)[5, 0] = n - 3
    bad.view(np.int64)[6, 0] = -1
    lo, u8 = (v.cpu().numpy() for v in stitch(ld, desc, bad, n, TC.TENT))
    a, b = offs[5], offs[5] + K * 17 * 16
    assert (lo[a:b] == 7).all() and (lo[offs[6]:] == 7).all()
    assert np.array_equal(lo[:a].view(np.int32), good_lo[:a].view(np.int32))


@pytest.fixture(scope="module")
def large():
    (h, w), K, (th, tw, o) = TC.LARGE_SHAPE, TC.LARGE_K, TC.LARGE_TILE
    assert K * h * w > TC.STITCH_GRID_THREADS
    tiles, grids, n = TC.tables([(h, w)], th, tw, o, K)
    logits = np.random.default_rng(9).uniform(-8, 8, (tiles.shape[0], K, th, tw)).astype(np.float32)
    return tiles, grids, n, logits


def test_capped_grid_stitch(large):
    tiles, grids, n, logits = large
    lo, u8 = stitch(dev(logits), shape_desc([TC.LARGE_SHAPE]), grids, n, TC.TENT)
    check_stitch(lo.cpu().numpy(), logits, tiles, grids, [TC.LARGE_SHAPE], TC.LARGE_K, TC.TENT, "stitch 3x420x421")
    assert torch.equal(u8, sigmoid_u8_of(lo))


# -- 4. the whole path ------------------------------------------------------------------------------------------------------------
TILE, NB = 32, 2


@functools.lru_cache(maxsize=None)
def _model(ds=False, dtype="fp32", ncls=1):
    """closed-form weights, non-fresh BatchNorm statistics; shared between the tests below - do not write to it"""
    st = nunet_amd.synth.closed_form_state(ncls, 3, ds, False)
    m = nunet_amd.archs.NestedUNet(ncls, 3, ds, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


def _full_batches(u8_tiles, n):
    """[n_tiles,Th,Tw,C] bytes -> batches of n, the last one filled with zero bytes (what null tiles stage)"""
    pad = (-u8_tiles.shape[0]) % n
    full = np.concatenate([u8_tiles, np.zeros((pad,) + u8_tiles.shape[1:], np.uint8)])
    return [full[k:k + n] for k in range(0, full.shape[0], n)]


def _eval_step_logits(ev, u8_tiles):
    """the last-head logits EvalStep gives for the same bytes, in full batches of its N"""
    out = []
    ev.begin()
    for b in _full_batches(u8_tiles, ev.n):
        ev.step(D.preprocess_images(dev(b)), torch.zeros((ev.n, ev.ncls, ev.h, ev.w), dtype=torch.float32, device=DEV))
        out.append(ev.last_logits.clone())
    return torch.cat(out)[:u8_tiles.shape[0]]


def _sources(shapes, seed):
    return RC.sources(shapes, 3, seed)


def _masks(shapes, seed):
    return RC.binary_sources(shapes, 1, seed)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sources_of_the_tiles_size_give_eval_steps_logits(dtype):
    model = _model(False, dtype)
    imgs = _sources([(TILE, TILE)] * 3, 50)                       # 3 tiles in batches of 2: the second replay carries a null tile
    tp = T.TiledPredictor(model, (NB, 3, TILE, TILE), source_capacity=3 * TILE * TILE * 3)
    r = tp.predict(*D.pack_ragged(imgs))
    assert tp.graph is not None and r["tiles"] == [1, 1, 1]
    ev = EvalStep(model, (NB, 3, TILE, TILE))
    want = _eval_step_logits(ev, np.stack(imgs))
    for i in range(3):
        assert tuple(r["logits"][i].shape) == (1, TILE, TILE) and r["masks"][i].dtype == torch.uint8
        assert torch.equal(r["logits"][i].view(torch.int32), want[i].view(torch.int32)), "image %d" % i
        assert torch.equal(r["masks"][i], sigmoid_masks_u8(want[i:i + 1])[0])


RAGGED = [(33, 70), (5, 40), (40, 56), (1, 1)]                   # 6 + 2 + 4 + 1 = 13 tiles of 32 x 32, overlap 8: not a multiple of 2
RAGGED2 = [(70, 33), (32, 32), (17, 16)]                          # 6 + 1 + 1 tiles


def _oracle_predict(model, imgs, overlap, kind):
    """oracle crop -> the module's eval forward on the same full batches -> the fp64 stitch: (per image fp64 blend, cover,
    fp32 single-cover values, the tile logits)"""
    shapes = [im.shape[:2] for im in imgs]
    K = model.num_classes
    tiles, grids, _ = TC.tables(shapes, TILE, TILE, overlap, K)
    u8 = oracle_crops(imgs, tiles, TILE, TILE)
    with torch.no_grad():
        out = []
        for b in _full_batches(u8, NB):
            y = model(D.preprocess_images(dev(b)))
            out.append((y[-1] if isinstance(y, list) else y).clone())
    logits = torch.cat(out)[:tiles.shape[0]].cpu().numpy()
    res = []
    for n, (h, w) in enumerate(shapes):
        blend, cover = TC.stitch(logits, tiles, n, h, w, kind)
        res.append((blend, cover, TC.single_cover_values(logits, tiles, n, h, w)))
    return res, logits


def _check_against_oracle(r, oracle, logits, what):
    tol = TC.logit_tolerance(logits)
    for i, (blend, cover, one) in enumerate(oracle):
        got = r["logits"][i].cpu().numpy()
        assert got.shape == blend.shape
        err = float(np.abs(got.astype(np.float64) - blend).max())
        print("%s image %d: max error %.3g, tolerance %.3g" % (what, i, err, tol))
        assert err <= tol, (what, i, err, tol)
        m = np.broadcast_to(cover == 1, got.shape)
        assert np.array_equal(got[m].view(np.int32), one[m].view(np.int32)), (what, i)
        assert torch.equal(r["masks"][i], sigmoid_masks_u8(r["logits"][i][None].contiguous())[0])


@pytest.mark.parametrize("kind", [TC.TENT, TC.UNIFORM])
def test_ragged_sources_against_the_oracle_path(kind):
    model = _model()
    imgs = _sources(RAGGED, 60)
    tp = T.TiledPredictor(model, (NB, 3, TILE, TILE), window=kind, source_capacity=1 << 16)
    r = tp.predict(*D.pack_ragged(imgs))
    assert r["tiles"] == [6, 2, 4, 1] and tp.overlap == 8
    oracle, logits = _oracle_predict(model, imgs, 8, kind)
    _check_against_oracle(r, oracle, logits, "ragged %s" % kind)


def test_graph_and_eager_agree_and_the_graph_replays_with_new_sizes():
    model = _model()
    imgs, imgs2 = _sources(RAGGED, 60), _sources(RAGGED2, 70)
    g = T.TiledPredictor(model, (NB, 3, TILE, TILE), overlap=4, source_capacity=1 << 16)
    e = T.TiledPredictor(model, (NB, 3, TILE, TILE), overlap=4, source_capacity=1 << 16, use_graph=False)
    rg, re = g.predict(*D.pack_ragged(imgs)), e.predict(*D.pack_ragged(imgs))
    assert g.graph is not None and e.graph is None
    for a, b in zip(rg["logits"] + rg["masks"], re["logits"] + re["masks"]):
        assert torch.equal(a, b)
    graph = g.graph
    r2 = g.predict(*D.pack_ragged(imgs2))
    assert g.graph is graph, "one captured graph serves every predict"
    oracle, logits = _oracle_predict(model, imgs2, 4, TC.TENT)
    _check_against_oracle(r2, oracle, logits, "second predict on the captured graph")
    for a, b in zip(r2["logits"], e.predict(*D.pack_ragged(imgs2))["logits"]):
        assert torch.equal(a, b)


def test_counts_equal_numpy_counts():
    model = _model(False, "fp32", 1)
    imgs, masks = _sources(RAGGED, 60), _masks(RAGGED, 60)
    tp = T.TiledPredictor(model, (NB, 3, TILE, TILE), source_capacity=1 << 16)
    r = tp.predict(*(D.pack_ragged(imgs) + D.pack_ragged(masks)))
    thr = np.float32(iou_logit_threshold())
    tot = dict(tp=0, fp=0, fn=0, tn=0)
    for i, m in enumerate(masks):
        a = r["logits"][i].cpu().numpy() >= thr
        b = m.transpose(2, 0, 1) > 127
        c = dict(tp=int((a & b).sum()), fp=int((a & ~b).sum()), fn=int((~a & b).sum()), tn=int((~a & ~b).sum()))
        for k in tot:
            tot[k] += c[k]
        assert r["iou"][i] == (c["tp"] + 1e-5) / (c["tp"] + c["fp"] + c["fn"] + 1e-5), i
        assert r["acc"][i] == (c["tp"] + c["tn"]) / float(a.size), i
        p = 1.0 / (1.0 + np.exp(-r["logits"][i].cpu().numpy().astype(np.float64)))
        dice = (2.0 * (p * b).sum() + 1e-5) / (p.sum() + b.sum() + 1e-5)
        assert abs(r["dice"][i] - dice) <= 1e-6, (i, r["dice"][i], dice)
    assert {k: v[0] for k, v in r["counts"].items()} == tot
    assert sum(tot.values()) == sum(h * w for h, w in RAGGED)
    assert repr(r["per_class"]) == repr(nunet_amd.metrics.scores_from_counts(*([tot[k]] for k in ("tp", "fp", "fn", "tn"))))
    assert "iou" not in tp.predict(*D.pack_ragged(imgs))


def test_deep_supervision_depth_and_weights():
    model = _model(True)
    imgs = _sources([(TILE, TILE)] * 2, 80)
    u8 = np.stack(imgs)
    cap = u8.size
    # the last head of the whole network is the one stitched
    r = T.TiledPredictor(model, (NB, 3, TILE, TILE), source_capacity=cap).predict(*D.pack_ragged(imgs))
    want = _eval_step_logits(EvalStep(model, (NB, 3, TILE, TILE)), u8)
    assert all(torch.equal(r["logits"][i].view(torch.int32), want[i].view(torch.int32)) for i in range(2))
    tp = T.TiledPredictor(model, (NB, 3, TILE, TILE), source_capacity=cap, depth=2)
    assert tp.heads == 1 and tp.pl.depth == 2
    r = tp.predict(*D.pack_ragged(imgs))
    want2 = _eval_step_logits(EvalStep(model, (NB, 3, TILE, TILE), depth=2), u8)
    assert all(torch.equal(r["logits"][i].view(torch.int32), want2[i].view(torch.int32)) for i in range(2))
    assert not torch.equal(want, want2)
    eng = model.engine()
    g = torch.Generator().manual_seed(4)
    fp = (eng.flat_params.cpu() * (1.0 + 0.05 * torch.randn(eng.flat_params.numel(), generator=g))).to(DEV)
    bb = (eng.bnbuf.cpu() * (1.0 + 0.05 * torch.rand(eng.bnbuf.numel(), generator=g))).to(DEV)
    r = T.TiledPredictor(model, (NB, 3, TILE, TILE), source_capacity=cap, weights=(fp, bb)).predict(*D.pack_ragged(imgs))
    want3 = _eval_step_logits(EvalStep(model, (NB, 3, TILE, TILE), weights=(fp, bb)), u8)
    assert all(torch.equal(r["logits"][i].view(torch.int32), want3[i].view(torch.int32)) for i in range(2))
    assert not torch.equal(want, want3)


def test_val_py_full_res_writes_masks_of_the_sources_sizes(tmp_path):
    """val.py --full_res true as a child process on a hand-written checkpoint (closed-form weights, no training run) of a
    --source_size 40,120 configuration: one mask per validation image, each of its source's size, the three means and the
    per-class table on stdout; without a ragged configuration the flag is refused with one error line."""
    import os
    import subprocess
    import sys
    import yaml
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(name="tiled_e2e", arch="NestedUNet", num_classes=1, input_channels=3, deep_supervision=False, dtype="bf16", loss="BCEDiceLoss",
               dataset="synthetic_blobs", source_size="40,120", train_size=0, val_size=5, input_h=32, input_w=32, batch_size=4)
    os.makedirs(os.path.join(str(tmp_path), "models", "tiled_e2e"))
    with open(os.path.join(str(tmp_path), "models", "tiled_e2e", "config.yml"), "w") as f:
        yaml.dump(cfg, f)
    st = nunet_amd.synth.closed_form_state(1, 3, False, False)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, os.path.join(str(tmp_path), "models", "tiled_e2e", "model.pth"))
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, os.path.join(root, "val.py"), "--name", "tiled_e2e", "--full_res", "true", "--tile_overlap", "6"]
    v = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert v.returncode == 0, (v.stdout[-3000:], v.stderr[-3000:])
    lines = v.stdout.strip().split("\n")
    print("\n".join(lines[-8:]))
    assert sum(ln.startswith(p) for ln in lines for p in ("IoU: ", "Dice: ", "Acc: ")) == 3 and any(ln.startswith("micro ") for ln in lines)
    from train import ragged_sets
    want = [s[0].shape[:2] for s in ragged_sets(cfg)[1]]
    assert len(want) == 5 and len(set(want)) > 1
    out = os.path.join(str(tmp_path), "outputs", "tiled_e2e", "0")
    assert sorted(os.listdir(out)) == ["val_%04d.jpg" % i for i in range(5)]
    for i, (h, w) in enumerate(want):
        assert Image.open(os.path.join(out, "val_%04d.jpg" % i)).size == (w, h), i
    cfg2 = dict(cfg, name="tiled_e2e_dense", source_size=None)
    os.makedirs(os.path.join(str(tmp_path), "models", "tiled_e2e_dense"))
    with open(os.path.join(str(tmp_path), "models", "tiled_e2e_dense", "config.yml"), "w") as f:
        yaml.dump(cfg2, f)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, os.path.join(str(tmp_path), "models", "tiled_e2e_dense", "model.pth"))
    v2 = subprocess.run(cmd[:3] + ["tiled_e2e_dense"] + cmd[4:], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert v2.returncode == 2 and any(ln.startswith("error: --full_res") for ln in v2.stdout.split("\n")), (v2.stdout[-2000:], v2.stderr[-2000:])


def test_python_misuse_raises_before_any_launch():
    model = _model()
    shape = (NB, 3, TILE, TILE)
    with pytest.raises(L.NunetError, match="source_capacity"):
        T.TiledPredictor(model, shape)
    with pytest.raises(L.NunetError, match="channels"):
        T.TiledPredictor(model, (NB, 1, TILE, TILE), source_capacity=1024)
    with pytest.raises(L.NunetError, match="overlap"):
        T.TiledPredictor(model, shape, overlap=17, source_capacity=1024)
    with pytest.raises(L.NunetError, match="window"):
        T.TiledPredictor(model, shape, window="hann", source_capacity=1024)
    with pytest.raises(L.NunetError, match="deep_supervision"):
        T.TiledPredictor(model, shape, depth=2, source_capacity=1024)
    with pytest.raises(L.NunetError, match="weights"):
        T.TiledPredictor(model, shape, source_capacity=1024, weights=(model.engine().flat_params[:-1], model.engine().bnbuf))
    imgs, masks = _sources([(5, 40), (17, 16)], 90), _masks([(5, 40), (17, 16)], 90)
    pool, desc = D.pack_ragged(imgs)
    tp = T.TiledPredictor(model, shape, source_capacity=pool.numel(), use_graph=False)
    tp.pool.fill_(0x5A)
    with pytest.raises(L.NunetError, match="source_capacity"):
        tp.predict(torch.cat([pool, pool[:1]]), desc)
    with pytest.raises(L.NunetError, match="outside the pool"):
        tp.predict(pool[:-1], desc)
    with pytest.raises(L.NunetError, match="flat uint8"):
        tp.predict(pool.to(torch.int16), desc)
    with pytest.raises(L.NunetError, match="host"):
        tp.predict(pool, desc.to(DEV))
    mp, md = D.pack_ragged(masks)
    with pytest.raises(L.NunetError, match="both or neither"):
        tp.predict(pool, desc, mp)
    with pytest.raises(L.NunetError, match="int32"):
        tp.predict(pool, desc, *D.pack_ragged(masks[:1]))
    with pytest.raises(L.NunetError, match="sizes differ"):
        tp.predict(pool, desc, *D.pack_ragged(masks[::-1]))
    assert bool((tp.pool == 0x5A).all()), "a refused predict copied sources"
    # the C entries refuse what the host can see
    z = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert L.lib().nunet_stitch_tiles(L.ptr(z), 1, 1, 4, 4, L.ptr(z), L.ptr(z), 1, 0, None, None, None, 16, L.stream()) != 0
    assert L.lib().nunet_stitch_tiles(L.ptr(z), 1, 1, 4, 4, L.ptr(z), L.ptr(z), 1, 2, None, L.ptr(z), None, 16, L.stream()) != 0
    assert L.lib().nunet_stitch_tiles(L.ptr(z), 1, 1, 4, 4, L.ptr(z), L.ptr(z), 1, 0, None, None, L.ptr(z), 16, L.stream()) != 0
    assert L.lib().nunet_crop_tiles_u8(L.ptr(z), 64, L.ptr(z), 1, L.ptr(z), 1, 3, 0, 4, L.ptr(z), L.stream()) != 0
