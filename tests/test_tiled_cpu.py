"""Host side of the tiled inference (nunet_amd.tiled): the geometry against brute force and the numpy oracle of
tests/tile_cases.py, the tables TiledPredictor builds, the host checks. No GPU."""
import numpy as np
import pytest
import torch

import nunet_amd
from nunet_amd import _lib as L
from nunet_amd import tiled as T
import tile_cases as TC


def _sweep():
    for t in (16, 32, 48, 96):
        for o in range(0, t // 2 + 1):
            for s in range(1, 4 * t + 3):
                yield s, t, o


def test_origins_increase_end_flush_and_cover_at_most_three_times():
    for s, t, o in _sweep():
        og = T.tile_origins(s, t, o)
        assert og == TC.origins(s, t, o), (s, t, o)
        assert (len(og), t - o) == T.axis_grid(s, t, o)
        if s <= t:
            assert og == [0]
            continue
        assert og[0] == 0 and og[-1] == s - t, (s, t, o, og)
        assert all(b > a for a, b in zip(og, og[1:])), (s, t, o, og)
        assert og == [min(j * (t - o), s - t) for j in range(len(og))]
        cover = np.zeros(s, np.int64)
        for a in og:
            cover[a:a + t] += 1
        assert cover.min() >= 1 and cover.max() <= 3, (s, t, o, og, cover.max())


def test_reflection_is_np_pad_reflect_and_the_loop_definition():
    assert [T.reflect_index(i, 1) for i in range(40)] == [0] * 40
    assert [T.reflect_index(i, 2) for i in range(7)] == [0, 1, 0, 1, 0, 1, 0]
    for s in range(2, 20):
        for t in (16, 32):
            got = [T.reflect_index(i, s) for i in range(t)]
            assert got == [TC.reflect_loop(i, s) for i in range(t)], (s, t)
            # (np.pad(mode='reflect') repeats the reflection when the pad is longer than the axis, the same way)
            assert got == list(np.pad(np.arange(s), (0, max(t - s, 0)), mode="reflect")[:t]), (s, t)
    src = np.arange(5 * 3 * 2, dtype=np.uint8).reshape(5, 3, 2)
    assert np.array_equal(TC.crop(src, 0, 0, 16, 16), np.pad(src, ((0, 11), (0, 13), (0, 0)), mode="reflect"))


def test_blend_windows():
    assert list(T.blend_window(16)) == list(TC.window(16, TC.TENT)) == [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert list(T.blend_window(5, "tent")) == [1, 2, 3, 2, 1]
    assert list(T.blend_window(7, "uniform")) == [1] * 7
    with pytest.raises(L.NunetError, match="window"):
        T.blend_window(8, "hann")


@pytest.mark.parametrize("case", TC.TILE_CASES, ids=TC.TILE_IDS)
def test_host_tables_equal_the_oracles(case):
    th, tw, o = case
    for k in (1, 3):
        tiles, grids, n = T.build_tables(TC.SRC_SHAPES, (th, tw), o, k)
        et, eg, en = TC.tables(TC.SRC_SHAPES, th, tw, o, k)
        assert tiles.dtype == grids.dtype == np.int32
        assert np.array_equal(tiles, et) and np.array_equal(grids, eg) and n == en
        offs = list(grids.view(np.int64)[:, 0]) + [n]
        assert all(a % 4 == 0 and 0 <= b - a - k * h * w < 4 for a, b, (h, w) in zip(offs, offs[1:], TC.SRC_SHAPES))
        T.check_tiles(tiles, TC.SRC_SHAPES)
        T.check_grids(grids, TC.SRC_SHAPES, tiles.shape[0], (th, tw), k, n, tiles)
    bt, smap = T.batch_tables(tiles, 4)
    assert bt.shape == (-(-tiles.shape[0] // 4), 4, 4) and smap.shape == bt.shape[:2]
    flat = bt.reshape(-1, 4)
    assert (flat[tiles.shape[0]:, 0] == -1).all(), "the last batch is filled with null tiles"
    for b in range(bt.shape[0]):
        for r in range(4):
            t = b * 4 + r
            if t < tiles.shape[0]:
                assert smap[b, bt[b, r, 0]] == tiles[t, 0] and tuple(bt[b, r, 1:3]) == tuple(tiles[t, 1:3])
        used = smap[b][smap[b] >= 0]
        assert len(set(used)) == len(used)


def test_host_checks_raise():
    shapes = [(33, 70), (5, 40)]
    tiles, grids, n = T.build_tables(shapes, (16, 16), 4, 1)
    nt = tiles.shape[0]
    for bad in (9, -1, 2.0, True):
        with pytest.raises(L.NunetError, match="overlap"):
            T.check_overlap((16, 16), bad)
    with pytest.raises(L.NunetError, match="overlap"):
        T.build_tables(shapes, (16, 32), 9, 1)                 # half the SMALLER side
    assert T.check_overlap((16, 32), 8) == 8
    with pytest.raises(L.NunetError, match="outside the store"):
        T.check_grids(grids, shapes, nt - 1, (16, 16), 1, n)
    g = grids.copy(); g[0, 2] = -1
    with pytest.raises(L.NunetError, match="outside the store"):
        T.check_grids(g, shapes, nt, (16, 16), 1, n)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_grids(grids.astype(np.int64), shapes, nt, (16, 16), 1, n)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_grids(grids[:, :7], shapes, nt, (16, 16), 1, n)
    with pytest.raises(L.NunetError, match="entries for"):
        T.check_grids(grids[:1], shapes, nt, (16, 16), 1, n)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_tiles(tiles.astype(np.int16), shapes)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_tiles(tiles.reshape(-1), shapes)
    for col, val, what in ((3, 0, "positive"), (5, 0, "positive"), (5, 17, "stride_y"), (6, 7, "stride_x"), (3, 1, "flush"), (4, 99, "outside the store")):
        g = grids.copy(); g[0, col] = val
        with pytest.raises(L.NunetError, match=what):
            T.check_grids(g, shapes, nt, (16, 16), 1, n)
    g = grids.copy(); g.view(np.int64)[1, 0] = 0
    with pytest.raises(L.NunetError, match="overlap"):
        T.check_grids(g, shapes, nt, (16, 16), 1, n)
    with pytest.raises(L.NunetError, match="outside 0"):
        T.check_grids(grids, shapes, nt, (16, 16), 1, n - 1)
    t2 = tiles.copy(); t2[1, 2] += 1
    with pytest.raises(L.NunetError, match="not the grid's tiles"):
        T.check_grids(grids, shapes, nt, (16, 16), 1, n, t2)
    t2 = tiles.copy(); t2[0, 0] = 2
    with pytest.raises(L.NunetError, match="sample 2 of 2"):
        T.check_tiles(t2, shapes)
    t2 = tiles.copy(); t2[0, 1] = 33
    with pytest.raises(L.NunetError, match="outside its"):
        T.check_tiles(t2, shapes)


def test_source_group_checks_raise():
    imgs = TC.sources([(5, 40), (17, 16)], 3)
    pool, desc = nunet_amd.dataset.pack_ragged(imgs)
    T.check_source_group(pool, desc, 3, pool.numel())
    with pytest.raises(L.NunetError, match="source_capacity"):
        T.check_source_group(pool, desc, 3, pool.numel() - 1)
    with pytest.raises(L.NunetError, match="outside the pool"):
        T.check_source_group(pool, desc, 4, 1 << 20)              # a channel count the pool was not packed with
    with pytest.raises(L.NunetError, match="flat uint8"):
        T.check_source_group(pool.to(torch.int32), desc, 3, 1 << 20)
    with pytest.raises(L.NunetError, match="flat uint8"):
        T.check_source_group(pool.view(2, -1), desc, 3, 1 << 20)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_source_group(pool, desc.to(torch.int64), 3, 1 << 20)
    with pytest.raises(L.NunetError, match="int32"):
        T.check_source_group(pool, desc, 3, 1 << 20, n=3)
    bad = desc.clone(); bad[1, 2] = 0
    with pytest.raises(L.NunetError, match="extents"):
        T.check_source_group(pool, bad, 3, 1 << 20)


def test_stitch_oracle_single_cover_and_constant_tiles():
    g = np.random.default_rng(3)
    for (th, tw, o) in TC.TILE_CASES:
        tiles, grids, _ = TC.tables(TC.SRC_SHAPES, th, tw, o, 2)
        logits = g.uniform(-8, 8, (tiles.shape[0], 2, th, tw)).astype(np.float32)
        for n, (h, w) in enumerate(TC.SRC_SHAPES):
            for kind in (TC.TENT, TC.UNIFORM):
                blend, cover = TC.stitch(logits, tiles, n, h, w, kind)
                assert cover.max() <= 9
                one = TC.single_cover_values(logits, tiles, n, h, w)
                m = np.broadcast_to(cover == 1, blend.shape)
                assert np.array_equal(blend[m], one[m].astype(np.float64))
                const, _ = TC.stitch(np.full_like(logits, 1.25), tiles, n, h, w, kind)
                assert np.allclose(const, 1.25, rtol=0, atol=1e-15)
        if o == 0:
            assert all(TC.stitch(logits, tiles, n, h, w, TC.TENT)[1].max() <= 4 for n, (h, w) in enumerate(TC.SRC_SHAPES))
