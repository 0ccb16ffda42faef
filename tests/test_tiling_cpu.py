"""Host-only checks of the conv3x3 / wgrad launch geometry (include/nunet_diag.h: nunet_conv3x3_launch_info,
nunet_conv3x3_wgrad_launch_info). The queries run the tile policy, the tile chooser, the K-split and the persistent-grid
rules of the launch itself; the kernels index LDS tables and decode work items on the strength of the invariants
asserted here. No GPU: no pointer of a descriptor is dereferenced."""
import ctypes as C
import itertools
import os

import pytest

from nunet_amd import _lib as L

NS = (1, 2, 3, 5, 7, 16)
HWS = (1, 2, 3, 5, 6, 12, 16, 20, 24, 40, 96)
# tile -> (BM, BN, HPMAX, threads): ConvCfg of csrc/conv3x3.hip
TILES = {1: (128, 32, 192, 256), 2: (128, 64, 192, 256), 3: (256, 32, 384, 256), 4: (256, 64, 344, 256)}
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.lib()


def cdesc(dt, n, h, w, c0, c1, cout, tile=0):
    d = L.ConvDesc()
    d.dtype = dt; d.N = n; d.H = h; d.W = w
    d.C0 = c0; d.P0 = c0; d.C1 = c1; d.P1 = c1
    d.D0 = cout; d.Q0 = cout
    d.tile = tile
    return d


def cinfo(lib, d):
    o = L.ConvLaunchInfo()
    rc = lib.nunet_conv3x3_launch_info(C.byref(d), C.byref(o))
    assert rc == 0, lib.nunet_last_error()
    return o


def check_pixel_tiling(o, n, h, w, bm, hpmax, where):
    """what both kernels rely on: the tile fits the MFMA rows and the halo table, and the tiles cover the batch"""
    assert o.NI >= 1 and o.TH >= 1 and o.TW >= 1, where
    assert o.NI * o.TH * o.TW <= bm, where
    assert o.NI * (o.TH + 2) * (o.TW + 2) <= hpmax, where
    assert o.TH + 2 < 1024 and o.TW + 2 < 1024 and o.NI < 2048, where          # packed (ni << 20 | y << 10 | x) codes
    if o.SH == 0:
        if o.NI > 1:
            assert o.TH == h and o.TW == w, where
        assert o.tilesX * o.TW >= w and o.tilesY * o.TH >= h and o.tilesG * o.NI >= n, where
        assert (o.tilesX - 1) * o.TW < w and (o.tilesY - 1) * o.TH < h and (o.tilesG - 1) * o.NI < n, where   # no empty tile
    else:
        # stacked rows: one virtual image of N * (H + 1) rows, full-width tiles
        assert o.SH == h + 1 and o.TW == w and o.NI == 1 and o.tilesX == 1 and o.tilesG == 1, where
        assert o.tilesY * o.TH >= n * (h + 1) and (o.tilesY - 1) * o.TH < n * (h + 1), where
        assert n * (h + 1) < (1 << 20) and o.SH <= 4096, where                   # range of the multiply-high division


@pytest.mark.parametrize("n", NS)
def test_conv_tiling_invariants(lib, n):
    for h, w, tile in itertools.product(HWS, HWS, (1, 2, 3, 4)):
        cout = 128
        o = cinfo(lib, cdesc(L.BF16, n, h, w, 32, 0, cout, tile))
        where = (n, h, w, tile)
        bm, bn, hpmax, nt = TILES[tile]
        assert (o.tile, o.BM, o.BN, o.HPMAX, o.NT) == (tile, bm, bn, hpmax, nt), where     # tile = k forces config k
        check_pixel_tiling(o, n, h, w, bm, hpmax, where)
        assert o.nCoT * o.BN == cout, where
        assert o.S == 1 and o.nch == 1, where                                     # no workspace: never split
        assert o.items == o.nCoT * o.tilesX * o.tilesY * o.tilesG * o.S, where
        assert 1 <= o.grid <= o.items, where
        # the grid holds resident workgroups only, and no workgroup runs more rounds than that needs
        assert o.per_cu >= 1 and o.grid <= 256 * o.per_cu, where
        assert -(-o.items // o.grid) == -(-o.items // (256 * o.per_cu)), where


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16])
def test_conv_policy_choice_is_one_of_the_forced_configs(lib, dt):
    """tile = 0: the policy's choice is a config the descriptor could also have forced, with the same geometry; the pixel
    tiling does not depend on the storage type."""
    kc = 16 if dt == L.F32 else 32
    for n, h, w, cout in itertools.product((1, 3, 16), HWS, (1, 12, 24, 96), (32, 64, 96, 256)):
        o = cinfo(lib, cdesc(dt, n, h, w, 2 * kc, kc, cout, 0))
        assert 1 <= o.tile <= 4 and (o.tile in (1, 3) or cout % 64 == 0)
        assert o.nch == 3
        f = cinfo(lib, cdesc(dt, n, h, w, 2 * kc, kc, cout, o.tile))
        names = [k for k, _ in L.ConvLaunchInfo._fields_]
        assert [getattr(o, k) for k in names] == [getattr(f, k) for k in names], (n, h, w, cout)
        check_pixel_tiling(o, n, h, w, o.BM, o.HPMAX, (n, h, w, cout))


def test_conv_rejects_64_wide_tiles_without_64_output_channels(lib):
    o = L.ConvLaunchInfo()
    for cout in (32, 96, 160):
        for tile in (2, 4):
            assert lib.nunet_conv3x3_launch_info(C.byref(cdesc(L.BF16, 2, 12, 12, 32, 0, cout, tile)), C.byref(o)) == EINVAL
            assert b"tile" in lib.nunet_last_error()
        for tile in (0, 1, 3):
            assert lib.nunet_conv3x3_launch_info(C.byref(cdesc(L.BF16, 2, 12, 12, 32, 0, cout, tile)), C.byref(o)) == 0
    assert lib.nunet_conv3x3_launch_info(C.byref(cdesc(L.BF16, 2, 12, 12, 32, 0, 64, 5)), C.byref(o)) == EINVAL
    assert lib.nunet_conv3x3_launch_info(C.byref(cdesc(L.BF16, 2, 12, 12, 16, 0, 64, 1)), C.byref(o)) == EINVAL   # half a channel chunk
    assert lib.nunet_conv3x3_launch_info(C.byref(cdesc(L.BF16, 2, 12, 12, 32, 0, 64, 1)), None) == EINVAL


def test_conv_ksplit_geometry(lib):
    """With a workspace the grid-starved long-K shapes are split: S slices multiply the items, never more than half the
    channel chunks, never more slabs than the workspace holds. (The workspace is only compared with NULL by the query.)"""
    token = (C.c_float * 4)()
    addr = C.addressof(token)
    seen_uneven = False
    for tile, (n, h, w), (c0, c1), cout in itertools.product((1, 2, 3, 4), ((2, 12, 12), (1, 6, 6), (16, 6, 6), (3, 1, 1)),
                                                             ((256, 256), (224, 128), (96, 160), (64, 0), (1024, 0)), (128, 512)):
        d = cdesc(L.BF16, n, h, w, c0, c1, cout, tile)
        base = cinfo(lib, d)
        assert base.S == 1
        d.splitk_ws = addr
        npix = n * h * w
        for cap in (0, npix * cout, 3 * npix * cout + 5, 1 << 40):
            d.splitk_ws_floats = cap
            o = cinfo(lib, d)
            where = (tile, n, h, w, c0, c1, cout, cap)
            assert o.nch == (c0 + c1) // 32, where
            assert o.items == base.items * o.S and 1 <= o.grid <= o.items, where
            assert (o.tilesX, o.tilesY, o.tilesG, o.nCoT) == (base.tilesX, base.tilesY, base.tilesG, base.nCoT), where
            if o.S > 1:
                assert 2 * o.S <= o.nch and o.S * npix * cout <= cap, where     # every slice has >= 2 chunks, the slabs fit
                seen_uneven |= o.nch % o.S != 0
            if cap < 2 * npix * cout or o.nch < 8:
                assert o.S == 1, where
    assert seen_uneven


@pytest.mark.parametrize("n", NS)
def test_wgrad_tiling_invariants(lib, n):
    o = L.WgradLaunchInfo()
    for h, w in itertools.product(HWS, HWS):
        for (c0, c1, cout), shape, (target, max_slabs) in itertools.product(
                ((64, 32, 64), (32, 0, 32)), (0, 11, 21, 12), ((0, 0), (1, 0), (64, 0), (100000, 0), (100000, 3), (0, 1))):
            d = L.WgradDesc()
            d.dtype = L.BF16; d.N = n; d.H = h; d.W = w
            d.C0 = c0; d.P0 = c0; d.C1 = c1; d.P1 = c1; d.Cout = cout; d.PY = cout
            d.target_wgs = target; d.max_slabs = max_slabs; d.item_shape = shape
            assert lib.nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == 0, lib.nunet_last_error()
            where = (n, h, w, c0, c1, cout, shape, target, max_slabs)
            check_pixel_tiling(o, n, h, w, 128, 192, where)
            cin = c0 + c1
            a, b = (2, 1) if shape == 21 and cout % 64 == 0 else (1, 2) if shape == 12 and cin >= 64 else (1, 1)
            assert (o.A, o.B) == (a, b), where
            assert o.nMT == o.tilesX * o.tilesY * o.tilesG, where
            assert o.nCoT == -(-cout // (32 * a)) and o.nCiT == -(-cin // (32 * b)), where
            assert o.ksplit == lib.nunet_conv3x3_wgrad_slabs(C.byref(d)), where
            assert 1 <= o.ksplit <= min(o.nMT, max_slabs or o.nMT), where
            assert o.grid == o.nCoT * o.nCiT * o.ksplit, where
            if target == 1:
                assert o.ksplit == 1, where
            if target == 100000 and not max_slabs:
                assert o.ksplit == o.nMT, where


def test_wgrad_launch_info_rejects_what_the_launch_rejects(lib):
    o = L.WgradLaunchInfo()
    d = L.WgradDesc()
    d.dtype = L.BF16; d.N = 2; d.H = 12; d.W = 12; d.C0 = 32; d.P0 = 32; d.Cout = 32; d.PY = 32
    assert lib.nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == 0
    d.item_shape = 22
    assert lib.nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == EINVAL and b"item_shape" in lib.nunet_last_error()
    d.item_shape = 0; d.Cout = 48
    assert lib.nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == EINVAL
    d.Cout = 32
    assert lib.nunet_conv3x3_wgrad_launch_info(C.byref(d), None) == EINVAL
