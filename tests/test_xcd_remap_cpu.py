"""Host-only checks of the block -> work item map and of the upsample launch geometry (include/nunet_diag.h).

xcd_remap(b, G) (csrc/common.h) hands every XCD one contiguous range of the G work items of a launch: block b, which runs
on XCD b % 8 as the (b / 8)-th block that XCD receives, takes item base(b % 8) + b / 8. Any placement is correct as long as
the map is a bijection of [0, G): every item is taken exactly once. The conv, weight-gradient and upsample kernels all
call it with G = their grid, so every grid size they can launch (up to the 4096-block cap of the element-wise kernels) is
walked here, through nunet_xcd_remap_host, the same function compiled for the host."""
import ctypes as C
import itertools

import pytest

from nunet_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def test_xcd_remap_is_a_bijection_for_every_grid(lib):
    f = lib.nunet_xcd_remap_host
    for G in range(1, 4201):
        items = list(map(f, range(G), itertools.repeat(G)))
        assert sorted(items) == list(range(G)), "G=%d: an item is out of range, taken twice or never" % G


def test_xcd_remap_gives_each_xcd_a_contiguous_range(lib):
    """the blocks of one XCD (b % 8 equal) take consecutive items, and XCD x's range lies before XCD x + 1's"""
    f = lib.nunet_xcd_remap_host
    for G in (1, 7, 8, 9, 15, 576, 1151, 1152, 4095, 4096):
        end = 0
        for x in range(min(8, G)):
            items = [f(b, G) for b in range(x, G, 8)]
            assert items == list(range(end, end + len(items))), (G, x)
            end += len(items)
        assert end == G


def info(lib, dt, n, h, w, c, backward):
    out = L.UpsampleLaunchInfo()
    L.check(lib.nunet_upsample_launch_info(dt, n, h, w, c, backward, C.byref(out)), "launch_info")
    return out


def test_upsample_launch_geometry(lib):
    """Tiled backward from extent 4 up, the gather kernel below; at least two workgroups fit a CU's 160 KB of LDS; the deep
    levels of the flagship workload (batch 16: 12 x 12 x 256 and 6 x 6 x 512) still give every one of the 256 CUs a workgroup;
    ragged widths (C = EPV, C % (4 EPV) != 0) get their last slab; the forward pass counts blocks of 256 outputs."""
    for dt, epv in ((L.F32, 4), (L.BF16, 8), (L.F16, 8)):
        for h, w in ((1, 1), (3, 8), (8, 3), (3, 3)):
            i = info(lib, dt, 2, h, w, 4 * epv, 1)
            assert i.tiled == 0 and i.items == -(-2 * h * w * 4 // 256) and i.lds_bytes == 0
        for n, h, w, c in ((16, 48, 48, 64), (16, 24, 24, 128), (16, 12, 12, 256), (16, 6, 6, 512), (1, 4, 4, epv), (2, 13, 9, 6 * epv)):
            i = info(lib, dt, n, h, w, c, 1)
            g = c // epv
            assert i.tiled == 1 and 1 <= i.TR <= 8 and 1 <= i.TC <= 8 and 1 <= i.SG <= 4
            assert i.items == n * -(-h // i.TR) * -(-w // i.TC) * -(-g // i.SG)
            assert i.workgroups == min(i.items, 4096) and i.passes == -(-i.items // i.workgroups)
            assert 2 * i.lds_bytes <= 160 * 1024
            if n == 16:
                assert i.workgroups >= 256
        i = info(lib, dt, 3, 50, 118, 16 * epv, 0)
        assert i.tiled == 0 and i.items == 4425 and i.workgroups == 4096 and i.passes == 2
    out = L.UpsampleLaunchInfo()
    assert lib.nunet_upsample_launch_info(L.BF16, 1, 4, 4, 12, 1, C.byref(out)) != 0      # C % EPV != 0: refused like the launch
    assert lib.nunet_upsample_launch_info(L.BF16, 1, 4, 4, 8, 1, None) != 0
