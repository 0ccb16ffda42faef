"""The LDS-tiled upsample backward kernel against the gather kernel it replaces, raw bytes equal, and the XCD block map of
both upsample kernels at the grid sizes where it can go wrong.

upsample_bwd_kernel (csrc/elementwise.hip) stages the high-res window of a work item (image, band of <= 8 low-res rows, band
of <= 8 columns, slab of <= 4 sixteen-byte channel groups) in LDS and sums the same 25 clamped taps with the same weights in
the same order as upsample_bwd_gather_kernel, which reads them from memory: the results are the same bits, NaN included,
so the comparison needs no tolerance. nunet_upsample2x_bwd takes the tiled kernel from extent 4 up, nunet_upsample2x_bwd_gather
always the gather kernel. The fp64 parity of nunet_upsample2x_bwd itself, at every extent 1..130, is test_elementwise_gpu.py's.

Shapes: edge bands shorter than the tile (5 x 7, 13 x 9: bands of 5|7 and 7 + 6|5 + 4), one band per image (4 x 4, 6 x 6),
several (12 x 12: 6 + 6, 24 x 24: 8 + 8 + 8), one slab (C = EPV: a single channel group, C = 32), a ragged last slab
(C = 48: 4 + 2 groups in bf16 / fp16), many slabs (C = 512), several images."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from nunet_amd import _lib as L  # noqa: E402
from test_ops_gpu import tdt, DEV, DT  # noqa: E402
from test_elementwise_gpu import epv, upsample_inputs, upsample_ref, upsample_check  # noqa: E402


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


DTS = [L.F32, L.BF16, L.F16]
PAD = 8
BITS = {L.F32: torch.int32, L.BF16: torch.int16, L.F16: torch.int16}
SHAPES = [(1, 4, 4, 0), (2, 5, 7, 32), (3, 6, 10, 64), (2, 13, 9, 48), (2, 12, 12, 256), (1, 24, 24, 128), (1, 6, 6, 512)]   # C = 0: EPV


def info(dt, n, h, w, c, backward):
    out = L.UpsampleLaunchInfo()
    L.check(L.lib().nunet_upsample_launch_info(dt, n, h, w, c, backward, C.byref(out)), "launch_info")
    return out


def filled(shape, dt, seed, scale=1.0):
    """guarded device buffer of N(0, scale) values rounded to the storage type"""
    g = torch.Generator().manual_seed(seed)
    t = torch.empty(shape, dtype=tdt(dt), device=DEV)
    t.copy_((torch.randn(shape, generator=g) * scale).to(tdt(dt)))
    return t


def copy_of(t):
    u = torch.empty_like(t)
    u.copy_(t)
    return u


def bits(t, dt):
    return t.contiguous().view(BITS[dt])


def bwd_pair(dt, n, h, w, c, acc, pdy, pdx, off_dy=0, off_dx=0, poison=None, seed=5):
    """both kernels on the same dy and the same initial dx (channels [off, off + c) of buffers of pitch pdy / pdx); returns
    (initial dx buffer, dx after the tiled kernel, dx after the gather kernel)"""
    assert info(dt, n, h, w, c, 1).tiled == 1
    dy = filled((n, 2 * h, 2 * w, pdy), dt, seed)
    if poison:
        poison(dy[..., off_dy:off_dy + c])
    dx0 = filled((n, h, w, pdx), dt, seed + 1)
    es = dy.element_size()
    outs = []
    for fn in (L.lib().nunet_upsample2x_bwd, L.lib().nunet_upsample2x_bwd_gather):
        dx = copy_of(dx0)
        L.check(fn(dt, n, h, w, c, L.ptr(dy, off_dy * es), pdy, L.ptr(dx, off_dx * es), pdx, acc, L.stream()), "up bwd")
        outs.append(dx)
    return dx0, outs[0], outs[1]


def assert_same_bytes(dt, dx0, tiled, gather, c, off, what):
    """the slot: tiled == gather bit for bit; everything around it: what it was"""
    a, b, z = bits(tiled, dt), bits(gather, dt), bits(dx0, dt)
    nbad = int((a[..., off:off + c] != b[..., off:off + c]).sum())
    assert nbad == 0, "%s (%s): %d elements differ between the tiled and the gather kernel" % (what, DT[dt], nbad)
    for got in (a, b):
        assert torch.equal(got[..., :off], z[..., :off]) and torch.equal(got[..., off + c:], z[..., off + c:]), what + ": wrote outside its channels"


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dxC%s" % (s[0], s[1], s[2], s[3] or "epv"))
@pytest.mark.parametrize("dt", DTS, ids=[DT[d] for d in DTS])
def test_tiled_equals_gather(dt, shape, acc):
    """pitched dy and dx (PAD channels in front of and behind the C in use)"""
    n, h, w, c = shape
    c = c or epv(dt)
    P = c + 2 * PAD
    dx0, t, g = bwd_pair(dt, n, h, w, c, acc, P, P, PAD, PAD, seed=1000 * h + w + c)
    assert_same_bytes(dt, dx0, t, g, c, PAD, "tiled %s acc=%d" % (shape, acc))
    if not acc:
        assert not torch.equal(bits(t, dt)[..., PAD:PAD + c], bits(dx0, dt)[..., PAD:PAD + c])     # (it did write)


@pytest.mark.parametrize("dt", DTS, ids=[DT[d] for d in DTS])
def test_tiled_dense(dt):
    """PDY == PDX == C"""
    n, h, w, c = 2, 13, 9, 48
    for acc in (0, 1):
        dx0, t, g = bwd_pair(dt, n, h, w, c, acc, c, c)
        assert_same_bytes(dt, dx0, t, g, c, 0, "dense acc=%d" % acc)


@pytest.mark.parametrize("dt", DTS, ids=[DT[d] for d in DTS])
def test_tiled_writes_one_slot_of_four(dt):
    """slot 1 of a four-slot level buffer (PDX = 4 C), as the plan calls it: slots 0, 2, 3 keep their (random) contents, the
    guard bands around the buffer theirs (the autouse fixture)"""
    n, h, w, c = 3, 6, 10, 64
    for acc in (0, 1):
        dx0, t, g = bwd_pair(dt, n, h, w, c, acc, c, 4 * c, 0, c)
        assert_same_bytes(dt, dx0, t, g, c, c, "slot 1 of 4 acc=%d" % acc)


@pytest.mark.parametrize("dt", DTS, ids=[DT[d] for d in DTS])
def test_tiled_propagates_non_finite(dt):
    """an inf and a NaN at a corner pixel and at a last-row pixel of dy: the clamped, zero-weighted taps of the window turn
    them into NaN (0 * inf) exactly where the gather kernel does - the fp16 overflow check of the training step relies on
    non-finite gradients propagating - and all bytes, NaN payloads included, are equal"""
    n, h, w, c = 2, 13, 9, 48

    def poison(v):
        v[0, 0, 0, 0] = float("inf")
        v[0, 0, 0, 1] = float("nan")
        v[n - 1, 2 * h - 1, 5, 2] = float("-inf")
        v[n - 1, 2 * h - 1, 5, 3] = float("nan")
    P = c + 2 * PAD
    for acc in (0, 1):
        dx0, t, g = bwd_pair(dt, n, h, w, c, acc, P, P, PAD, PAD, poison=poison)
        assert_same_bytes(dt, dx0, t, g, c, PAD, "non-finite acc=%d" % acc)
        bad = ~torch.isfinite(t[..., PAD:PAD + c].float())
        assert bool(bad[0, 0, 0, 0]) and bool(bad[0, 0, 0, 1]) and bool(bad[n - 1, h - 1, 2, 2]) and bool(bad[n - 1, h - 1, 2, 3])
        assert torch.equal(bad, ~torch.isfinite(g[..., PAD:PAD + c].float()))
        assert not bool(bad[..., 4:].any())


# ---------------------------------------------------------------------------------------------------------------------
# launch shapes: grids that are no multiple of 8 (the remap's ragged XCD ranges), smaller than 8, and beyond one pass
# ---------------------------------------------------------------------------------------------------------------------
REGIMES = {"below8": lambda i: i.workgroups < 8 and i.passes == 1, "1mod8": lambda i: i.workgroups > 8 and i.workgroups % 8 == 1 and i.passes == 1,
           "7mod8": lambda i: i.workgroups > 8 and i.workgroups % 8 == 7 and i.passes == 1, "passes": lambda i: i.passes > 1 and i.items % i.workgroups != 0}
BWD_CANDIDATES = [(3, 8, 8, 32), (1, 24, 24, 32), (1, 24, 40, 32), (3, 50, 118, 512)]       # 3, 9, 15 items; 5040 items on 4096 workgroups
FWD_CANDIDATES = [(1, 4, 4, 64), (1, 6, 6, 128), (1, 6, 10, 128), (3, 50, 118, 128)]        # 2, 9, 15 blocks; 4425 blocks on 4096 workgroups


def pick(cands, regime, backward):
    for s in cands:
        i = info(L.BF16, *s, backward)
        if REGIMES[regime](i):
            return s, i
    raise AssertionError("no candidate shape reaches the launch regime %s" % regime)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_bwd_launch_regimes(regime):
    """bf16, dense; the tiled kernel's map (items over workgroups, xcd_remap, passes) against the gather kernel"""
    (n, h, w, c), i = pick(BWD_CANDIDATES, regime, 1)
    assert i.tiled == 1
    print("%s: %s -> %d items on %d workgroups, %d passes" % (regime, (n, h, w, c), i.items, i.workgroups, i.passes))
    dx0, t, g = bwd_pair(L.BF16, n, h, w, c, 1, c, c)
    assert_same_bytes(L.BF16, dx0, t, g, c, 0, "bwd regime " + regime)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_fwd_launch_regimes(regime):
    """bf16; the forward kernel's map (blocks of 256 outputs, xcd_remap, passes) against fp64 F.interpolate under the
    criterion of test_elementwise_gpu.py (its backward check rides along)"""
    (n, h, w, c), i = pick(FWD_CANDIDATES, regime, 0)
    assert i.tiled == 0
    print("%s: %s -> %d blocks on %d workgroups, %d passes" % (regime, (n, h, w, c), i.items, i.workgroups, i.passes))
    x, dy, prev = upsample_inputs(L.BF16, n, h, w, c, seed=31)
    upsample_check(L.BF16, x, dy, prev, upsample_ref(x, dy), "upsample_fwd " + regime, accs=(0,))
