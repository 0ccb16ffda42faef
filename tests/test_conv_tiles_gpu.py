"""conv3x3 / wgrad: every kernel instantiation and every loop regime of the real workload against torch fp64.

tests/test_ops_gpu.py launches the 128 x 32 conv tile with one work item per workgroup and the weight gradient with one
pixel tile per slice. Here the descriptor forces each of the four conv tiles (nunet_conv_desc.tile) and each wgrad
K-split (max_slabs), and every case first asserts - from the launch-geometry query of include/nunet_diag.h - that it
reaches the path it is about: a case that no longer does FAILS instead of passing vacuously.

The reference is always torch fp64 on the CPU on inputs rounded through the storage type; tolerances are those of
test_ops_gpu.py. Runs on the MI355X only."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nunet_amd import _lib as L  # noqa: E402
from test_ops_gpu import DEV, DT, TOL, conv_desc, nhwc, pack, q, rel_err, tdt, to_nchw, wgrad_desc, wgrad_run  # noqa: E402


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


DTS = [L.F32, L.BF16, L.F16]
TILES = [1, 2, 3, 4]
WTOL = {L.F32: 5e-5, L.BF16: 1e-3, L.F16: 1e-3}      # weight gradients (test_conv3x3_wgrad)
dt_id = DT.get


def conv_info(d):
    o = L.ConvLaunchInfo()
    L.check(L.lib().nunet_conv3x3_launch_info(C.byref(d), C.byref(o)), "conv launch info")
    return o


def wgrad_info(d):
    o = L.WgradLaunchInfo()
    L.check(L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)), "wgrad launch info")
    return o


def stat_words(stats):
    """integer sum of the replicas of a fixed-point statistics buffer: the exact totals, word for word"""
    return stats.view(L.BN_SUM_REPLICAS, -1).sum(0)


def check_stats(stats, stored, bias, m, cout):
    """BN partial sums are taken about the bias on the rounded outputs (as in test_conv3x3_fwd)"""
    dd = stored.double() - bias.double().view(1, -1, 1, 1)
    s = L.fx_decode(stats, cout)
    np.testing.assert_allclose(s[:cout].numpy() / m, dd.sum((0, 2, 3)).numpy() / m, atol=1e-4 * float(dd.abs().max()) + 1e-6)
    np.testing.assert_allclose(s[cout:].numpy() / m, (dd * dd).sum((0, 2, 3)).numpy() / m, rtol=1e-3, atol=1e-6)


def require_multi_item(d, tile):
    """The persistent loop's `nitem = item + grid` branch: workgroups run several items, and not all the same number."""
    o = conv_info(d)
    assert o.tile == tile and o.S == 1, (o.tile, o.S)
    assert o.items > o.grid and o.items % o.grid != 0, "not the multi-item regime: %d items on %d workgroups" % (o.items, o.grid)
    assert o.nCoT > 1 and o.grid % o.nCoT != 0, "a workgroup would stay on one Cout tile"
    return o


# ---------------------------------------------------------------------------------------------------------------------
# a. every tile against fp64 at the edge shapes
# ---------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [
    (2, 20, 24, 32, 0, 64),     # ragged tiles
    (1, 16, 16, 64, 64, 64),    # two sources
    (5, 6, 6, 32, 0, 64),       # several images per tile
    (3, 1, 1, 32, 0, 64),       # 1 x 1 images
    (16, 12, 12, 64, 32, 64),   # stacked-rows tiling
    (7, 3, 5, 32, 0, 64),       # odd tiny images
]


@functools.lru_cache(maxsize=None)
def _edge_case(dt, shape):
    n, h, w, c0, c1, cout = shape
    g = torch.Generator().manual_seed(100 + EDGE_SHAPES.index(shape))
    cin = c0 + c1
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(q(x, dt).double(), q(wt, dt).double(), b.double(), padding=1)
    return x, wt, b, ref


def _edge_run(dt, shape, tile):
    n, h, w, c0, c1, cout = shape
    x, wt, b, _ = _edge_case(dt, shape)
    s0 = nhwc(x[:, :c0], dt, pitch=c0 + 32, off=0)      # source 0 lives in a wider level buffer, source 1 is dense
    s1 = nhwc(x[:, c0:], dt) if c1 else None
    wf, _ = pack(wt, dt)
    y = torch.full((n, h, w, cout), 7.0, dtype=tdt(dt), device=DEV)
    stats = L.fx_zeros(cout, DEV)
    bg = b.to(DEV)
    d = conv_desc(dt, n, h, w, s0, c0, c0 + 32, wf, y, cout, cout, src1=s1, c1=c1, p1=c1, bias=bg, stats=stats)
    d.tile = tile
    o = conv_info(d)
    assert o.tile == tile and o.S == 1 and o.nCoT * o.BN == cout, (shape, tile, o.tile, o.S)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv")
    torch.cuda.synchronize()
    return y, stats, o


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("tile", TILES)
def test_every_tile_against_fp64_at_the_edge_shapes(tile, dt):
    """Each tile configuration against fp64, and bit for bit against the next one (1 = 2, 2 = 3, 3 = 4, 4 = 1: all four
    agree): without a K-split every output element is accumulated chunk -> tap -> k-step in all four configurations.
    The BatchNorm statistics are NOT the same words: a workgroup sums its tile's pixels in fp32 before the fixed-point add,
    and which pixels share a workgroup (and a lane) depends on the tile; they agree to that fp32 summation noise."""
    other = tile % 4 + 1
    seen = set()
    for shape in EDGE_SHAPES:
        n, h, w, c0, c1, cout = shape
        _, _, b, ref = _edge_case(dt, shape)
        y, stats, o = _edge_run(dt, shape, tile)
        y2, stats2, _ = _edge_run(dt, shape, other)
        seen |= {"stacked"} if o.SH else set()
        seen |= {"multi-image"} if o.NI > 1 else set()
        seen |= {"partial"} if o.NI * o.TH * o.TW < o.BM else set()          # MFMA rows without a pixel
        got = to_nchw(y, cout)
        assert rel_err(got, ref) < TOL[dt], (DT[dt], shape, tile)
        check_stats(stats, got, b, n * h * w, cout)
        assert torch.equal(y, y2), (DT[dt], shape, tile, other)
        # statistics of the two tiles: each is a sum of per-workgroup fp32 sums of at most 256 terms (error <= 255 * 2^-24 * sum |d|
        # per side, any summation order) of the SAME rounded outputs
        dd = got.double() - b.double().view(1, -1, 1, 1)
        s, s2 = L.fx_decode(stats, cout), L.fx_decode(stats2, cout)
        bound1 = 2 * 260 * 2.0 ** -24 * dd.abs().sum((0, 2, 3)) + 1e-12      # (260: 255 additions, the higher-order terms, the
        bound2 = 2 * 260 * 2.0 ** -24 * (dd * dd).sum((0, 2, 3)) + 1e-12     #  rounding of d and of its square)
        print("stats words of tiles %d / %d equal: %s  %s %s" % (tile, other, torch.equal(stat_words(stats), stat_words(stats2)), DT[dt], shape))
        assert bool(((s[:cout] - s2[:cout]).abs() <= bound1).all()), (DT[dt], shape, tile, other)
        assert bool(((s[cout:] - s2[cout:]).abs() <= bound2).all()), (DT[dt], shape, tile, other)
    assert seen == {"stacked", "multi-image", "partial"}, seen


# ---------------------------------------------------------------------------------------------------------------------
# b. / c. the persistent multi-item loop
# ---------------------------------------------------------------------------------------------------------------------
# The smallest batch found (by the geometry query, over N <= 6 and H, W multiples of 4) at which EVERY tile and every
# fused variant below has more items than workgroups and an uneven split of them: 15600 pixels x 512 output channels,
# 2080 / 1040 / 1040 / 560 items for tiles 1..4, ragged on both image axes. The preconditions are asserted per case.
MN, MH, MW, MCOUT = 5, 52, 60, 512
MPX = MN * MH * MW
MULTI_CASES = [(t, dt) for t in TILES for dt in (L.F32, L.BF16)] + [(2, L.F16), (4, L.F16)]
multi_id = lambda v: DT[v[1]] + "-tile%d" % v[0]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _multi_plain(dt):
    g = torch.Generator().manual_seed(51)
    x = torch.randn(MN, 64, MH, MW, generator=g)
    wt = torch.randn(MCOUT, 64, 3, 3, generator=g) / (3 * 64 ** 0.5)
    b = torch.randn(MCOUT, generator=g) * 0.1
    prev = torch.randn(MN, 256, MH, MW, generator=g)
    ref = F.conv2d(q(x, dt).double(), q(wt, dt).double(), b.double(), padding=1)
    return x, wt, b, prev, ref


@pytest.mark.parametrize("case", MULTI_CASES, ids=multi_id)
def test_multi_item_loop_plain(case):
    """Workgroups that decode, prefetch and run a second and third item (other pixel tile, other Cout tile): bias, statistics,
    two sources, two destinations with a slot-wise accumulate mask."""
    tile, dt = case
    x, wt, b, prev, ref = _multi_plain(dt)
    s0 = nhwc(x[:, :32], dt, pitch=64)
    s1 = nhwc(x[:, 32:], dt)
    wf, _ = pack(wt, dt)
    d0 = nhwc(prev, dt, pitch=320)                       # 4 slots of 64 and one spare slot
    d1 = torch.full((MN, MH, MW, 256), 7.0, dtype=tdt(dt), device=DEV)
    stats = L.fx_zeros(MCOUT, DEV)
    bg = b.to(DEV)
    d = conv_desc(dt, MN, MH, MW, s0, 32, 64, wf, d0, 256, 320, src1=s1, c1=32, p1=32, bias=bg,
                  dst1=d1, d1=256, q1=256, slot_w=64, mask=0b0110, stats=stats)
    d.tile = tile
    require_multi_item(d, tile)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv")
    torch.cuda.synchronize()
    exp0 = ref[:, :256].clone()
    exp0[:, 64:192] += q(prev, dt)[:, 64:192].double()   # slots 1 and 2 accumulate, 0 and 3 overwrite
    got0, got1 = to_nchw(d0, 256), to_nchw(d1, 256)
    assert rel_err(got0, exp0) < TOL[dt]
    assert rel_err(got1, ref[:, 256:]) < TOL[dt]
    assert float(d0[..., 256:].float().abs().max()) == 0.0          # the spare slot is untouched
    # the statistics are those of conv + bias as rounded to the storage type, BEFORE a slot accumulates
    stored = torch.cat([got0, got1], 1)
    stored[:, 64:192] = q(ref[:, 64:192].float(), dt)
    check_stats(stats, stored, b, MPX, MCOUT)


@functools.lru_cache(maxsize=None)
def _multi_bn_fwd(dt, training):
    g = torch.Generator().manual_seed(23)
    cin = 32
    y1 = q(torch.randn(MN, cin, MH, MW, generator=g) * 0.8 + 0.3, dt)
    wt = torch.randn(MCOUT, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    bias = torch.randn(cin, generator=g) * 0.3
    gamma = 1 + 0.2 * torch.randn(cin, generator=g)
    gamma[1] = -gamma[1]
    beta = 0.2 * torch.randn(cin, generator=g)
    rm0, rv0 = 0.1 * torch.randn(cin, generator=g), 0.5 + torch.rand(cin, generator=g)
    yfull = (y1 + bias.view(1, -1, 1, 1)).double()
    a64 = F.relu(F.batch_norm(yfull, rm0.clone().double(), rv0.clone().double(), gamma.double(), beta.double(), training, 0.1, 1e-5))
    ref = F.conv2d(q(a64.float(), dt).double(), q(wt, dt).double(), padding=1)
    return y1, wt, bias, gamma, beta, rm0, rv0, ref


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", MULTI_CASES, ids=multi_id)
def test_multi_item_loop_bn_relu_input_transform(case, training):
    """NUNET_TF_BN_RELU with workgroups that move between Cout tiles: the side-stored activation is written once per pixel
    (by the items of Cout tile 0 only, wherever in a workgroup's sequence they fall) and equals bn_relu_fwd's; outputs equal
    the unfused pair bit for bit; running statistics, saved mean / invstd and num_batches_tracked as the BN kernel leaves them."""
    tile, dt = case
    n, h, w, cin, cout = MN, MH, MW, 32, MCOUT
    y1, wt, bias_c, gamma_c, beta_c, rm0, rv0, ref = _multi_bn_fwd(dt, training)
    bias, gamma, beta = bias_c.to(DEV), gamma_c.to(DEV), beta_c.to(DEV)
    yb = nhwc(y1, dt)
    dd = y1.double()
    stats = L.fx_encode(torch.cat([dd.sum((0, 2, 3)), (dd * dd).sum((0, 2, 3))]), cin, DEV)
    wf, _ = pack(wt, dt)
    # reference path: stand-alone BN kernel, then the plain conv on the same tile
    a_ref = torch.zeros((n, h, w, cin), dtype=tdt(dt), device=DEV)
    rm_a, rv_a = rm0.clone().to(DEV), rv0.clone().to(DEV)
    nbt_a = torch.tensor([2], dtype=torch.int64, device=DEV)
    save_a = torch.zeros(2 * cin, dtype=torch.float32, device=DEV)
    b = L.BnFwdDesc(dt, n, h, w, cin, L.ptr(yb), cin, L.ptr(bias), L.ptr(stats), L.ptr(gamma), L.ptr(beta),
                    L.ptr(rm_a), L.ptr(rv_a), L.ptr(nbt_a), L.ptr(save_a), 1 if training else 0, 0.1, 1e-5,
                    L.ptr(a_ref), cin, None, 0)
    L.check(L.lib().nunet_bn_relu_fwd(C.byref(b), L.stream()), "bn")
    out_ref = torch.zeros((n, h, w, cout), dtype=tdt(dt), device=DEV)
    d0 = conv_desc(dt, n, h, w, a_ref, cin, cin, wf, out_ref, cout, cout)
    d0.tile = tile
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d0), L.stream()), "conv")
    # fused path
    out = torch.zeros_like(out_ref)
    a_side = torch.full((n, h, w, cin), 5.0, dtype=tdt(dt), device=DEV)
    rm_b, rv_b = rm0.clone().to(DEV), rv0.clone().to(DEV)
    nbt_b = torch.tensor([2], dtype=torch.int64, device=DEV)
    save_b = torch.zeros(2 * cin, dtype=torch.float32, device=DEV)
    st2 = L.fx_zeros(cout, DEV)
    d = conv_desc(dt, n, h, w, yb, cin, cin, wf, out, cout, cout, stats=st2)
    d.tile = tile
    d.in_tf = L.TF_BN_RELU; d.tf_training = 1 if training else 0
    d.tf_fx = L.ptr(stats).value; d.tf_gamma = L.ptr(gamma).value; d.tf_beta = L.ptr(beta).value; d.tf_conv_bias = L.ptr(bias).value
    d.tf_running_mean = L.ptr(rm_b).value; d.tf_running_var = L.ptr(rv_b).value; d.tf_nbt = L.ptr(nbt_b).value
    d.tf_mean_invstd = L.ptr(save_b).value; d.tf_momentum = 0.1; d.tf_eps = 1e-5
    d.tf_store = L.ptr(a_side).value; d.tf_ps = cin
    require_multi_item(d, tile)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv+tf")
    torch.cuda.synchronize()
    assert float(a_ref.float().abs().max()) > 0
    assert torch.equal(a_side, a_ref)                       # every pixel stored, same rounding
    assert torch.equal(out, out_ref)
    assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b) and torch.equal(save_a, save_b) and torch.equal(nbt_a, nbt_b)
    assert int(nbt_b.item()) == (3 if training else 2)
    got = to_nchw(out, cout)
    assert rel_err(got, ref) < 4 * TOL[dt]
    m = n * h * w
    tot = L.fx_decode(st2, cout)
    gd = got.double()
    np.testing.assert_allclose(tot[:cout].numpy() / m, gd.sum((0, 2, 3)).numpy() / m, atol=1e-4 * float(gd.abs().max()) + 1e-6)


@functools.lru_cache(maxsize=None)
def _multi_bn_bwd(dt):
    g = torch.Generator().manual_seed(29)
    c = 32
    y = q(torch.randn(MN, c, MH, MW, generator=g), dt)
    da = q(torch.randn(MN, c, MH, MW, generator=g), dt)
    wt = torch.randn(MCOUT, c, 3, 3, generator=g) / (3 * c ** 0.5)
    gamma = 1 + 0.2 * torch.randn(c, generator=g)
    beta = 0.2 * torch.randn(c, generator=g)

    def z(t):
        return F.batch_norm(t.double(), None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
    # The ReLU mask is a step: where bn(y) is within rounding of 0, the kernel's fp32 and the reference's fp64 may take different
    # sides and the gradient of that element differs by all of da. Half a million elements make such an element likely, so the
    # few within 2e-3 of the threshold are moved off it (by 0.05 in y, ~0.05 in bn(y)); the fp64 comparison is then well posed.
    y = q(y + 0.05 * (z(y).abs() < 2e-3).float(), dt)
    assert float(z(y).abs().min()) > 1e-3
    yd = y.double().requires_grad_(True)
    F.relu(F.batch_norm(yd, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)).backward(da.double())
    ref = F.conv2d(q(yd.grad.float(), dt).double(), q(wt, dt).double(), padding=1)
    return y, da, wt, gamma, beta, ref


@pytest.mark.parametrize("case", MULTI_CASES, ids=multi_id)
def test_multi_item_loop_bn_relu_bwd_input_transform(case):
    """NUNET_TF_BN_RELU_BWD in the multi-item regime: outputs and the side-stored dy equal nunet_bn_relu_bwd_apply followed by
    the plain conv bit for bit; d gamma / d beta / d bias equal the stand-alone kernel's; and against fp64."""
    tile, dt = case
    n, h, w, c, cout = MN, MH, MW, 32, MCOUT
    y, da, wt, gamma_c, beta_c, ref = _multi_bn_bwd(dt)
    gamma, beta = gamma_c.to(DEV), beta_c.to(DEV)
    mean = y.double().mean((0, 2, 3))
    istd = 1 / (y.double().var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    mi = torch.cat([mean, istd]).float().to(DEV)
    yb = nhwc(y, dt)
    dab = nhwc(da, dt, pitch=c + 64, off=32)               # the gradient lives in a slot of a wider level buffer
    da_ptr = L.ptr(dab, 32 * dab.element_size())
    sums = L.fx_zeros(c, DEV)
    vec = [torch.full((c,), 9.0, dtype=torch.float32, device=DEV) for _ in range(6)]
    dy_ref = torch.zeros((n, h, w, c), dtype=tdt(dt), device=DEV)
    b = L.BnBwdDesc(dt, n, h, w, c, da_ptr, c + 64, L.ptr(yb), c, L.ptr(mi), L.ptr(gamma), L.ptr(beta), L.ptr(sums),
                    L.ptr(vec[0]), L.ptr(vec[1]), L.ptr(vec[2]), L.ptr(dy_ref), c)
    L.check(L.lib().nunet_bn_relu_bwd_reduce(C.byref(b), L.stream()), "reduce")
    L.check(L.lib().nunet_bn_relu_bwd_apply(C.byref(b), L.stream()), "apply")
    wf, _ = pack(wt, dt)
    out_ref = torch.zeros((n, h, w, cout), dtype=tdt(dt), device=DEV)
    d0 = conv_desc(dt, n, h, w, dy_ref, c, c, wf, out_ref, cout, cout)
    d0.tile = tile
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d0), L.stream()), "dgrad")
    out = torch.zeros_like(out_ref)
    dy_side = torch.full((n, h, w, c), 5.0, dtype=tdt(dt), device=DEV)
    d = L.ConvDesc()
    d.dtype = dt; d.N = n; d.H = h; d.W = w
    d.src0 = da_ptr.value; d.C0 = c; d.P0 = c + 64
    d.wpack = L.ptr(wf).value; d.dst0 = L.ptr(out).value; d.D0 = cout; d.Q0 = cout
    d.tile = tile
    d.in_tf = L.TF_BN_RELU_BWD; d.tf_y = L.ptr(yb).value; d.tf_py = c; d.tf_fx = L.ptr(sums).value
    d.tf_gamma = L.ptr(gamma).value; d.tf_beta = L.ptr(beta).value; d.tf_mean_invstd = L.ptr(mi).value
    d.tf_dgamma = L.ptr(vec[3]).value; d.tf_dbeta = L.ptr(vec[4]).value; d.tf_dbias = L.ptr(vec[5]).value
    d.tf_store = L.ptr(dy_side).value; d.tf_ps = c
    require_multi_item(d, tile)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "dgrad+tf")
    torch.cuda.synchronize()
    assert float(dy_ref.float().abs().max()) > 0
    assert torch.equal(dy_side, dy_ref)
    assert torch.equal(out, out_ref)
    for k in range(3):
        assert torch.equal(vec[k], vec[3 + k])
    assert float(vec[5].abs().max()) == 0.0
    assert rel_err(to_nchw(out, cout), ref) < 4 * TOL[dt]


@functools.lru_cache(maxsize=None)
def _multi_bnr(dt):
    g = torch.Generator().manual_seed(17)
    cin = 32
    x = torch.randn(MN, cin, MH, MW, generator=g)
    wt = torch.randn(MCOUT, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    y1 = q(torch.randn(MN, MCOUT, MH, MW, generator=g), dt)
    gamma = 1 + 0.2 * torch.randn(MCOUT, generator=g)
    beta = 0.2 * torch.randn(MCOUT, generator=g)
    ref = F.conv2d(q(x, dt).double(), q(wt, dt).double(), padding=1)
    return x, wt, y1, gamma, beta, ref


def _bnr_sums_check(dt, n, h, w, cout, out, yb, mi, gamma_g, beta_g, sums):
    """the fused sums equal nunet_bn_relu_bwd_reduce run on the tensor the conv stored"""
    ref_sums = L.fx_zeros(cout, DEV)
    dummy = torch.zeros(cout, dtype=torch.float32, device=DEV)
    b = L.BnBwdDesc(dt, n, h, w, cout, L.ptr(out), cout, L.ptr(yb), cout, L.ptr(mi), L.ptr(gamma_g), L.ptr(beta_g),
                    L.ptr(ref_sums), L.ptr(dummy), L.ptr(dummy), L.ptr(dummy), None, 0)
    L.check(L.lib().nunet_bn_relu_bwd_reduce(C.byref(b), L.stream()), "reduce")
    torch.cuda.synchronize()
    assert float(ref_sums.abs().max()) > 0
    tot, rtot = L.fx_decode(sums, cout), L.fx_decode(ref_sums, cout)
    scale = float(rtot.abs().max())
    assert float((tot - rtot).abs().max()) < 2e-4 * scale + 1e-5


@pytest.mark.parametrize("case", MULTI_CASES, ids=multi_id)
def test_multi_item_loop_fused_bn_bwd_reduce(case):
    """The BatchNorm+ReLU backward reduce in the conv epilogue, with the y1 vectors of an item requested under the sweep that
    also prefetches the next item."""
    tile, dt = case
    n, h, w, cin, cout = MN, MH, MW, 32, MCOUT
    x, wt, y1, gamma, beta, ref = _multi_bnr(dt)
    mean = y1.double().mean((0, 2, 3))
    istd = 1 / (y1.double().var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    mi = torch.cat([mean, istd]).float().to(DEV)
    s0 = nhwc(x, dt)
    wf, _ = pack(wt, dt)
    yb = nhwc(y1, dt)
    out = torch.zeros((n, h, w, cout), dtype=tdt(dt), device=DEV)
    sums = L.fx_zeros(cout, DEV)
    gamma_g, beta_g = gamma.to(DEV), beta.to(DEV)
    d = conv_desc(dt, n, h, w, s0, cin, cin, wf, out, cout, cout)
    d.tile = tile
    d.bn_y = L.ptr(yb).value; d.bn_py = cout; d.bn_mean_invstd = L.ptr(mi).value
    d.bn_gamma = L.ptr(gamma_g).value; d.bn_beta = L.ptr(beta_g).value; d.bn_sums = L.ptr(sums).value
    require_multi_item(d, tile)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv+bnr")
    torch.cuda.synchronize()
    assert rel_err(to_nchw(out, cout), ref) < TOL[dt]
    _bnr_sums_check(dt, n, h, w, cout, out, yb, mi, gamma_g, beta_g, sums)


# ---------------------------------------------------------------------------------------------------------------------
# d. K-split under every tile, uneven and source-straddling slices
# ---------------------------------------------------------------------------------------------------------------------
KS_SHAPE = (2, 12, 12, 128)
# channel CHUNKS (64 bytes: 32 / 16 channels) of source 0 and source 1
KS_CHUNKS = [
    (8, 8),     # 16 chunks, S = 8: even slices that end on the source boundary
    (7, 4),     # 11 chunks, S = 5: slices of 2, 2, 2, 2, 3 chunks; chunks 6 | 7 of the fourth are source 0 | source 1
    (3, 6),     # 9 chunks, S = 4: slices of 2, 2, 2, 3; the second holds the last chunk of source 0 and the first of source 1
]


@functools.lru_cache(maxsize=None)
def _ksplit_case(dt, chunks):
    n, h, w, cout = KS_SHAPE
    kc = 16 if dt == L.F32 else 32
    c0, c1 = chunks[0] * kc, chunks[1] * kc
    g = torch.Generator().manual_seed(21 + chunks[0])
    cin = c0 + c1
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    prev = torch.randn(n, cout, h, w, generator=g)
    ref = F.conv2d(q(x, dt).double(), q(wt, dt).double(), b.double(), padding=1)
    return c0, c1, x, wt, b, prev, ref


def _slices(o):
    """chunk ranges of the K-split slices (conv3x3.hip: slice k walks chunks [k * nch / S, (k + 1) * nch / S))"""
    return [(k * o.nch // o.S, (k + 1) * o.nch // o.S) for k in range(o.S)]


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("chunks", KS_CHUNKS, ids=lambda c: "chunks%d+%d" % c)
@pytest.mark.parametrize("tile", TILES)
def test_ksplit_every_tile_uneven_and_straddling_slices(tile, chunks, dt):
    n, h, w, cout = KS_SHAPE
    c0, c1, x, wt, b, prev, ref = _ksplit_case(dt, chunks)
    s0, s1 = nhwc(x[:, :c0], dt), nhwc(x[:, c0:], dt)
    wf, _ = pack(wt, dt)
    bg = b.to(DEV)
    ws = torch.full((8 * n * h * w * cout,), 7.0, dtype=torch.float32, device=DEV)   # garbage: slabs are fully overwritten
    outs, sts = [], []
    for accum in (0, 1, 0):
        y = nhwc(prev, dt)
        stats = L.fx_zeros(cout, DEV)
        d = conv_desc(dt, n, h, w, s0, c0, c0, wf, y, cout, cout, src1=s1, c1=c1, p1=c1, bias=bg, stats=stats,
                      slot_w=64, mask=0b10 if accum else 0)
        d.splitk_ws = L.ptr(ws).value
        d.splitk_ws_floats = ws.numel()
        d.tile = tile
        o = conv_info(d)
        assert o.tile == tile and o.S > 1 and o.nch == sum(chunks), (o.tile, o.S, o.nch)
        sl = _slices(o)
        if chunks != (8, 8):
            assert o.nch % o.S != 0 and len({hi - lo for lo, hi in sl}) > 1, "slices are even"
            assert any(lo < chunks[0] < hi for lo, hi in sl), "no slice holds chunks of both sources"
        L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv splitk")
        exp = ref.clone()
        if accum:
            exp[:, 64:] += q(prev, dt)[:, 64:].double()          # slot 1 accumulates, slot 0 overwrites
        got = to_nchw(y, cout)
        assert rel_err(got, exp) < TOL[dt], (DT[dt], chunks, tile, accum)
        if not accum:
            check_stats(stats, got, b, n * h * w, cout)
            outs.append(y.clone()); sts.append(stats.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(stat_words(sts[0]), stat_words(sts[1]))   # integer sums: exact


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("tile", TILES)
def test_ksplit_finalize_bn_bwd_reduce_every_tile(tile, dt):
    """The K-split finalize that also takes the BatchNorm-backward sums, fed by the slabs of each tile configuration
    (uneven slices, one of them over both sources)."""
    n, h, w, cout = KS_SHAPE
    chunks = (7, 4)
    c0, c1, x, wt, _, _, _ = _ksplit_case(dt, chunks)
    g = torch.Generator().manual_seed(77)
    y1 = q(torch.randn(n, cout, h, w, generator=g), dt)
    gamma = 1 + 0.2 * torch.randn(cout, generator=g)
    beta = 0.2 * torch.randn(cout, generator=g)
    mean = y1.double().mean((0, 2, 3))
    istd = 1 / (y1.double().var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    mi = torch.cat([mean, istd]).float().to(DEV)
    s0, s1 = nhwc(x[:, :c0], dt), nhwc(x[:, c0:], dt)
    wf, _ = pack(wt, dt)
    yb = nhwc(y1, dt)
    out = torch.zeros((n, h, w, cout), dtype=tdt(dt), device=DEV)
    sums = L.fx_zeros(cout, DEV)
    gamma_g, beta_g = gamma.to(DEV), beta.to(DEV)
    ws = torch.full((8 * n * h * w * cout,), 7.0, dtype=torch.float32, device=DEV)
    d = conv_desc(dt, n, h, w, s0, c0, c0, wf, out, cout, cout, src1=s1, c1=c1, p1=c1)
    d.splitk_ws = L.ptr(ws).value; d.splitk_ws_floats = ws.numel()
    d.tile = tile
    d.bn_y = L.ptr(yb).value; d.bn_py = cout; d.bn_mean_invstd = L.ptr(mi).value
    d.bn_gamma = L.ptr(gamma_g).value; d.bn_beta = L.ptr(beta_g).value; d.bn_sums = L.ptr(sums).value
    o = conv_info(d)
    assert o.tile == tile and o.S > 1 and o.nch % o.S != 0, (o.tile, o.S, o.nch)
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv splitk + bnr")
    torch.cuda.synchronize()
    ref = F.conv2d(q(x, dt).double(), q(wt, dt).double(), padding=1)
    assert rel_err(to_nchw(out, cout), ref) < TOL[dt]
    _bnr_sums_check(dt, n, h, w, cout, out, yb, mi, gamma_g, beta_g, sums)


# ---------------------------------------------------------------------------------------------------------------------
# e. / f. the weight gradient's pixel-tile loop
# ---------------------------------------------------------------------------------------------------------------------
WG_SHAPES = {
    "regular": (2, 24, 48, 64, 32, 64),     # 2304 pixels: 18 tiles of 8 x 16
    "stacked": (16, 12, 12, 64, 32, 64),    # stacked-rows tiling: 21 tiles of 10 virtual rows
}
WG_BIG = 100000                              # target_wgs: as many slices as max_slabs allows


@functools.lru_cache(maxsize=None)
def _wgrad_case(dt, name, seed=11):
    n, h, w, c0, c1, cout = WG_SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    cin = c0 + c1
    x = torch.randn(n, cin, h, w, generator=g)
    dy = torch.randn(n, cout, h, w, generator=g)
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(q(x, dt).double(), wt, padding=1).backward(q(dy, dt).double())
    return x, dy, wt.grad


def _wgrad_inputs(dt, name, seed=11):
    n, h, w, c0, c1, cout = WG_SHAPES[name]
    x, dy, ref = _wgrad_case(dt, name, seed)
    s0 = nhwc(x[:, :c0], dt, pitch=c0 + 64)
    s1 = nhwc(x[:, c0:], dt) if c1 else None
    dyb = nhwc(dy, dt)
    return (dt, n, h, w, s0, c0, c0 + 64, s1, c1, dyb, cout), ref


def _wgrad_slabs(args, ks, item_shape, fill):
    cout, cin = args[10], args[5] + args[8]
    slabs = torch.full((ks * 9 * cout * cin,), fill, dtype=torch.float32, device=DEV)   # plain stores: fully overwritten
    return slabs, wgrad_desc(*args, slabs, ks, WG_BIG, item_shape)


def _wgrad_reduce(args, slabs, ks):
    nw = 9 * args[10] * (args[5] + args[8])
    dw = torch.full((nw,), 3.0, dtype=torch.float32, device=DEV)
    L.check(L.lib().nunet_wgrad_reduce(L.ptr(slabs), nw, ks, nw, L.ptr(dw), 0, L.stream()), "wgrad_reduce")
    return dw


def _pick_ks(kind, nmt):
    if kind == "one":
        return 1
    if kind == "two":
        return 2
    if kind == "ragged":
        return next(k for k in range(3, nmt) if nmt % k != 0)      # slices of different lengths
    return nmt - 1                                                # one slice runs two tiles, the others one


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("item_shape", [11, 21, 12])
@pytest.mark.parametrize("kind", ["one", "two", "ragged", "all_but_one"])
@pytest.mark.parametrize("name", ["regular", "stacked"])
def test_wgrad_pixel_tile_loop(name, kind, item_shape, dt):
    """Slices that walk several pixel tiles: the next tile's loads in flight under the MFMAs, both LDS stages written and
    reused, accumulation across tiles (with one slice: a single fp32 chain over every pixel)."""
    args, ref = _wgrad_inputs(dt, name)
    cout, cin = args[10], args[5] + args[8]
    probe = wgrad_info(wgrad_desc(*args, None, 0, WG_BIG, item_shape))
    assert probe.nMT >= 5 and probe.ksplit == probe.nMT
    assert (probe.SH != 0) == (name == "stacked")
    assert (probe.A * 10 + probe.B) == item_shape
    ks = _pick_ks(kind, probe.nMT)
    slabs, d = _wgrad_slabs(args, ks, item_shape, 1e30)
    o = wgrad_info(d)
    assert o.ksplit == ks == L.lib().nunet_conv3x3_wgrad_slabs(C.byref(d)) and o.nMT > o.ksplit, (o.ksplit, o.nMT)
    if kind == "one":
        assert o.nMT >= 5                    # stage 0, 1, 0, 1, 0: both stages are written again after they were read
    if kind == "ragged":
        assert o.nMT % o.ksplit != 0
    L.check(L.lib().nunet_conv3x3_wgrad(C.byref(d), L.stream()), "wgrad")
    dw = _wgrad_reduce(args, slabs, ks)
    gout = torch.zeros(cout * cin * 9, dtype=torch.float32, device=DEV)
    L.check(L.lib().nunet_unpack_wgrad(L.ptr(dw), cout, cin, cin, L.ptr(gout), 0, L.stream()), "unpack")
    got = gout.view(cout, cin, 3, 3).cpu()
    assert rel_err(got, ref) < WTOL[dt], (DT[dt], name, kind, item_shape)


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("names", [("regular", "regular"), ("stacked", "stacked"), ("regular", "stacked")], ids="+".join)
@pytest.mark.parametrize("shapes", [(12, 11), (21, 11), (11, 21), (21, 21)], ids=lambda s: "%d%d" % s)
def test_wgrad_pair_item_shapes_and_fallback(shapes, names, dt):
    """Every fused item-shape pair of the pair kernel, in both tiling modes, and the two-launch fallback (problems of different
    tiling modes): bit-identical to two single launches, with slices that walk several pixel tiles."""
    ks = 4
    lib = L.lib()
    single, paired, keep = [], [], []
    for name, ish, seed in zip(names, shapes, (5, 6)):
        args, _ = _wgrad_inputs(dt, name, seed)
        keep.append(args)
        slabs, d = _wgrad_slabs(args, ks, ish, 1e30)
        o = wgrad_info(d)
        assert o.ksplit == ks and o.nMT > ks and (o.A * 10 + o.B) == ish and (o.SH != 0) == (name == "stacked")
        L.check(lib.nunet_conv3x3_wgrad(C.byref(d), L.stream()), "wgrad")
        single.append(_wgrad_reduce(args, slabs, ks))
        paired.append(_wgrad_slabs(args, ks, ish, -7.0))
    L.check(lib.nunet_conv3x3_wgrad_pair(C.byref(paired[0][1]), C.byref(paired[1][1]), L.stream()), "wgrad_pair")
    for args, (slabs, _), ref in zip(keep, paired, single):
        dw = _wgrad_reduce(args, slabs, ks)
        assert float(ref.abs().max()) > 0
        assert torch.equal(dw, ref)      # same slices, same summation order: bit-identical


def test_wgrad_default_split_agrees_with_a_forced_one():
    """wgrad_run (the default K-split: one tile per slice here) and a two-slice launch differ by fp32 summation order only."""
    dt = L.BF16
    args, _ = _wgrad_inputs(dt, "regular")
    dw0 = wgrad_run(*args)
    slabs, d = _wgrad_slabs(args, 2, 0, 1e30)
    assert wgrad_info(d).ksplit == 2
    L.check(L.lib().nunet_conv3x3_wgrad(C.byref(d), L.stream()), "wgrad")
    dw = _wgrad_reduce(args, slabs, 2)
    assert rel_err(dw.cpu(), dw0.cpu()) < 2e-5
