"""conv3x3 BatchNorm-backward instantiations: registers, residency and grid against each other, results against the unfused path.

The persistent grid of a conv launch is sized for `per_cu` resident workgroups per CU (nunet_conv3x3_launch_info). That only
holds if the kernel instantiation the launch takes really fits that many: no scratch (a spilling kernel also pays memory
traffic the result does not need) and an occupancy, as the runtime computes it from the code object's registers and LDS, of
at least `per_cu` (nunet_conv_kernel_attrs). The cases are the input-gradient convs of the training step: the BatchNorm+ReLU
backward apply in the loader (LT2), with the BatchNorm-1 backward reduce in the epilogue for a block's second conv (BNR+LT2),
on each tile the plan launches them with, and the K-split form of the deep levels. The remaining instantiations of the
128 x 32 tile, which carry the same three-per-CU promise, are asked for scratch and occupancy only (last test).

Every GPU case is N = 2, 12 x 12 (ragged pixel tiles, several work items of both pixel and Cout tiles, two channel chunks
for Cin = 64), K-split: N = 1, 6 x 6 with 16 chunks. What a workgroup does when it runs SEVERAL items is the subject of
tests/test_conv_tiles_gpu.py; here each case asserts which instantiation it reaches."""
import ctypes as C
import functools

import pytest
import torch

from nunet_amd import _lib as L


def conv_info(d):
    o = L.ConvLaunchInfo()
    L.check(L.lib().nunet_conv3x3_launch_info(C.byref(d), C.byref(o)), "conv launch info")
    return o


def test_b22_dgrad1_grid_fits_the_resident_workgroups():
    """Host only. B22.dgrad1 of the 96 x 96, batch 16 step: 24 x 24 x 16 pixels in 80 pixel tiles of 5 rows, Cin 128 -> Cout 512
    (two destinations), BatchNorm-backward loader. Whatever tile it runs on, its grid fits per_cu workgroups on each of the 256 CUs and needs no
    more rounds than that residency gives; per_cu is what LDS, threads AND the registers of the LT2 instantiation admit.
    The policy gives it the 128 x 64 tile (640 items, two per CU by LDS and by registers). Forced onto the 128 x 32 tile it has
    1280 items: three workgroups per CU are resident - the LT2 kernel runs in at most 168 registers - so the grid of 640 holds
    no workgroup that waits for another one to run all its rounds (with two per CU it would have to be 427, three rounds)."""
    for tile, want in ((0, (2, 128, 64, 640, 2, 320)), (1, (1, 128, 32, 1280, 3, 640))):
        d = L.ConvDesc()
        d.dtype = L.BF16; d.N = 16; d.H = 24; d.W = 24
        d.C0 = 128; d.P0 = 128; d.D0 = 256; d.Q0 = 256; d.D1 = 256; d.Q1 = 256
        d.in_tf = L.TF_BN_RELU_BWD; d.tf_py = 128; d.tile = tile
        o = conv_info(d)
        assert o.S == 1 and o.tilesX * o.tilesY * o.tilesG == 80
        assert o.per_cu >= 1 and o.grid <= 256 * o.per_cu, (tile, o.grid, o.per_cu)
        assert -(-o.items // o.grid) == -(-o.items // (256 * o.per_cu)), (tile, o.items, o.grid, o.per_cu)
        assert (o.tile, o.BM, o.BN, o.items, o.per_cu, o.grid) == want, (tile, o.tile, o.BM, o.BN, o.items, o.per_cu, o.grid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------------------------------------------------
# (name, BNR, Cin, Cout, (N, H, W), forced tile (0: the policy's), expected tile, K-split)
CASES = [
    ("lt2-128x32", False, 64, 96, (2, 12, 12), 1, 1, False),
    ("lt2-256x32", False, 64, 96, (2, 12, 12), 3, 3, False),
    ("bnr+lt2-128x32", True, 32, 32, (2, 12, 12), 1, 1, False),
    ("bnr+lt2-256x32", True, 32, 32, (2, 12, 12), 3, 3, False),
    ("bnr+lt2-128x64", True, 64, 64, (2, 12, 12), 2, 2, False),
    ("lt2-ksplit", False, 512, 32, (1, 6, 6), 0, 1, True),
]


@functools.lru_cache(maxsize=None)
def _inputs(cin, cout, shape):
    """fp32 CPU inputs of a case, shared by its dtypes (left unchanged)"""
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 + cin + cout + h)
    y = torch.randn(n, cin, h, w, generator=g)                  # raw output of the conv whose BatchNorm the loader differentiates
    da = torch.randn(n, cin, h, w, generator=g)                 # gradient w.r.t. that BatchNorm+ReLU's output
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    gamma = 1 + 0.2 * torch.randn(cin, generator=g)
    beta = 0.2 * torch.randn(cin, generator=g)
    y1 = torch.randn(n, cout, h, w, generator=g)                # BNR: raw output of the block's first conv
    gamma1 = 1 + 0.2 * torch.randn(cout, generator=g)
    beta1 = 0.2 * torch.randn(cout, generator=g)
    return y, da, wt, gamma, beta, y1, gamma1, beta1


def _mean_invstd(t, dev):
    mean = t.double().mean((0, 2, 3))
    istd = 1 / (t.double().var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    return torch.cat([mean, istd]).float().to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [L.BF16, L.F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bn_backward_conv_fits_its_grid_and_equals_the_unfused_path(case, dt, guard_bands):
    from test_ops_gpu import DEV, conv_desc, nhwc, pack, q, tdt
    name, bnr, cin, cout, (n, h, w), tile, want_tile, ksplit = case
    lib = L.lib()
    y_c, da_c, wt, gamma_c, beta_c, y1_c, gamma1_c, beta1_c = _inputs(cin, cout, (n, h, w))
    y, da, y1 = q(y_c, dt), q(da_c, dt), q(y1_c, dt)
    gamma, beta, gamma1, beta1 = gamma_c.to(DEV), beta_c.to(DEV), gamma1_c.to(DEV), beta1_c.to(DEV)
    mi, mi1 = _mean_invstd(y, DEV), _mean_invstd(y1, DEV)
    yb, dab, y1b = nhwc(y, dt), nhwc(da, dt), nhwc(y1, dt)
    wf, _ = pack(wt, dt)
    ws = torch.full((8 * n * h * w * cout,), 7.0, dtype=torch.float32, device=DEV) if ksplit else None   # slabs are fully overwritten

    def finish(d):
        d.tile = tile
        if ws is not None:
            d.splitk_ws = L.ptr(ws).value; d.splitk_ws_floats = ws.numel()
        return d

    def with_bnr(d, sums):
        d.bn_y = L.ptr(y1b).value; d.bn_py = cout; d.bn_mean_invstd = L.ptr(mi1).value
        d.bn_gamma = L.ptr(gamma1).value; d.bn_beta = L.ptr(beta1).value; d.bn_sums = L.ptr(sums).value
        return d

    # ---- the unfused path: stand-alone reduce + apply, the plain conv on the same tile, stand-alone reduce of BatchNorm 1
    sums = L.fx_zeros(cin, DEV)
    vec = [torch.full((cin,), 9.0, dtype=torch.float32, device=DEV) for _ in range(6)]
    dy_ref = torch.zeros((n, h, w, cin), dtype=tdt(dt), device=DEV)
    b = L.BnBwdDesc(dt, n, h, w, cin, L.ptr(dab), cin, L.ptr(yb), cin, L.ptr(mi), L.ptr(gamma), L.ptr(beta), L.ptr(sums),
                    L.ptr(vec[0]), L.ptr(vec[1]), L.ptr(vec[2]), L.ptr(dy_ref), cin)
    L.check(lib.nunet_bn_relu_bwd_reduce(C.byref(b), L.stream()), "reduce")
    L.check(lib.nunet_bn_relu_bwd_apply(C.byref(b), L.stream()), "apply")
    out_ref = torch.zeros((n, h, w, cout), dtype=tdt(dt), device=DEV)
    L.check(lib.nunet_conv3x3_fwd(C.byref(finish(conv_desc(dt, n, h, w, dy_ref, cin, cin, wf, out_ref, cout, cout))), L.stream()), "plain conv")
    if bnr:
        ref_sums = L.fx_zeros(cout, DEV)
        dummy = torch.zeros(cout, dtype=torch.float32, device=DEV)
        b1 = L.BnBwdDesc(dt, n, h, w, cout, L.ptr(out_ref), cout, L.ptr(y1b), cout, L.ptr(mi1), L.ptr(gamma1), L.ptr(beta1),
                         L.ptr(ref_sums), L.ptr(dummy), L.ptr(dummy), L.ptr(dummy), None, 0)
        L.check(lib.nunet_bn_relu_bwd_reduce(C.byref(b1), L.stream()), "reduce 1")
        # ... and the same reduce taken in the epilogue of the conv on the unfused input: the same partition of the sums
        epi_sums = L.fx_zeros(cout, DEV)
        out_epi = torch.zeros_like(out_ref)
        d1 = with_bnr(finish(conv_desc(dt, n, h, w, dy_ref, cin, cin, wf, out_epi, cout, cout)), epi_sums)
        L.check(lib.nunet_conv3x3_fwd(C.byref(d1), L.stream()), "conv + reduce")

    # ---- the fused launch
    out = torch.zeros_like(out_ref)
    dy_side = torch.full((n, h, w, cin), 5.0, dtype=tdt(dt), device=DEV)
    bn_sums = L.fx_zeros(cout, DEV)
    d = finish(conv_desc(dt, n, h, w, dab, cin, cin, wf, out, cout, cout))
    d.in_tf = L.TF_BN_RELU_BWD; d.tf_y = L.ptr(yb).value; d.tf_py = cin; d.tf_fx = L.ptr(sums).value
    d.tf_gamma = L.ptr(gamma).value; d.tf_beta = L.ptr(beta).value; d.tf_mean_invstd = L.ptr(mi).value
    d.tf_dgamma = L.ptr(vec[3]).value; d.tf_dbeta = L.ptr(vec[4]).value; d.tf_dbias = L.ptr(vec[5]).value
    d.tf_store = L.ptr(dy_side).value; d.tf_ps = cin
    if bnr:
        with_bnr(d, bn_sums)

    # which instantiation, how many of it fit, and what the grid assumes
    o = conv_info(d)
    assert o.tile == want_tile and (o.S > 1) == ksplit and o.nch == cin // 32, (name, o.tile, o.S, o.nch)
    assert o.items > 1 and o.nCoT * o.BN == cout
    a = L.ConvKernelAttrs()
    L.check(lib.nunet_conv_kernel_attrs(C.byref(d), C.byref(a)), "conv kernel attrs")
    print("%s %s: %d registers, %d bytes of scratch, %d + %d bytes of LDS, occupancy %d, promised %d, per_cu %d, grid %d of %d items"
          % (name, {L.BF16: "bf16", L.F16: "fp16"}[dt], a.numRegs, a.localSizeBytes, a.sharedSizeBytes, a.dynLdsBytes, a.occupancy,
             a.wg_per_cu, o.per_cu, o.grid, o.items))
    assert a.blockSize == o.NT
    assert a.localSizeBytes == 0
    assert a.occupancy >= o.per_cu
    assert a.wg_per_cu >= o.per_cu
    assert o.grid <= 256 * o.per_cu

    L.check(lib.nunet_conv3x3_fwd(C.byref(d), L.stream()), "fused conv")
    torch.cuda.synchronize()
    assert float(dy_ref.float().abs().max()) > 0 and float(out_ref.float().abs().max()) > 0
    assert torch.equal(dy_side, dy_ref)                     # the tf_store side store: every pixel, same rounding
    assert torch.equal(out, out_ref)
    for k in range(3):
        assert torch.equal(vec[k], vec[3 + k])              # d gamma, d beta, d bias
    if bnr:
        assert torch.equal(out_epi, out_ref)
        assert float(ref_sums.abs().max()) > 0
        # Word for word the sums of the epilogue reduce on the unfused input (same workgroups, same fp32 partial sums).
        assert torch.equal(bn_sums, epi_sums)
        # Against the stand-alone reduce kernel the fixed-point words can only agree up to fp32 summation order: both add
        # fp32 partial sums (exactly, in fixed point) of the SAME dz and dz * xhat terms, but over different groups of pixels.
        # Any order of summing the N = n * h * w terms of a channel is within (N - 1) * 2^-24 * sum |term| of the exact sum
        # (first order; + 4 for the terms' own rounding, xhat and the product), so the two differ by at most twice that.
        # (|dz| <= |stored gradient| whatever the ReLU mask; xhat from the saved mean / invstd)
        npx = n * h * w
        dz = out_ref.float().permute(0, 3, 1, 2).cpu().double()
        m1 = mi1.cpu().double()
        xhat = (y1.double() - m1[:cout].view(1, -1, 1, 1)) * m1[cout:].view(1, -1, 1, 1)
        got, ref = L.fx_decode(bn_sums, cout), L.fx_decode(ref_sums, cout)
        bound1 = 2 * (npx + 4) * 2.0 ** -24 * dz.abs().sum((0, 2, 3)) + 1e-12
        bound2 = 2 * (npx + 4) * 2.0 ** -24 * (dz * xhat).abs().sum((0, 2, 3)) + 1e-12
        assert bool(((got[:cout] - ref[:cout]).abs() <= bound1).all()), float(((got[:cout] - ref[:cout]).abs() / bound1).max())
        assert bool(((got[cout:] - ref[cout:]).abs() <= bound2).all()), float(((got[cout:] - ref[cout:]).abs() / bound2).max())


# The other instantiations of the 128 x 32 tile carry the same three-per-CU promise in their __launch_bounds__ (at most 168
# registers): a compiler that no longer fits one of them spills without any result changing, so their scratch and occupancy
# are asserted as well. No launch: nunet_conv_kernel_attrs only asks the runtime about the code object.
# (name, in_tf, BNR, Cin, Cout, (N, H, W), K-split)
SMALL_TILE = [
    ("plain", 0, False, 64, 96, (2, 12, 12), False),
    ("lt1", 1, False, 64, 96, (2, 12, 12), False),
    ("bnr", 0, True, 32, 32, (2, 12, 12), False),
    ("bnr+lt1", 1, True, 32, 32, (2, 12, 12), False),
    ("ksplit", 0, False, 512, 32, (1, 6, 6), True),
    ("lt1-ksplit", 1, False, 512, 32, (1, 6, 6), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [L.BF16, L.F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", SMALL_TILE, ids=[c[0] for c in SMALL_TILE])
def test_small_tile_instantiations_keep_three_per_cu_without_scratch(case, dt):
    from test_ops_gpu import DEV
    name, in_tf, bnr, cin, cout, (n, h, w), ksplit = case
    d = L.ConvDesc()
    d.dtype = dt; d.N = n; d.H = h; d.W = w
    d.C0 = cin; d.P0 = cin; d.D0 = cout; d.Q0 = cout
    d.in_tf = in_tf; d.tf_training = 1; d.tile = 0 if ksplit else 1
    keep = []
    if bnr:
        keep.append(torch.zeros((n, h, w, cout), dtype=torch.float32, device=DEV))
        d.bn_y = L.ptr(keep[-1]).value; d.bn_py = cout
    if ksplit:
        keep.append(torch.zeros((8 * n * h * w * cout,), dtype=torch.float32, device=DEV))
        d.splitk_ws = L.ptr(keep[-1]).value; d.splitk_ws_floats = keep[-1].numel()
    o = conv_info(d)
    assert o.tile == 1 and (o.S > 1) == ksplit, (name, o.tile, o.S)
    a = L.ConvKernelAttrs()
    L.check(L.lib().nunet_conv_kernel_attrs(C.byref(d), C.byref(a)), "conv kernel attrs")
    print("%s %s: %d registers, %d bytes of scratch, occupancy %d, promised %d, per_cu %d"
          % (name, {L.BF16: "bf16", L.F16: "fp16"}[dt], a.numRegs, a.localSizeBytes, a.occupancy, a.wg_per_cu, o.per_cu))
    assert o.per_cu == 3 and a.wg_per_cu == 3
    assert a.localSizeBytes == 0
    assert a.occupancy >= o.per_cu
    assert o.grid <= 256 * o.per_cu
