"""Element-wise kernels (csrc/elementwise.hip) against plain torch fp64 on the CPU, per element, in every regime of their
launch code: all channel widths (thread geometry G = C / EPV, ppb = 256 / G, bn_sum_replicas(C)), all three storage types,
grids past their caps (second, ragged passes of the software-pipelined loops), both sides of the fast-index-decode edge
(make_dec4), the generic class count of the head backward and the 5 x 5 window of the upsample backward at every size.

Inputs are rounded to the storage type T first; the kernels evaluate in fp32 and round once to T, so the criterion is

    |got - ref64| <= ulp_T(ref64) + 2^-20 * S                                                   (assert_close)

with ulp_T the spacing of T at |ref64| (8 / 11 / 24 significant bits) and S the sum of the magnitudes of the terms added
(given next to every check). The upsample has one further term, 2^-22 * max(2H, 2W) * S: the fp32 source coordinate
scale * dst carries up to one fp32 ulp of the coordinate (< 2^-23 * max(2H, 2W), relative 2^-24) into the lerp weight.

An fp32 CPU evaluation of the same formulas (torch fp32, the fmas rounded once, sequential accumulation) on the inputs
of these tests - the case builders below at every shape of parts A, B, C and D - stayed within this fraction of the bound:
BN apply 0.50, BN backward apply 0.50, upsample forward 0.50, upsample backward 0.50, head backward dx 0.50, max-pool
backward accumulate 0.50 (all of it the half-ulp of the final rounding to T); head forward 0.29 (C = 32, 10^6 pixels)
and 0.24 (C = 64); saved invstd 0.12, running mean 0.35, running variance 0.12. No formula needed a larger constant.

Reductions keep the project's criteria: 2e-4 * scale + 1e-5 for the BatchNorm sums (_bnr_check), rel_err < 1e-4 for
dgamma / dbeta and the head's dw / db slab totals. Routing, padding, sentinels and dbias are exact."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nunet_amd import _lib as L  # noqa: E402
from test_ops_gpu import nhwc, to_nchw, q, tdt, rel_err, DEV, DT, _bnr_setup, _bnr_check  # noqa: E402


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


DTS = [L.F32, L.BF16, L.F16]
P_BITS = {L.F32: 24, L.BF16: 8, L.F16: 11}            # significant bits
E_MIN = {L.F32: -126, L.BF16: -126, L.F16: -14}       # exponent of the smallest normal number
PAD = 8                                               # pitched buffers: PAD elements in front of and behind the C channels


def epv(dt):
    return 4 if dt == L.F32 else 8


def widths(dt):
    """G = C / EPV runs over 1, .., 64 (bf16 / fp16) or 1, .., 128 (fp32): ppb = 256 / G from 256 down to 2;
    bn_sum_replicas(C) = 8, 8, 4, 2, 1, 1"""
    return [epv(dt), 32, 64, 128, 256, 512]


def dtc(cs, dts=None):
    """(dt, C) parameters with readable ids"""
    return [pytest.param(dt, c, id="%s-C%d" % (DT[dt], c)) for dt in (dts or DTS) for c in cs(dt)]


def dt_ids(dts):
    return dict(argvalues=dts, ids=[DT[d] for d in dts])


def nrep_of(c):
    return max(1, min(L.BN_SUM_REPLICAS, 256 // c))    # bn_sum_replicas() of csrc/common.h


def ulp(ref, dt):
    """spacing of the storage type at |ref| (fp64 tensor): 2^floor(log2 |ref|) is the exponent field
    of the double; below the smallest normal number of T (and at 0) the spacing is that of T's subnormals"""
    pow2 = (ref.view(torch.int64) & 0x7FF0000000000000).view(torch.float64)
    return pow2.clamp_(min=2.0 ** E_MIN[dt]).mul_(2.0 ** -(P_BITS[dt] - 1))


def assert_close(got, ref, S, dt, what, coord=0):
    """|got - ref| <= ulp_T(ref) + 2^-20 * S (+ 2^-22 * coord * S for the upsample, coord = max(2H, 2W)), every element.
    S: a float or an fp64 tensor that broadcasts against ref. Prints the worst error / bound ratio before it asserts."""
    k = 2.0 ** -20 + 2.0 ** -22 * coord
    worst, bad = 0.0, 0
    step = max(1, (1 << 25) // max(1, ref[0].numel())) if ref.dim() else 1
    for i in range(0, ref.shape[0] if ref.dim() else 1, step):
        sl = slice(i, i + step) if ref.dim() else Ellipsis
        r = ref[sl].double()
        s = S[sl] if torch.is_tensor(S) and S.dim() == ref.dim() and S.shape[0] == ref.shape[0] else S
        bound = ulp(r, dt).add_(s * k if torch.is_tensor(s) else s * k)
        err = got[sl].double().sub_(r).abs_() if got.dtype != torch.float64 else (got[sl] - r).abs_()
        bad += int((~(err <= bound)).sum())            # (a NaN counts as bad)
        worst = max(worst, float(err.div_(bound).nan_to_num_(nan=float("inf")).max()))
    print("%-28s %s worst err/bound %.3f" % (what, DT[dt], worst))
    assert bad == 0, "%s (%s): %d elements past the bound, worst err/bound %.3f" % (what, DT[dt], bad, worst)


def out_buf(n, h, w, c, dt, fill=5.0):
    """pitched, offset output buffer full of a sentinel; the kernel gets ptr_in(buf) and pitch c + 2 * PAD"""
    return torch.full((n, h, w, c + 2 * PAD), fill, dtype=tdt(dt), device=DEV)


def ptr_in(buf):
    return L.ptr(buf, PAD * buf.element_size())


def pad_untouched(buf, c, fill=5.0):
    return bool((buf[..., :PAD].float() == fill).all()) and bool((buf[..., PAD + c:].float() == fill).all())


def in_buf(x, dt):
    c = x.shape[1]
    return nhwc(x, dt, pitch=c + 2 * PAD, off=PAD)


def fx_encode_replicas(shares, c, device):
    """Fixed-point sum buffer whose replica r holds shares[r] ([nrep][2c] float64): L.fx_encode, one replica at a time
    (what producers leave: each workgroup adds to replica blockIdx & (nrep - 1))."""
    buf = torch.zeros(L.BN_SUM_REPLICAS, 2 * c, L.FX_WORDS, dtype=torch.int64)
    for r in range(shares.shape[0]):
        buf[r] = L.fx_encode(shares[r], c, "cpu").view(L.BN_SUM_REPLICAS, 2 * c, L.FX_WORDS)[0]
    return buf.reshape(-1).to(device)


SHARE_W = [0.9, -0.55, 0.4, 0.3, -0.35, 0.2, 0.15]    # unequal, some negative; the last replica takes the remainder


def spread(total, nrep):
    sh = [total * SHARE_W[r] for r in range(nrep - 1)]
    return torch.stack(sh + [total - sum(sh) if sh else total])


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU forward
# ---------------------------------------------------------------------------------------------------------------------
def bn_fwd_case(dt, n, h, w, c, training, seed=2):
    """inputs (rounded to T) and the fp64 reference: F.batch_norm + relu of stored + conv bias; S = |y sc| + |mean sc| + |beta|"""
    g = torch.Generator().manual_seed(seed)
    k = dict(dt=dt, n=n, h=h, w=w, c=c, training=training)
    k["bias"] = torch.randn(c, generator=g) * 0.3
    k["ys"] = ys = q(torch.randn(n, c, h, w, generator=g) * 0.7 + 0.2 * torch.randn(1, c, 1, 1, generator=g), dt)
    k["gamma"] = gamma = 1 + 0.2 * torch.randn(c, generator=g)
    gamma[1 % c] = -gamma[1 % c]
    k["beta"] = beta = 0.2 * torch.randn(c, generator=g)
    k["rm"] = rm = 0.1 * torch.randn(c, generator=g)
    k["rv"] = rv = 0.5 + torch.rand(c, generator=g)
    dd = ys.double()
    k["tot"] = torch.cat([dd.sum((0, 2, 3)), (dd * dd).sum((0, 2, 3))])
    rm2, rv2 = rm.double(), rv.double()
    k["ref"] = F.relu(F.batch_norm(dd + k["bias"].double().view(1, -1, 1, 1), rm2, rv2, gamma.double(), beta.double(), training, 0.1, 1e-5))
    k["rm2"], k["rv2"] = rm2, rv2
    if training:
        mean, var = dd.mean((0, 2, 3)), dd.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rm.double() - k["bias"].double(), rv.double()
    k["mean"], k["var"] = mean, var
    sc = gamma.double() / (var + 1e-5).sqrt()
    v = lambda t: t.view(1, -1, 1, 1)
    k["S"] = (dd * v(sc)).abs() + v((mean * sc).abs() + beta.double().abs())
    return k


def bn_fwd_run(k, pool, up, what):
    dt, n, h, w, c, training = k["dt"], k["n"], k["h"], k["w"], k["c"], k["training"]
    yb = in_buf(k["ys"], dt)
    stats = fx_encode_replicas(spread(k["tot"], nrep_of(c)), c, DEV) if training else None
    a = out_buf(n, h, w, c, dt)
    pooled = torch.full((n, h // 2, w // 2, c), 5.0, dtype=tdt(dt), device=DEV) if pool else None
    upb = out_buf(n, 2 * h, 2 * w, c, dt) if up else None
    rmg, rvg = k["rm"].clone().to(DEV), k["rv"].clone().to(DEV)
    nbt = torch.tensor([4], dtype=torch.int64, device=DEV)
    save = torch.zeros(2 * c, dtype=torch.float32, device=DEV)
    bias_g, gamma_g, beta_g = k["bias"].to(DEV), k["gamma"].to(DEV), k["beta"].to(DEV)
    d = L.BnFwdDesc(dt, n, h, w, c, ptr_in(yb), c + 2 * PAD, L.ptr(bias_g), L.ptr(stats), L.ptr(gamma_g), L.ptr(beta_g),
                    L.ptr(rmg), L.ptr(rvg), L.ptr(nbt), L.ptr(save), 1 if training else 0, 0.1, 1e-5,
                    ptr_in(a), c + 2 * PAD, L.ptr(pooled), c, ptr_in(upb) if up else None, c + 2 * PAD)
    L.check(L.lib().nunet_bn_relu_fwd(C.byref(d), L.stream()), "bn")
    got = to_nchw(a, c, off=PAD)
    assert_close(got, k["ref"], k["S"], dt, what + " a")
    assert pad_untouched(a, c)
    if pool:
        assert torch.equal(to_nchw(pooled, c), F.max_pool2d(got, 2, 2)), what + " pooled"
    if up:
        # the fused upsample is defined on the STORED activation (every tap rounded to T first)
        amax = float(got.abs().max())
        for i in range(n):      # (one image at a time: the x4 tensor in fp64 is the largest thing these tests hold)
            ref_up = F.interpolate(got[i:i + 1].double(), scale_factor=2, mode="bilinear", align_corners=True)
            assert_close(to_nchw(upb[i:i + 1], c, off=PAD), ref_up, amax, dt, what + " up[%d]" % i, coord=max(2 * h, 2 * w))
        assert pad_untouched(upb, c)
    if training:
        m = float(n * h * w)
        mean, var = k["mean"], k["var"]
        # saved mean: the fp32 rounding of the exact mean; saved invstd = 1 / sqrtf(var + eps): four fp32 roundings
        assert_close(save[:c].cpu(), mean, 0.0, L.F32, what + " save_mean")
        invstd = 1 / (var + 1e-5).sqrt()
        assert_close(save[c:].cpu(), invstd, invstd, L.F32, what + " save_invstd")
        mf = mean + k["bias"].double()
        assert_close(rmg.cpu(), k["rm2"], 0.9 * k["rm"].double().abs() + 0.1 * mf.abs(), L.F32, what + " running_mean")
        assert_close(rvg.cpu(), k["rv2"], 0.9 * k["rv"].double() + 0.1 * var * (m / (m - 1)), L.F32, what + " running_var")
        assert int(nbt.item()) == 5
    else:
        assert torch.equal(rmg.cpu(), k["rm"]) and torch.equal(rvg.cpu(), k["rv"]) and int(nbt.item()) == 4


def bn_fwd_widths(dt):
    return widths(dt) + [256 * epv(dt)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dt,c", dtc(bn_fwd_widths))
def test_bn_relu_fwd_widths(dt, c, training):
    """Part A: every channel width at 3 x 6 x 10 = 180 pixels (45 quads), which no ppb = 256 / G (256 .. 1) and no
    ppb * U divides; the largest C the kernel accepts, 256 * EPV (G = 256, ppb = 1: the s_sc / s_sh tables are full), too.
    Plain, pooled, up and pooled + up; the training statistics are spread over all bn_sum_replicas(C) replicas."""
    k = bn_fwd_case(dt, 3, 6, 10, c, training)
    for pool in (False, True):
        for up in (False, True):
            bn_fwd_run(k, pool, up, "bn_fwd C=%d pool=%d up=%d" % (c, pool, up))


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU backward
# ---------------------------------------------------------------------------------------------------------------------
def bn_bwd_case(dt, n, h, w, c, seed=4):
    g = torch.Generator().manual_seed(seed)
    k = dict(dt=dt, n=n, h=h, w=w, c=c)
    k["y"] = y = q(torch.randn(n, c, h, w, generator=g) + 0.2 * torch.randn(1, c, 1, 1, generator=g), dt)
    da = q(torch.randn(n, c, h, w, generator=g), dt)
    k["gamma"] = gamma = 1 + 0.2 * torch.randn(c, generator=g)
    gamma[1 % c] = -gamma[1 % c]
    k["beta"] = beta = 0.2 * torch.randn(c, generator=g)
    v = lambda t: t.view(1, -1, 1, 1)
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    istd = 1 / (yd.var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    k["mi"] = mi = torch.cat([mean, istd]).float()
    mean, istd = mi[:c].double(), mi[c:].double()                  # what the kernels are given
    sc = gamma.double() * istd
    act = yd * v(sc) + v(beta.double() - mean * sc)
    # the ReLU mask is a step function of act: where act is within fp32 rounding of 0 the incoming gradient is made 0,
    # so that fp32 and fp64 agree on every element's contribution whichever side they take (an input choice, no element
    # of the outputs is left out of a check)
    near = act.abs() < 2.0 ** -18 * ((yd * v(sc)).abs() + v((mean * sc).abs() + beta.double().abs()))
    da[near] = 0
    k["da"] = da
    ydr = yd.clone().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.relu(F.batch_norm(ydr, None, None, gd, bd, True, 0.1, 1e-5)).backward(da.double())
    k["dy"], k["dgamma"], k["dbeta"] = ydr.grad, gd.grad, bd.grad
    dz = torch.where(act > 0, da.double(), torch.zeros((), dtype=torch.float64))
    xh = (yd - v(mean)) * v(istd)
    k["sums"] = torch.cat([dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))])
    m = float(n * h * w)
    k1a, k2a = dz.abs().sum((0, 2, 3)) / m, (dz * xh).abs().sum((0, 2, 3)) / m
    B = sc * (k["sums"][c:] / m) * istd
    # dy = fma(sc, dz, -fma(B, y, A)), A = fma(-B, mean, sc k1), B = sc k2 istd; k1, k2 are fp32 sums of |dz|, |dz xhat| terms
    k["S"] = (v(sc) * dz).abs() + (v(B) * yd).abs() + v((B * mean).abs() + sc.abs() * k1a) + (v(sc) * xh).abs() * v(k2a)
    return k


def bn_bwd_run(k, what):
    dt, n, h, w, c = k["dt"], k["n"], k["h"], k["w"], k["c"]
    yb, dab = in_buf(k["y"], dt), in_buf(k["da"], dt)
    mi, gamma_g, beta_g = k["mi"].to(DEV), k["gamma"].to(DEV), k["beta"].to(DEV)
    sums = L.fx_zeros(c, DEV)
    dg, db, dbias = (torch.full((c,), 9.0, dtype=torch.float32, device=DEV) for _ in range(3))     # assigned, not accumulated
    dyb = out_buf(n, h, w, c, dt)
    d = L.BnBwdDesc(dt, n, h, w, c, ptr_in(dab), c + 2 * PAD, ptr_in(yb), c + 2 * PAD, L.ptr(mi), L.ptr(gamma_g), L.ptr(beta_g),
                    L.ptr(sums), L.ptr(dg), L.ptr(db), L.ptr(dbias), ptr_in(dyb), c + 2 * PAD)
    L.check(L.lib().nunet_bn_relu_bwd_reduce(C.byref(d), L.stream()), "bn bwd reduce")
    tot = L.fx_decode(sums, c)
    scale = float(k["sums"].abs().max())
    err = float((tot - k["sums"]).abs().max())
    print("%-28s %s sums err %.3g of %.3g" % (what, DT[dt], err, 2e-4 * scale + 1e-5))
    assert scale > 0 and err < 2e-4 * scale + 1e-5, what
    if nrep_of(c) > 1 and n * h * w > 256 // (c // epv(dt)) * 8:      # more than one block: more than one replica in use
        used = sums.view(L.BN_SUM_REPLICAS, -1).ne(0).any(1).cpu()
        assert int(used.sum()) > 1 and not bool(used[nrep_of(c):].any())
    L.check(L.lib().nunet_bn_relu_bwd_apply(C.byref(d), L.stream()), "bn bwd apply")
    assert_close(to_nchw(dyb, c, off=PAD), k["dy"], k["S"], dt, what + " dy")
    assert pad_untouched(dyb, c)
    assert rel_err(dg.cpu(), k["dgamma"]) < 1e-4 and rel_err(db.cpu(), k["dbeta"]) < 1e-4
    assert float(dbias.abs().max()) == 0.0


@pytest.mark.parametrize("dt,c", dtc(widths))
def test_bn_relu_bwd_widths(dt, c):
    """Part A: reduce (LDS reduction over ppb = 256 / G threads, one fixed-point add per channel into replica
    blockIdx & (nrep - 1)) and apply (the [6][C] table, fx_totals over the replicas) at every width, 180 pixels."""
    bn_bwd_run(bn_bwd_case(dt, 3, 6, 10, c), "bn_bwd C=%d" % c)


# ---------------------------------------------------------------------------------------------------------------------
# MaxPool2d(2, 2)
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_check(dt, n, h, w, c, what, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(n, c, h, w, generator=g), dt)
    # ties, first maximum in scan order must win: quad j (row-major) holds 6.0, above everything else, in the slots of
    # ties[j]: every pair of slots, three and all four at once, so each slot 0..2 wins a tie and slot 3 loses every one
    ties = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2, 3), (1, 2, 3)]
    assert (h // 2) * (w // 2) >= len(ties)
    for j, slots in enumerate(ties):
        qy, qx = divmod(j, w // 2)
        for s in slots:
            x[:, :, 2 * qy + (s >> 1), 2 * qx + (s & 1)] = 6.0
    dy = q(torch.randn(n, c, h // 2, w // 2, generator=g), dt)
    prev = q(torch.randn(n, c, h, w, generator=g), dt)
    xb = in_buf(x, dt)
    yb = out_buf(n, h // 2, w // 2, c, dt)
    P = c + 2 * PAD
    L.check(L.lib().nunet_maxpool2x2_fwd(dt, n, h, w, c, ptr_in(xb), P, ptr_in(yb), P, L.stream()), "pool")
    xd = x.double().requires_grad_(True)
    ref = F.max_pool2d(xd, 2, 2)
    assert torch.equal(to_nchw(yb, c, off=PAD).double(), ref.detach()), what
    assert pad_untouched(yb, c)
    ref.backward(dy.double())
    dyb = in_buf(dy, dt)
    for acc in (0, 1):
        dxb = in_buf(prev, dt)
        L.check(L.lib().nunet_maxpool2x2_bwd(dt, n, h, w, c, ptr_in(xb), P, ptr_in(dyb), P, ptr_in(dxb), P, acc, L.stream()), "pool bwd")
        got = to_nchw(dxb, c, off=PAD).double()
        if acc:     # one rounding of prev + g; S = |prev| + |g|
            assert_close(got, xd.grad + prev.double(), prev.double().abs() + xd.grad.abs(), dt, what + " bwd acc")
        else:
            assert torch.equal(got, xd.grad), what + " bwd routing"
        assert float(dxb[..., :PAD].float().abs().max()) == 0 and float(dxb[..., PAD + c:].float().abs().max()) == 0


@pytest.mark.parametrize("dt,c", dtc(widths))
def test_maxpool_widths(dt, c):
    """Part A: 3 x 6 x 10 (45 quads x G threads: a ragged single pass for every G), ties in every quad position."""
    maxpool_check(dt, 3, 6, 10, c, "maxpool C=%d" % c)


# ---------------------------------------------------------------------------------------------------------------------
# Upsample x2, bilinear, align_corners
# ---------------------------------------------------------------------------------------------------------------------
def upsample_ref(x, dy):
    """fp64 F.interpolate, its autograd, and the transposed interpolation of |dy| (S of the backward)"""
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=True)
    gx, = torch.autograd.grad(ref, xd, dy.double(), retain_graph=True)
    gabs, = torch.autograd.grad(ref, xd, dy.double().abs())
    return ref.detach(), gx, gabs


def upsample_check(dt, x, dy, prev, refs, what, accs=(0, 1)):
    n, c, h, w = x.shape
    ref, gx, gabs = refs
    P = c + 2 * PAD
    coord = max(2 * h, 2 * w)
    xb = in_buf(x, dt)
    yb = out_buf(n, 2 * h, 2 * w, c, dt)
    L.check(L.lib().nunet_upsample2x_fwd(dt, n, h, w, c, ptr_in(xb), P, ptr_in(yb), P, L.stream()), "up")
    assert_close(to_nchw(yb, c, off=PAD), ref, float(x.abs().max()), dt, what + " fwd", coord=coord)
    assert pad_untouched(yb, c)
    dyb = in_buf(dy, dt)
    for acc in accs:
        dxb = in_buf(prev, dt)
        L.check(L.lib().nunet_upsample2x_bwd(dt, n, h, w, c, ptr_in(dyb), P, ptr_in(dxb), P, acc, L.stream()), "up bwd")
        exp = gx + (prev.double() if acc else 0)
        S = gabs + (prev.double().abs() if acc else 0)
        assert_close(to_nchw(dxb, c, off=PAD), exp, S, dt, what + " bwd acc=%d" % acc, coord=coord)
        assert float(dxb[..., :PAD].float().abs().max()) == 0 and float(dxb[..., PAD + c:].float().abs().max()) == 0


def upsample_inputs(dt, n, h, w, c, seed=8):
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(n, c, h, w, generator=g), dt)
    dy = q(torch.randn(n, c, 2 * h, 2 * w, generator=g), dt)
    prev = q(torch.randn(n, c, h, w, generator=g), dt)
    return x, dy, prev


@pytest.mark.parametrize("dt,c", dtc(widths))
def test_upsample_widths(dt, c):
    """Part A: 3 x 6 x 10 at every width (H, W >= 4: the 5 x 5 window form of the backward), accumulate 0 and 1."""
    x, dy, prev = upsample_inputs(dt, 3, 6, 10, c)
    upsample_check(dt, x, dy, prev, upsample_ref(x, dy), "upsample C=%d" % c)


GEOM = sorted(set([(h, 4) for h in range(1, 131)] + [(4, w) for w in range(1, 131)] + [(97, 131), (256, 8), (8, 256)]))


@functools.lru_cache(maxsize=None)
def geom_case(h, w):
    """one set of inputs (8 channels, exact in bf16 and therefore in fp32 too) and one fp64 reference per shape,
    shared by both storage types; fp32 (EPV = 4) takes the first four channels"""
    x, dy, prev = upsample_inputs(L.BF16, 1, h, w, 8, seed=1000 * h + w)
    return (x, dy, prev) + upsample_ref(x, dy)


@pytest.mark.parametrize("dt", **dt_ids([L.F32, L.BF16]))
@pytest.mark.parametrize("hw", GEOM, ids=lambda hw: "%dx%d" % hw)
def test_upsample_geometry(dt, hw):
    """Part B: C = EPV, N = 1, every H in 1..130 at W = 4 and every W in 1..130 at H = 4, plus (97, 131), (256, 8), (8, 256).
    Extents 1..3 take the general loop of upsample_bwd_kernel, 4 and up the 5 x 5 window, whose base
    floorf((ic - 1) / sc) in fp32 is walked through every size (sc = (n - 1) / (2n - 1): (ic - 1) / sc lands next to an
    integer whenever (ic - 1)(2n - 1) is close to a multiple of n - 1)."""
    h, w = hw
    c = epv(dt)
    x, dy, prev, ref, gx, gabs = geom_case(h, w)
    upsample_check(dt, x[:, :c], dy[:, :c], prev[:, :c], (ref[:, :c], gx[:, :c], gabs[:, :c]), "upsample %dx%d" % hw, accs=(0,))


# ---------------------------------------------------------------------------------------------------------------------
# 1x1 heads
# ---------------------------------------------------------------------------------------------------------------------
KS = [1, 2, 3, 4, 8]


def head_fwd_check(dt, n, h, w, c, k, what, seed=9):
    g = torch.Generator().manual_seed(seed + k)
    x = q(torch.randn(n, c, h, w, generator=g), dt)
    wt = torch.randn(k, c, 1, 1, generator=g) * 0.2
    b = torch.randn(k, generator=g) * 0.1
    xb = in_buf(x, dt)
    logits = torch.full((n, k, h, w), 5.0, dtype=torch.float32, device=DEV)
    wt_g, b_g = wt.to(DEV), b.to(DEV)
    L.check(L.lib().nunet_head_fwd(dt, n, h, w, c, k, ptr_in(xb), c + 2 * PAD, L.ptr(wt_g), L.ptr(b_g), L.ptr(logits), L.stream()), "head")
    ref = F.conv2d(x.double(), wt.double(), b.double())
    S = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs())       # sum |x w| + |b|
    assert_close(logits.cpu(), ref, S, L.F32, what)


@pytest.mark.parametrize("k", KS, ids=lambda v: "K%d" % v)
@pytest.mark.parametrize("dt,c", dtc(lambda dt: (epv(dt), 32, 64)))
def test_head_fwd_widths(dt, c, k):
    """Part A: K in {1, 2, 3, 4, 8}; C = 32 (the network's), EPV (one vector per pixel) and 64 (the largest accepted: the
    s_w table is full at K = 8); 3 x 7 x 13 = 273 pixels: one full block and a ragged one, H W = 91 divides nothing."""
    head_fwd_check(dt, 3, 7, 13, c, k, "head_fwd C=%d K=%d" % (c, k))


@pytest.mark.parametrize("nslabs", [1, 3, 64], ids=lambda v: "nslabs%d" % v)
@pytest.mark.parametrize("k", KS, ids=lambda v: "K%d" % v)
@pytest.mark.parametrize("dt", **dt_ids(DTS))
def test_head_bwd(dt, k, nslabs):
    """Part A: C = 32, 3 x 23 x 29 = 2001 pixels. K = 3 and 8 take the generic instantiation (KT = 0), 1 / 2 / 4 their own.
    A pass covers U * nslabs * ppb pixels with ppb = 256 / G = 64 (16-bit) or 32 (fp32): 8 (16) passes at nslabs = 1,
    3 (6) ragged ones at 3; at 64 one ragged pass and blocks from ceil(2001 / ppb) = 32 (63) on idle. Every slab is
    overwritten (NaN sentinel), idle blocks' with zeros. dx = NULL, dx with accumulate 0 / 1, and the form with the
    fused BatchNorm-backward reduce, which must leave the same bits plus the sums of the tensor it completes."""
    n, h, w, c = 3, 23, 29, 32
    g = torch.Generator().manual_seed(90 + k)
    x = q(torch.randn(n, c, h, w, generator=g), dt)
    wt = torch.randn(k, c, 1, 1, generator=g) * 0.2
    dl = torch.randn(n, k, h, w, generator=g)
    prev = q(torch.randn(n, c, h, w, generator=g), dt)
    xd, wd_ = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    bd = torch.zeros(k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, wd_, bd).backward(dl.double())
    S0 = F.conv_transpose2d(dl.double().abs(), wt.double().abs())             # sum_k |dl_k w_k|
    xb = in_buf(x, dt)
    wt_g, dl_g = wt.to(DEV), dl.to(DEV)
    P = c + 2 * PAD
    ppb = 256 // (32 // epv(dt))
    first_idle = -(-n * h * w // ppb)

    def slabs_ok(slabs, what):
        assert not bool(torch.isnan(slabs).any()), what + ": a slab was not fully overwritten"
        if first_idle < nslabs:
            assert float(slabs[first_idle:].abs().max()) == 0.0, what + ": idle blocks store zeros"
        tot = slabs.double().sum(0).cpu()
        assert rel_err(tot[:k * c].view(k, c), wd_.grad.view(k, c)) < 1e-4, what
        assert rel_err(tot[k * c:], bd.grad) < 1e-4, what

    def run(dxb, acc, bnr=None):
        slabs = torch.full((nslabs, k * c + k), float("nan"), dtype=torch.float32, device=DEV)
        if bnr is None:
            L.check(L.lib().nunet_head_bwd(dt, n, h, w, c, k, ptr_in(xb), P, L.ptr(wt_g), L.ptr(dl_g),
                                           ptr_in(dxb) if dxb is not None else None, P, acc, L.ptr(slabs), nslabs, L.stream()), "head bwd")
        else:
            L.check(L.lib().nunet_head_bwd_bnr(dt, n, h, w, c, k, ptr_in(xb), P, L.ptr(wt_g), L.ptr(dl_g), ptr_in(dxb), P, acc,
                                               L.ptr(slabs), nslabs, C.byref(bnr), L.stream()), "head bwd bnr")
        return slabs

    s_null = run(None, 0)
    slabs_ok(s_null, "dx=NULL")
    for acc in (0, 1):
        what = "head_bwd K=%d nslabs=%d acc=%d" % (k, nslabs, acc)
        dxb = in_buf(prev, dt)
        s = run(dxb, acc)
        slabs_ok(s, what)
        assert torch.equal(s, s_null)
        exp = xd.grad + (prev.double() if acc else 0)
        assert_close(to_nchw(dxb, c, off=PAD), exp, S0 + (prev.double().abs() if acc else 0), dt, what + " dx")
        assert float(dxb[..., :PAD].float().abs().max()) == 0 and float(dxb[..., PAD + c:].float().abs().max()) == 0
        bnr, sums, keep = _bnr_setup(n, h, w, c, dt, g)
        dxb2 = in_buf(prev, dt)
        s2 = run(dxb2, acc, bnr)
        assert torch.equal(dxb2, dxb) and torch.equal(s2, s), what + " bnr"
        _bnr_check(dt, n, h, w, c, ptr_in(dxb2), P, sums, keep)


# ---------------------------------------------------------------------------------------------------------------------
# Part C: grids past their caps, second (ragged) passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,shape", [(512, (3, 100, 110)), (32, (3, 420, 417))], ids=["C512", "C32"])
def test_bn_relu_fwd_capped_grid(c, shape):
    """bn_relu_fwd_kernel<T, false>, bf16: the grid is ceil(pixels / (4 ppb)) capped at 2048, and a block's `while` body
    repeats once pixels > 2048 * 4 * ppb = 8192 ppb. C = 512: ppb = 4, 3 x 100 x 110 = 33000 > 32768, the second pass
    holds 232 pixels (58 of 2048 blocks, first load of the batch only). C = 32: ppb = 64, 3 x 420 x 417 = 525420 > 524288,
    1132 pixels in the second pass."""
    n, h, w = shape
    bn_fwd_run(bn_fwd_case(L.BF16, n, h, w, c, True, seed=12), False, False, "bn_fwd capped C=%d" % c)


def test_bn_relu_fwd_pooled_up_capped_grid():
    """bn_relu_fwd_kernel<T, true> with the upsample role, bf16, C = 512 (G = 64, ppb = 4), 3 x 150 x 148: the main role
    has ceil(quads / (2 ppb)) blocks capped at 2048 and steps 2048 * ppb = 8192 quads: 3 x 75 x 74 = 16650 quads > 16384,
    a third qload pass of 266 quads. The upsample role has ceil(4 pixels G / 2048) blocks capped at 1024 (2^21 outputs
    per pass): 4 * 66600 * 64 = 17049600 outputs, 65.04 passes of 262144 threads, the last one ragged."""
    bn_fwd_run(bn_fwd_case(L.BF16, 3, 150, 148, 512, True, seed=13), True, True, "bn_fwd pooled+up capped")


@pytest.mark.parametrize("dt,shape", [(L.BF16, (3, 100, 110)), (L.F32, (3, 50, 110))], ids=["bf16", "fp32"])
def test_bn_relu_bwd_capped_grid(dt, shape):
    """bn_relu_bwd_kernel, C = 512: grid ceil(pixels / (8 ppb)) capped at 512 (reduce) / 1024 (apply); a pass is
    4 * grid * ppb pixels, so the loop repeats once pixels > 2048 ppb (reduce) / 4096 ppb (apply) and the cap itself
    binds from 4096 ppb / 8192 ppb on. bf16: ppb = 4, 33000 pixels > 32768: reduce 4 passes of 8192 and one of 232,
    apply 2 of 16384 and one of 232. fp32: ppb = 2, 16500 pixels > 16384: reduce 4 x 4096 + 116, apply 2 x 8192 + 116."""
    n, h, w = shape
    bn_bwd_run(bn_bwd_case(dt, n, h, w, 512, seed=14), "bn_bwd capped")


def test_maxpool_capped_grid():
    """maxpool fwd / bwd, bf16, C = 512 (G = 64): grid_for caps at 4096 blocks = 2^20 threads; 3 x 50 x 118 quads x 64 =
    1132800 > 1048576: a second grid-stride pass of 84224 threads (329 blocks)."""
    maxpool_check(L.BF16, 3, 100, 236, 512, "maxpool capped", seed=15)


def test_upsample_fwd_capped_grid():
    """upsample_fwd, bf16, C = 128 (G = 16): 3 * 4 * 50 * 118 * 16 = 1132800 threads' worth > 2^20: second pass of 84224.
    (The backward at this shape runs below its cap; its own case follows.)"""
    x, dy, prev = upsample_inputs(L.BF16, 3, 50, 118, 128, seed=16)
    upsample_check(L.BF16, x, dy, prev, upsample_ref(x, dy), "upsample_fwd capped", accs=(0,))


def test_upsample_bwd_capped_grid():
    """upsample_bwd, bf16, C = 512 (G = 64): 3 * 50 * 118 * 64 = 1132800 > 2^20: second pass of 84224 threads; the forward
    at this shape is 4.3 passes."""
    x, dy, prev = upsample_inputs(L.BF16, 3, 50, 118, 512, seed=17)
    upsample_check(L.BF16, x, dy, prev, upsample_ref(x, dy), "upsample_bwd capped", accs=(1,))


def test_head_fwd_capped_grid():
    """head_fwd, bf16, C = 32, K = 2: one thread per pixel, 4096 blocks: 5 x 500 x 421 = 1052500 pixels > 2^20: a second
    pass of 3924 pixels (16 blocks, the last one ragged)."""
    head_fwd_check(L.BF16, 5, 500, 421, 32, 2, "head_fwd capped")


# ---------------------------------------------------------------------------------------------------------------------
# Part D: the edge of the fast index decode (make_dec4: fast while total * max(G, W, H) < 2^32) and the 64-bit path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 8], ids=["fast", "slow"])
def test_dec4_edge_upsample_fwd_and_fused(n):
    """upsample_fwd and the upsample role of bn_relu_fwd, bf16, C = 32 (G = 4), (N, 1, 4096): Dec4 over [N][2][8192][4],
    total = N * 2^16, max extent 8192 = 2^13: total * 2^13 = N * 2^29 < 2^32 for N = 7 (fast), = 2^32 for N = 8 (slow)."""
    x, dy, prev = upsample_inputs(L.BF16, n, 1, 4096, 32, seed=18)
    upsample_check(L.BF16, x, dy, prev, upsample_ref(x, dy), "dec4 upsample N=%d" % n, accs=(0,))
    bn_fwd_run(bn_fwd_case(L.BF16, n, 1, 4096, 32, True, seed=19), False, True, "dec4 bn_fwd+up N=%d" % n)


@pytest.mark.parametrize("dt,n", [(L.BF16, 15), (L.BF16, 16), (L.F32, 7), (L.F32, 8)], ids=["bf16-fast", "bf16-slow", "fp32-fast", "fp32-slow"])
def test_dec4_edge_maxpool(dt, n):
    """maxpool fwd / bwd, C = 32, (N, 2, 16384): Dec4 over [N][1][8192][G], max extent 2^13. bf16 (G = 4): total = N * 2^15,
    product N * 2^28: fast for N = 15, slow for N = 16. fp32 (G = 8): total = N * 2^16, product N * 2^29: fast 7, slow 8."""
    maxpool_check(dt, n, 2, 16384, 32, "dec4 maxpool N=%d" % n, seed=20)


@pytest.mark.parametrize("n", [3, 4], ids=["fast", "slow"])
def test_dec4_edge_upsample_bwd(n):
    """upsample_bwd, bf16, C = 32 (G = 4), (N, 4, 8192): Dec4 over [N][4][8192][4], total = N * 2^17, max extent 2^13:
    N * 2^30 < 2^32 for N = 3 (fast), = 2^32 for N = 4 (slow); H = 4 and W = 8192 take the 5 x 5 window, with the largest
    column coordinates of the file."""
    x, dy, prev = upsample_inputs(L.BF16, n, 4, 8192, 32, seed=21)
    upsample_check(L.BF16, x, dy, prev, upsample_ref(x, dy), "dec4 upsample_bwd N=%d" % n, accs=(0,))
