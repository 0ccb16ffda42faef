"""The weight-gradient kernel's operand transforms (nunet_wgrad_desc.x_tf / d_tf) and the plan paths built on them.

Op level: a transformed launch must leave the bits of the same launch on the tensor the transform replaces - the a1 the forward
conv side-stores (tf_store), the dy nunet_bn_relu_bwd_apply writes - so every comparison is torch.equal on the raw K-split slabs.
The geometries are the smallest at which the tiling can go wrong: stacked rows (2 x 12 x 12), regular tiling with ragged edge
tiles (1 x 20 x 24), three whole images (3 x 16 x 16). Plan level: one training step with dy formed by the input-gradient convs'
side stores against the same step with dy formed in the weight gradients' loaders."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import synth  # noqa: E402
from test_ops_gpu import DEV, conv_desc, nhwc, pack, q, tdt, wgrad_desc  # noqa: E402

NUNET_EINVAL = -1
GEOMS = [(2, 12, 12), (1, 20, 24), (3, 16, 16)]
DTS = [L.BF16, L.F16, L.F32]
CH = [(32, 32), (32, 64), (64, 32), (64, 64)]          # (Cin, Cout)


def dt_id(dt):
    return {L.F32: "fp32", L.BF16: "bf16", L.F16: "fp16"}[dt]


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer of a test sits between guard bands that are checked after it"""
    yield


def test_tiling_of_the_three_geometries():
    """the geometries reach what they are there for: stacked rows with a ragged last tile; regular tiling whose 10 x 12 tiles leave
    MFMA rows of the 128-pixel tile unused; several images of two tiles each - and more pixel tiles than the two K-slices the
    tests allow (problem()), so that every workgroup also loads and transforms tiles inside its loop"""
    def info(n, h, w):
        d = L.WgradDesc(); d.dtype = L.BF16; d.N = n; d.H = h; d.W = w; d.C0 = 32; d.P0 = 32; d.Cout = 32; d.PY = 32
        o = L.WgradLaunchInfo()
        L.check(L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)), "info")
        return o
    o = info(2, 12, 12)
    assert o.SH == 13 and o.nMT == 3 and (2 * 13) % o.TH
    o = info(1, 20, 24)
    assert o.SH == 0 and o.NI == 1 and o.TH * o.TW < 128 and o.nMT == 4
    o = info(3, 16, 16)
    assert o.SH == 0 and o.tilesG == 3 and o.nMT == 6


# ---------------------------------------------------------------------------------------------------------------------
# the two halves of a problem: an input operand (plain, or y1 with the a1 its forward conv side-stores) and a dY operand
# (dA and y with the dy / small vectors the stand-alone apply kernel writes)
# ---------------------------------------------------------------------------------------------------------------------
def x_plain(dt, n, h, w, c0, c1, seed):
    g = torch.Generator().manual_seed(seed)
    s0 = nhwc(q(torch.randn(n, c0, h, w, generator=g), dt), dt)
    s1 = nhwc(q(torch.randn(n, c1, h, w, generator=g), dt), dt) if c1 else None
    return {"s0": s0, "c0": c0, "s1": s1, "c1": c1}


def x_bn_relu(dt, n, h, w, c, seed):
    """y1 and relu(bn(y1)) as nunet_conv3x3_fwd(in_tf = NUNET_TF_BN_RELU, training) side-stores it; beta > 0 on the even channels
    (a transformed halo pixel would be relu(shift) != 0) and a negative shift on the odd ones (a missed ReLU would let negative
    values through): both kinds and both zeros and non-zeros in a1 are asserted on the inputs"""
    g = torch.Generator().manual_seed(seed)
    y1 = q(torch.randn(n, c, h, w, generator=g) * 0.8 + 0.3, dt)
    gamma = (1 + 0.2 * torch.rand(c, generator=g)).to(DEV)
    beta = torch.where(torch.arange(c) % 2 == 0, torch.tensor(0.9), torch.tensor(-0.6)).to(DEV)
    bias = (0.3 * torch.randn(c, generator=g)).to(DEV)
    yb = nhwc(y1, dt)
    dd = y1.double()
    stats = L.fx_encode(torch.cat([dd.sum((0, 2, 3)), (dd * dd).sum((0, 2, 3))]), c, DEV)
    wf, _ = pack(torch.randn(32, c, 3, 3, generator=g) / (3 * c ** 0.5), dt)
    out = torch.zeros((n, h, w, 32), dtype=tdt(dt), device=DEV)
    a1 = torch.full((n, h, w, c), 5.0, dtype=tdt(dt), device=DEV)
    save = torch.zeros(2 * c, dtype=torch.float32, device=DEV)
    d = conv_desc(dt, n, h, w, yb, c, c, wf, out, 32, 32)
    d.in_tf = L.TF_BN_RELU; d.tf_training = 1
    d.tf_fx = L.ptr(stats).value; d.tf_gamma = L.ptr(gamma).value; d.tf_beta = L.ptr(beta).value; d.tf_conv_bias = L.ptr(bias).value
    d.tf_mean_invstd = L.ptr(save).value; d.tf_momentum = 0.1; d.tf_eps = 1e-5
    d.tf_store = L.ptr(a1).value; d.tf_ps = c
    L.check(L.lib().nunet_conv3x3_fwd(C.byref(d), L.stream()), "conv + side store")
    torch.cuda.synchronize()
    shift = beta - save[:c] * gamma * save[c:]
    assert bool((shift > 0.1).any()) and bool((shift < -0.1).any()) and bool((beta > 0).any())
    assert bool((a1 == 0).any()) and bool((a1 != 0).any()) and bool((a1.float() >= 0).all())
    return {"s0": a1, "c0": c, "s1": None, "c1": 0, "y1": yb, "save": save, "gamma": gamma, "beta": beta}


def d_bn_bwd(dt, n, h, w, c, seed):
    """(dA, y) and the dy, d bias, d gamma, d beta nunet_bn_relu_bwd_apply forms from them; dA sits in a slot of a wider buffer"""
    g = torch.Generator().manual_seed(seed)
    y = q(torch.randn(n, c, h, w, generator=g), dt)
    da = q(torch.randn(n, c, h, w, generator=g), dt)
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(DEV)
    beta = (0.3 * torch.randn(c, generator=g)).to(DEV)
    mean = y.double().mean((0, 2, 3))
    istd = 1 / (y.double().var((0, 2, 3), unbiased=False) + 1e-5).sqrt()
    mi = torch.cat([mean, istd]).float().to(DEV)
    yb = nhwc(y, dt)
    dab = nhwc(da, dt, pitch=c + 32, off=32)
    da_ptr = L.ptr(dab, 32 * dab.element_size())
    sums = L.fx_zeros(c, DEV)
    vec = [torch.full((c,), 9.0, dtype=torch.float32, device=DEV) for _ in range(3)]      # d gamma, d beta, d bias
    dy = torch.zeros((n, h, w, c), dtype=tdt(dt), device=DEV)
    b = L.BnBwdDesc(dt, n, h, w, c, da_ptr, c + 32, L.ptr(yb), c, L.ptr(mi), L.ptr(gamma), L.ptr(beta), L.ptr(sums),
                    L.ptr(vec[0]), L.ptr(vec[1]), L.ptr(vec[2]), L.ptr(dy), c)
    L.check(L.lib().nunet_bn_relu_bwd_reduce(C.byref(b), L.stream()), "reduce")
    L.check(L.lib().nunet_bn_relu_bwd_apply(C.byref(b), L.stream()), "apply")
    torch.cuda.synchronize()
    assert float(dy.float().abs().max()) > 0 and bool((yb.float() * 0 == 0).all())
    return {"dy": dy, "c": c, "dab": dab, "da_ptr": da_ptr, "da_pitch": c + 32, "y": yb, "mi": mi, "gamma": gamma, "beta": beta,
            "sums": sums, "vec": vec}


def d_plain(dt, n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return {"dy": nhwc(q(torch.randn(n, c, h, w, generator=g), dt), dt), "c": c}


def problem(dt, geom, x, dd, xt, dtf, item_shape=0):
    """(descriptor, slabs, [d gamma, d beta, d bias] or None, keep-alive) of one weight-gradient problem: transformed
    operands where asked, the tensors the transforms replace otherwise"""
    n, h, w = geom
    cin, cout = x["c0"] + x["c1"], dd["c"]
    probe = wgrad_desc(dt, n, h, w, None, x["c0"], x["c0"], None, x["c1"], None, cout, None, 0, 0, item_shape)
    ks = min(L.lib().nunet_conv3x3_wgrad_slabs(C.byref(probe)), 2)     # two K-slices: 2 + 1, 2 + 2, 3 + 3 pixel tiles per workgroup
    slabs = torch.full((ks * 9 * cout * cin,), 1e30, dtype=torch.float32, device=DEV)
    d = wgrad_desc(dt, n, h, w, x["s0"], x["c0"], x["c0"], x["s1"], x["c1"], dd["dy"], cout, slabs, ks, 0, item_shape)
    vec = None
    if xt:
        d.src0 = L.ptr(x["y1"]).value; d.x_tf = L.TF_BN_RELU
        d.x_mean_invstd = L.ptr(x["save"]).value; d.x_gamma = L.ptr(x["gamma"]).value; d.x_beta = L.ptr(x["beta"]).value
    if dtf:
        vec = [torch.full((cout,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
        d.dy = dd["da_ptr"].value; d.PY = dd["da_pitch"]; d.d_tf = L.TF_BN_RELU_BWD
        d.d_y = L.ptr(dd["y"]).value; d.d_py = cout; d.d_sums = L.ptr(dd["sums"]).value
        d.d_mean_invstd = L.ptr(dd["mi"]).value; d.d_gamma = L.ptr(dd["gamma"]).value; d.d_beta = L.ptr(dd["beta"]).value
        d.d_dgamma = L.ptr(vec[0]).value; d.d_dbeta = L.ptr(vec[1]).value; d.d_dbias = L.ptr(vec[2]).value
    return d, slabs, vec


def single(d):
    L.check(L.lib().nunet_conv3x3_wgrad(C.byref(d), L.stream()), "wgrad")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("ch", CH, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%dx%d" % g)
def test_xt_equals_the_side_stored_activation(geom, ch, dt):
    cin, cout = ch
    x, dd = x_bn_relu(dt, *geom, cin, 3), d_plain(dt, *geom, cout, 4)
    d0, ref, _ = problem(dt, geom, x, dd, False, False)
    d1, got, _ = problem(dt, geom, x, dd, True, False)
    single(d0); single(d1)
    assert float(ref.abs().max()) < 1e29 and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("ch", CH + [((64, 32), 32)], ids=lambda c: "%sto%d" % c)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%dx%d" % g)
def test_dt_equals_the_stand_alone_apply_pass(geom, ch, dt):
    cin, cout = ch
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)       # 96 -> 32: two concat sources
    x, dd = x_plain(dt, *geom, c0, c1, 5), d_bn_bwd(dt, *geom, cout, 6)
    d0, ref, _ = problem(dt, geom, x, dd, False, False)
    d1, got, vec = problem(dt, geom, x, dd, False, True)
    single(d0); single(d1)
    assert float(ref.abs().max()) < 1e29 and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)
    for k in range(3):
        assert torch.equal(vec[k], dd["vec"][k])
    assert float(vec[2].abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("ch", CH, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%dx%d" % g)
def test_pair_dt_and_xt_dt_equals_the_untransformed_pair(geom, ch, dt):
    """problem a = conv1's (plain input, DT), problem b = conv2's (XT, DT): the form a VGGBlock's backward launches"""
    cin, f = ch
    xa, da = x_plain(dt, *geom, cin, 0, 7), d_bn_bwd(dt, *geom, f, 8)
    xb, db = x_bn_relu(dt, *geom, f, 9), d_bn_bwd(dt, *geom, f, 10)
    a0, ref_a, _ = problem(dt, geom, xa, da, False, False)
    b0, ref_b, _ = problem(dt, geom, xb, db, False, False)
    a1, got_a, vec_a = problem(dt, geom, xa, da, False, True)
    b1, got_b, vec_b = problem(dt, geom, xb, db, True, True)
    L.check(L.lib().nunet_conv3x3_wgrad_pair(C.byref(a0), C.byref(b0), L.stream()), "pair")
    L.check(L.lib().nunet_conv3x3_wgrad_pair(C.byref(a1), C.byref(b1), L.stream()), "pair, transformed")
    torch.cuda.synchronize()
    for ref in (ref_a, ref_b):
        assert float(ref.abs().max()) < 1e29 and float(ref.abs().max()) > 0
    assert torch.equal(got_a, ref_a) and torch.equal(got_b, ref_b)
    for vec, dd in ((vec_a, da), (vec_b, db)):
        for k in range(3):
            assert torch.equal(vec[k], dd["vec"][k])


@pytest.mark.parametrize("item_shape", [21, 12])
@pytest.mark.parametrize("tf", ["x_tf", "d_tf"])
def test_wide_items_refuse_a_transform(tf, item_shape):
    d = L.WgradDesc()
    d.dtype = L.BF16; d.N = 2; d.H = 16; d.W = 16; d.C0 = 64; d.P0 = 64; d.Cout = 64; d.PY = 64; d.d_py = 64
    d.item_shape = item_shape
    o = L.WgradLaunchInfo()
    assert L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == 0 and 10 * o.A + o.B == item_shape
    setattr(d, tf, L.TF_BN_RELU if tf == "x_tf" else L.TF_BN_RELU_BWD)
    assert L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == NUNET_EINVAL
    assert b"32 x 32" in L.lib().nunet_last_error()
    d.item_shape = 11
    assert L.lib().nunet_conv3x3_wgrad_launch_info(C.byref(d), C.byref(o)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# plan level
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_step(unet, dtype, dy_in_wgrad):
    """one SGD step of the eager module path at 2 x 3 x 32 x 32: gradients, parameters and BN buffers after it, the census"""
    n, h, w = 2, 32, 32
    st = synth.closed_form_state_unet(1, 3) if unet else synth.closed_form_state(1, 3, False, True)
    img, msk = synth.synth_batch(n, h, w, 3, 1, seed=1234)
    cls = nunet_amd.archs.UNet if unet else nunet_amd.archs.NestedUNet
    m = cls(1, 3, False, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.to(DEV).train()
    x, t = torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)
    pl = m.plan_for(x)
    pl.set_wgrad_dy(dy_in_wgrad)
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
    loss = nunet_amd.losses.BCEDiceLoss()(m(x), t)
    opt.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    r = {"grads": {k: p.grad.detach().clone() for k, p in m.named_parameters()}}
    r["census"] = (pl.census(False), pl.census(True))
    if dtype == "fp32" and not dy_in_wgrad:
        blocks = [(e.label.decode()[1], e.label.decode()[2]) for e in r["census"][0] if e.label.decode().endswith("conv2")]
        r["act1"] = {(int(i), int(j)): pl.block_act1(int(i), int(j)) for i, j in blocks}
        r["block00"] = [t.detach().cpu().double() for t in (m.conv0_0.conv1.weight, m.conv0_0.bn1.weight, m.conv0_0.bn1.bias)]
    opt.step()
    torch.cuda.synchronize()
    r["state"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return r


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("unet", [False, True], ids=["nested", "unet"])
def test_step_is_the_same_wherever_dy_is_formed(unet, dtype):
    a, b = plan_step(unet, dtype, False), plan_step(unet, dtype, True)
    assert a["grads"] and sorted(a["grads"]) == sorted(b["grads"])
    for k, g in a["grads"].items():
        assert torch.equal(g, b["grads"][k]), k
    assert float(max(g.abs().max() for g in a["grads"].values())) > 0
    for k, v in a["state"].items():
        assert torch.equal(v, b["state"][k]), k


@pytest.mark.parametrize("unet", [False, True], ids=["nested", "unet"])
def test_census_no_a1_store_no_stand_alone_apply(unet):
    for dy_in_wgrad in (False, True):
        fwd, bwd = plan_step(unet, "bf16", dy_in_wgrad)["census"]
        conv2 = [e for e in fwd if e.label.decode().endswith(".conv2")]
        assert len(conv2) == (9 if unet else 15)
        for e in fwd:
            assert e.kind == L.CENSUS_CONV and not e.has_tf_store, e.label      # no forward conv writes an a1
        assert not [e.label for e in bwd if b"bnA1" in e.label]
        wg = {e.label.decode(): e for e in bwd if e.kind == L.CENSUS_WGRAD_PAIR}
        assert len(wg) == len(conv2)
        for lab, e in wg.items():
            first = lab == "B00.wgrad"                                           # its conv1 has no input gradient: always DT
            assert e.wgrad_tf[0] == (2 if dy_in_wgrad or first else 0), lab
            assert e.wgrad_tf[1] == (3 if dy_in_wgrad else 1), lab
        for e in bwd:
            if e.kind == L.CENSUS_CONV:
                assert bool(e.has_tf_store) == (not dy_in_wgrad), e.label


@pytest.mark.parametrize("unet", [False, True], ids=["nested", "unet"])
def test_block_act1_is_the_stand_alone_bn_relu_of_y1(unet):
    """Plan.block_act1 after an fp32 forward + backward: every block's a1 is an activation of the right shape with zeros and
    non-zeros, and block (0, 0)'s - whose input is the image - equals relu(bn1(conv1(image))) evaluated in fp64"""
    r = plan_step(unet, "fp32", False)
    assert len(r["act1"]) == (9 if unet else 15)
    for (i, j), a1 in r["act1"].items():
        assert a1.shape == (2, 32 >> i, 32 >> i, (32, 64, 128, 256, 512)[i])
        assert bool((a1 >= 0).all()) and bool((a1 == 0).any()) and bool((a1 > 0).any())
    # block (0, 0): its input is the image, so a1 follows from the parameters alone
    img, _ = synth.synth_batch(2, 32, 32, 3, 1, seed=1234)
    w1, g1, b1 = r["block00"]
    y = torch.nn.functional.conv2d(torch.from_numpy(img).double(), w1, padding=1)
    ref = torch.relu(torch.nn.functional.batch_norm(y, None, None, g1, b1, True, 0.1, 1e-5))
    got = r["act1"][(0, 0)].permute(0, 3, 1, 2).cpu().double()
    assert float((got - ref).abs().max()) < 1e-4 * float(ref.abs().max())
