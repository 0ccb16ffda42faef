"""nunet_head_fwd_bn - BatchNorm2 + ReLU of a block output and its 1x1 head in one launch - against the two launches it
replaces, bit for bit; nunet_head_fwd against an fp64 dot product. Runs on the MI355X only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402,F401
from nunet_amd import _lib as L  # noqa: E402


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate sits between guard bands that are checked after the test (conftest.py)"""
    yield


DEV = "cuda:0"
C32, PITCH, SLOT = 32, 160, 4          # the network's level 0: five slots of 32 channels, the head's block writes the last
HEAD_TOL = 2e-5                        # tests/test_ops_gpu.py::test_head, relative to the largest |logit|


def tdt(dt):
    return L.TORCH_DTYPE[dt]


def launch_info(dt, n, h, w, c, with_bn):
    li = L.LossLaunchInfo()
    L.check(L.lib().nunet_head_launch_info(dt, n, h, w, c, with_bn, C.byref(li)), "head_launch_info")
    return li


def bits(t):
    """the tensor's bytes (NaN-filled regions compare equal as bytes)"""
    return t.contiguous().view(torch.uint8)


class Case:
    """A raw conv output y with exact batch sums, BatchNorm parameters and running statistics, K heads' weights."""

    def __init__(self, dt, n, h, w, kmax, seed):
        g = torch.Generator().manual_seed(seed)
        c = C32
        self.dt, self.n, self.h, self.w = dt, n, h, w
        y = (torch.randn(n, h, w, c, generator=g) * 0.7).to(tdt(dt))
        self.y = torch.empty((n, h, w, c), dtype=tdt(dt), device=DEV)
        self.y.copy_(y)
        dd = y.double()
        self.stats = L.fx_encode(torch.cat([dd.sum((0, 1, 2)), (dd * dd).sum((0, 1, 2))]), c, DEV)
        self.bias = (torch.randn(c, generator=g) * 0.3).to(DEV)
        self.gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(DEV)
        self.beta = (0.2 * torch.randn(c, generator=g)).to(DEV)
        self.rm = 0.1 * torch.randn(c, generator=g)
        self.rv = 0.5 + torch.rand(c, generator=g)
        self.wt = (torch.randn(kmax, c, generator=g) * 0.2)
        self.b = (torch.randn(kmax, generator=g) * 0.1)

    def run(self, fused, k, training, running=True):
        """-> (logits, slot buffer, saved mean|invstd, running mean, running var, num_batches_tracked), every output NaN-filled first"""
        n, h, w, c, dt = self.n, self.h, self.w, C32, self.dt
        nan = float("nan")
        slot = torch.full((n, h, w, PITCH), nan, dtype=tdt(dt), device=DEV)
        logits = torch.full((n, k, h, w), nan, dtype=torch.float32, device=DEV)
        save = torch.full((2 * c,), nan, dtype=torch.float32, device=DEV)
        rm, rv = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rm.copy_(self.rm)
        rv.copy_(self.rv)
        nbt = torch.full((1,), 4, dtype=torch.int64, device=DEV)
        wt = torch.empty((k, c), device=DEV)
        wt.copy_(self.wt[:k])
        b = torch.empty(k, device=DEV)
        b.copy_(self.b[:k])
        es = slot.element_size()
        a = L.ptr(slot, SLOT * c * es)
        d = L.BnFwdDesc(dt, n, h, w, c, L.ptr(self.y), c, L.ptr(self.bias), L.ptr(self.stats), L.ptr(self.gamma), L.ptr(self.beta),
                        L.ptr(rm) if running else None, L.ptr(rv) if running else None, L.ptr(nbt) if running else None,
                        L.ptr(save), 1 if training else 0, 0.1, 1e-5, a, PITCH, None, 0, None, 0)
        if fused:
            L.check(L.lib().nunet_head_fwd_bn(C.byref(d), k, L.ptr(wt), L.ptr(b), L.ptr(logits), L.stream()), "head_fwd_bn")
        else:
            L.check(L.lib().nunet_bn_relu_fwd(C.byref(d), L.stream()), "bn_relu_fwd")
            L.check(L.lib().nunet_head_fwd(dt, n, h, w, c, k, a, PITCH, L.ptr(wt), L.ptr(b), L.ptr(logits), L.stream()), "head_fwd")
        torch.cuda.synchronize()
        return logits, slot, save, rm, rv, nbt


def assert_same(case, k, training, running=True):
    two = case.run(False, k, training, running)
    one = case.run(True, k, training, running)
    names = ("logits", "slot buffer", "saved mean | invstd", "running_mean", "running_var", "num_batches_tracked")
    for name, a, b in zip(names, one, two):
        assert torch.equal(bits(a), bits(b)), (name, k, training, running)
    logits, slot = one[0], one[1]
    assert bool(torch.isfinite(logits).all())
    live = slot[..., SLOT * C32:(SLOT + 1) * C32]
    assert bool(torch.isfinite(live.float()).all()) and bool(torch.isnan(slot[..., :SLOT * C32].float()).all())   # the other four slots: untouched
    assert int(one[5].item()) == (5 if training and running else 4)


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 16, 48), (2, 32, 32)])
def test_head_fwd_bn_equals_the_two_launches(dt, training, shape):
    """Logits, the slot (pitch 160, slot 4), saved statistics, running statistics and num_batches_tracked, bit for bit, for
    K = 1 (the compile-time class count), 2, 4 and 5 (the run-time one). At (2, 32, 32) a lane group walks four pixels - read
    from the launch's own grid formula - and at (1, 16, 16) and (3, 16, 48) the last pass of a workgroup is partly idle."""
    n, h, w = shape
    li = launch_info(dt, n, h, w, C32, 1)
    if shape == (2, 32, 32):
        assert li.trips_max == 4 and li.trips_min == 4, (li.grid_x, li.trips_max, li.trips_min)
    case = Case(dt, n, h, w, 5, seed=11 + n)
    for k in (1, 2, 4, 5):
        assert_same(case, k, training)
    if training:
        assert_same(case, 1, 1, running=False)      # a BatchNorm without running statistics


def test_head_fwd_bn_second_loop_pass():
    """More pixels than one loop pass of the capped grid covers (four per lane group): a lane group walks more than four - asserted
    from the launch's grid formula."""
    dt, n, h, w = L.BF16, 2, 512, 528
    li = launch_info(dt, n, h, w, C32, 1)
    assert li.trips_max > 4, (li.grid_x, li.trips_max)
    assert_same(Case(dt, n, h, w, 1, seed=5), 1, 1)


def test_head_fwd_bn_refuses_pool_and_upsample():
    case = Case(L.BF16, 1, 16, 16, 1, seed=3)
    n, h, w, c = 1, 16, 16, C32
    slot = torch.zeros((n, h, w, c), dtype=torch.bfloat16, device=DEV)
    other = torch.zeros((n, 2 * h, 2 * w, c), dtype=torch.bfloat16, device=DEV)
    logits = torch.zeros((n, 1, h, w), device=DEV)
    save = torch.zeros(2 * c, device=DEV)
    wt, b = torch.zeros((1, c), device=DEV), torch.zeros(1, device=DEV)
    for pooled, up in ((other, None), (None, other)):
        d = L.BnFwdDesc(L.BF16, n, h, w, c, L.ptr(case.y), c, L.ptr(case.bias), L.ptr(case.stats), L.ptr(case.gamma), L.ptr(case.beta),
                        None, None, None, L.ptr(save), 1, 0.1, 1e-5, L.ptr(slot), c, L.ptr(pooled), c, L.ptr(up), c)
        assert L.lib().nunet_head_fwd_bn(C.byref(d), 1, L.ptr(wt), L.ptr(b), L.ptr(logits), L.stream()) == -1      # NUNET_EINVAL
    torch.cuda.synchronize()
    assert float(logits.abs().max()) == 0 and float(slot.float().abs().max()) == 0


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16])
@pytest.mark.parametrize("c", [32, 64, 16])
def test_head_fwd_against_fp64(dt, c):
    """The stand-alone head (the unrolled C = 32 form and the general one) against an fp64 dot product of the stored values."""
    n, h, w = 3, 16, 48
    g = torch.Generator().manual_seed(9 + c)
    pitch = 5 * c
    for k in (1, 2, 4, 5):
        x = torch.full((n, h, w, pitch), float("nan"), dtype=tdt(dt), device=DEV)
        xs = torch.randn(n, h, w, c, generator=g).to(tdt(dt))
        x[..., 4 * c:] = xs.to(DEV)
        wt = torch.randn(k, c, generator=g) * 0.2
        b = torch.randn(k, generator=g) * 0.1
        wt_g, b_g = torch.empty((k, c), device=DEV), torch.empty(k, device=DEV)
        wt_g.copy_(wt)
        b_g.copy_(b)
        logits = torch.full((n, k, h, w), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.lib().nunet_head_fwd(dt, n, h, w, c, k, L.ptr(x, 4 * c * x.element_size()), pitch, L.ptr(wt_g), L.ptr(b_g),
                                       L.ptr(logits), L.stream()), "head_fwd")
        ref = F.conv2d(xs.double().permute(0, 3, 1, 2), wt.double().view(k, c, 1, 1), b.double())
        err = float((logits.cpu().double() - ref).abs().max() / ref.abs().max())
        assert err < HEAD_TOL, (c, k, err)


def test_head_fwd_grid_stride():
    """Past the grid cap a thread of the stand-alone head walks more than one pixel (from the launch's grid formula)."""
    dt, n, h, w, c, k = L.BF16, 2, 528, 1024, C32, 1
    li = launch_info(dt, n, h, w, c, 0)
    assert li.trips_max > 1, (li.grid_x, li.trips_max)
    g = torch.Generator().manual_seed(2)
    xs = torch.randn(n, h, w, c, generator=g).to(tdt(dt))
    x = torch.empty((n, h, w, c), dtype=tdt(dt), device=DEV)
    x.copy_(xs)
    wt, b = torch.randn(k, c, generator=g) * 0.2, torch.randn(k, generator=g) * 0.1
    wt_g, b_g = torch.empty((k, c), device=DEV), torch.empty(k, device=DEV)
    wt_g.copy_(wt)
    b_g.copy_(b)
    logits = torch.full((n, k, h, w), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().nunet_head_fwd(dt, n, h, w, c, k, L.ptr(x), c, L.ptr(wt_g), L.ptr(b_g), L.ptr(logits), L.stream()), "head_fwd")
    ref = (x.double() @ wt_g.double().t() + b_g.double()).permute(0, 3, 1, 2)       # fp64, on the device
    err = float((logits.double() - ref).abs().max() / ref.abs().max())
    assert err < HEAD_TOL, err
