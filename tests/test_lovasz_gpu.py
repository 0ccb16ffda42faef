"""The Lovasz-hinge kernels (csrc/lovasz.hip) against oracle.lovasz_hinge in fp64, per pixel, on the tie-free cases of
tests/lovasz_cases.py (pinned on the CPU by tests/test_lovasz_cpu.py): the in-LDS kernel from one pixel to the LDS limit, the
global-memory pipeline from two chunks to the 512 x 512 workload geometry, both mean kernels past one wave of entries, the
degenerate label patterns, inputs with ties, the raw C entry on poisoned buffers and the fused nunet_loss_step.

The gradient criterion is rtol = 1e-6 with atol = 0 on every pixel whose fp64 gradient is nonzero, and exactly 0.0 elsewhere.
The kernels form the Jaccard increment as 1 / U_k at a positive (and at k = 1) and I_k / (U_{k-1} U_k) at a negative, with
I = gts - cum and U = gts + k - cum exact integers in fp32: one or two roundings, then the 1/N multiply and the upstream
scale, where differencing two Jaccard values near 1 left 1e-7 of absolute noise on increments as small as 1e-9.

The worst relative error measured per shape, before and after that change, is in test_gradient_per_pixel's docstring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
import lovasz_cases as LC  # noqa: E402

DEV = "cuda:0"
RTOL = 1e-6


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate - the loss module's workspace included - sits between guard bands that are
    checked after the test (conftest.py)"""
    yield


def loss_close(got, ref):
    assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (got, ref)


def check_gradient(got, ref, what):
    """got: device result as an fp64 array, ref: the oracle's. Prints the worst relative error before it asserts."""
    nz = ref != 0
    print("%s: worst relative gradient error %.3e over %d nonzero pixels; %d pixels exactly zero" % (what, LC.worst_rel(got, ref), int(nz.sum()), int((~nz).sum())))
    assert not got[~nz].any(), "%s: %d pixels are nonzero where the fp64 gradient is exactly 0" % (what, int((got[~nz] != 0).sum()))
    np.testing.assert_allclose(got[nz], ref[nz], rtol=RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_gradient_per_pixel(case):
    """LovaszHingeLoss forward and backward. (1, 512, 512) backpropagates through loss * 0.37: the backward scale kernel's
    grid-stride loop with a seed that is not 1.

    Worst relative gradient error over the nonzero pixels, differencing kernels -> these kernels, measured on an MI355X
    (30 % positives unless a pattern is named):
        (3, 24, 40)    2.66e-4 -> 1.19e-7        (2, 128, 128)  5.29e-3 -> 1.15e-7        (2, 128, 256)  1.07e-2 -> 1.14e-7
        (1, 512, 512)  8.30e-2 -> 1.53e-7        (130, 8, 8)    2.44e-5 -> 1.08e-7
        (3, 24, 40) zero_one 2.42e-4 -> 1.15e-7, one_top 2.98e-8 -> 2.98e-8, one_bottom 1.48e-2 -> 1.19e-7,
        half_free 3.54e-4 -> 1.19e-7, all_nonpos 0 -> 0;  nunet_loss_step, (2, 1, 16385), head 0: 4.92e-3 -> 1.13e-7
    The [N, 1, W] shapes have no device figure yet. An fp32 evaluation of both formulas on the CPU, which reproduced every
    device figure above to three digits, gives for them:
        (2, 1, 1) 0 -> 0    (2, 1, 2) 0 -> 0    (3, 1, 63) 1.87e-5 -> 1.08e-7    (2, 1, 2047) 6.93e-4 -> 5.91e-8
        (2, 1, 2048) 5.58e-4 -> 5.84e-8    (2, 1, 2049) 5.69e-4 -> 5.83e-8    (2, 1, 16383) 5.18e-3 -> 1.13e-7
        (2, 1, 16385) 4.92e-3 -> 1.13e-7    (1, 1, 65537) 2.26e-2 -> 1.07e-7    (33, 1, 16385) 5.93e-3 -> 1.95e-7
        (2, 1, 16385) zero_one 9.16e-4 -> 3.73e-9, one_top 0 -> 0, one_bottom 5.26 -> 8.90e-8, half_free 7.09e-3 -> 1.13e-7"""
    shape, pattern = case
    x, t, _ = LC.build(shape, pattern)
    ref_loss, ref_dx = LC.reference(shape, pattern)
    seed = 0.37 if shape == (1, 512, 512) else 1.0
    xd = x.unsqueeze(1).to(DEV).requires_grad_(True)             # [N, 1, H, W], as the network's head hands it over
    loss = nunet_amd.losses.LovaszHingeLoss()(xd, t.unsqueeze(1).to(DEV))
    (loss * seed).backward()
    loss_close(float(loss.detach()), ref_loss)
    got = xd.grad.cpu().double().reshape(shape[0], -1).numpy()
    check_gradient(got, ref_dx.numpy() * seed, LC.case_id(case))
    if pattern == "all_nonpos":
        assert float(loss.detach()) == 0.0 and not got.any()


@pytest.mark.parametrize("kind", ["init", "quarter"])
@pytest.mark.parametrize("shape", LC.TIE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_ties_keep_group_sums_and_signs(shape, kind):
    """With equal errors the per-pixel subgradient depends on the sort order inside a tie group; the sum of |dx| over a
    group (the Jaccard difference across it, over N) and the sign of every entry do not."""
    x, t = LC.build_ties(shape, kind)
    ref_loss, ref_dx = LC.reference_ties(shape, kind)
    xd = x.unsqueeze(1).to(DEV).requires_grad_(True)             # [N, 1, H, W], as the network's head hands it over
    loss = nunet_amd.losses.LovaszHingeLoss()(xd, t.unsqueeze(1).to(DEV))
    loss.backward()
    loss_close(float(loss.detach()), ref_loss)
    n = shape[0]
    got = xd.grad.cpu().double().reshape(n, -1).numpy()
    ref = ref_dx.numpy()
    tt = t.reshape(n, -1).numpy()
    e = 1.0 - x.reshape(n, -1).double().numpy() * (2.0 * tt - 1.0)
    assert np.array_equal(np.sign(got)[got != 0], -(2.0 * tt - 1.0)[got != 0])
    for i in range(n):
        vals, inv = np.unique(e[i], return_inverse=True)
        gs = np.bincount(inv, weights=np.abs(got[i]), minlength=vals.size)
        rs = np.bincount(inv, weights=np.abs(ref[i]), minlength=vals.size)
        print("%s %s image %d: %d tie groups, worst relative group-sum error %.3e" % (shape, kind, i, vals.size, LC.worst_rel(gs, rs)))
        np.testing.assert_allclose(gs, rs, rtol=1e-5, atol=0)


def _raw_fwd(x, t, ws_fill, dx_fill, slack=4096):
    """nunet_lovasz_hinge_fwd on a workspace and a gradient buffer over-allocated by `slack` bytes, called twice
    -> per call (loss, gradient with its tail, workspace tail)"""
    lib = L.lib()
    n, per = x.shape[0], x[0].numel()
    need = lib.nunet_lovasz_ws_bytes(n, per)
    ws = torch.full((need + slack,), ws_fill, dtype=torch.uint8, device=DEV)
    dx = torch.full((n * per + slack // 4,), dx_fill, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), dx_fill, dtype=torch.float32, device=DEV)
    out = []
    for _ in range(2):
        L.check(lib.nunet_lovasz_hinge_fwd(L.ptr(x), L.ptr(t), n, per, L.ptr(ws), need, L.ptr(dx), L.ptr(loss), L.stream()), "nunet_lovasz_hinge_fwd")
        torch.cuda.synchronize()
        out.append((loss.cpu().clone(), dx.cpu().clone(), ws[need:].cpu().clone()))
    return out


@pytest.mark.parametrize("shape", LC.TIE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_raw_entry_reads_nothing_it_did_not_write(shape):
    """A workspace of 0xFF bytes and a gradient buffer of NaN give bit for bit what zeroed buffers give, every gradient entry is
    written, nothing past the stated sizes is touched, and a second call on the same buffers repeats the first exactly (no
    float atomics, nothing carried over in the workspace)."""
    x, t, _ = LC.build(shape, "p30")
    n, per = shape[0], shape[1] * shape[2]
    xd, td = x.to(DEV).contiguous(), t.to(DEV).contiguous()
    clean = _raw_fwd(xd, td, 0, 0.0)
    dirty = _raw_fwd(xd, td, 0xFF, float("nan"))
    bits = lambda a: a.view(torch.int32)
    for loss, dx, ws_tail in dirty:
        assert torch.equal(bits(loss), bits(clean[0][0]))
        assert torch.equal(bits(dx[:n * per]), bits(clean[0][1][:n * per]))
        assert bool(torch.isfinite(dx[:n * per]).all())
        assert bool((bits(dx[n * per:]) == bits(torch.full((1,), float("nan")))).all())
        assert bool((ws_tail == 0xFF).all())
    for loss, dx, ws_tail in clean:
        assert torch.equal(bits(loss), bits(clean[0][0])) and torch.equal(bits(dx), bits(clean[0][1]))
        assert not dx[n * per:].any() and not ws_tail.any()


def test_fused_loss_step_per_pixel():
    """nunet_loss_step with the Lovasz hinge, two heads on one target, against the fp64 oracle (the stand-alone entry is not
    the reference here): loss per head, their mean, and d mean / d logits per pixel at the same rtol."""
    shape, heads = LC.FUSED_SHAPE, LC.FUSED_HEADS
    n, per = shape[0], shape[1] * shape[2]
    cases = [LC.build(shape, "p30", q, ("p30", 0)) for q in range(heads)]
    refs = [LC.reference(shape, "p30", q, ("p30", 0)) for q in range(heads)]
    assert all(torch.equal(c[1], cases[0][1]) for c in cases)
    lib = L.lib()
    xd = torch.stack([c[0].reshape(n, per) for c in cases]).to(DEV).contiguous()
    td = cases[0][1].reshape(n, per).to(DEV).contiguous()
    ws = torch.full(((lib.nunet_loss_step_ws_bytes(n, per, heads, L.LOSS_LOVASZ_HINGE) + 7) // 8 * 8,), 0xFF, dtype=torch.uint8, device=DEV)
    dl = torch.full((heads, n, per), float("nan"), device=DEV)
    lo = torch.zeros(heads + 1, device=DEV)
    L.check(lib.nunet_loss_step(L.ptr(xd), L.ptr(td), n, per, heads, L.LOSS_LOVASZ_HINGE, L.ptr(ws), L.nbytes(ws), L.ptr(dl), L.ptr(lo), None,
                                nunet_amd.metrics.iou_logit_threshold(), L.stream()), "nunet_loss_step")
    got_l = lo.tolist()
    for q in range(heads):
        loss_close(got_l[q], refs[q][0])
        check_gradient(dl[q].cpu().double().numpy(), refs[q][1].numpy() / heads, "loss_step head %d" % q)
    loss_close(got_l[heads], sum(r[0] for r in refs) / heads)
