"""The BCE-Dice loss (stand-alone and inside nunet_loss_step), the IoU counts and the mask export of csrc/loss.hip
against fp64 / the host expressions, in every launch regime of their grid-stride loops. The cases, the fp64 reference and the
per-pixel gradient bound are those of tests/loss_cases.py (pinned on the CPU by tests/test_bce_dice_cpu.py); every case first
asserts, from the library's own nunet_loss_launch_info, the regime it is named for - blocks per image, the most grid-stride
trips of a thread and the spread down to the fewest - so a case that no longer reaches its regime fails.

The gradient criterion is loss_cases' bound with c = 4 on every pixel: twice what the fp32 emulation on the CPU is held to
(c = 2), for a device expf, log1pf or reciprocal an ulp off the host's. The smallest c each case needs is printed before it is
asserted; the figures measured on an MI355X stand in the docstrings of test_standalone_raw_entries and test_fused_step."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
import loss_cases as LC  # noqa: E402

DEV = "cuda:0"
C_DEVICE = 4.0
NAN = float("nan")


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate with a torch factory - the loss module's workspace included - sits between
    guard bands that are checked after the test (conftest.py)"""
    yield


def bits(a):
    return a.view(torch.int32)


def launch_info(entry, n, per_or_n, heads=1):
    info = L.LossLaunchInfo()
    L.check(L.lib().nunet_loss_launch_info(entry, n, per_or_n, heads, C.byref(info)), "nunet_loss_launch_info")
    return info


def assert_regime(entries, claim, n, per_or_n, heads=1):
    """claim = (gx, most trips, fewest trips) as the case list states it; the library answers from the launch's own expressions"""
    for entry in entries:
        i = launch_info(entry, n, per_or_n, heads)
        got = (i.grid_x, i.trips_max, i.trips_max - i.trips_min)
        assert got == (claim[0], claim[1], claim[1] - claim[2]), (entry, got, claim)
        assert (i.grid_y, i.grid_z, i.block) == (n, heads, 256)


def loss_close(got, ref):
    assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (got, ref, got - ref)


def check_gradient(got, case, k, what, factor=1.0):
    """got: device gradient [N, per] of head k; every pixel within factor * bound(c = 4). -> the smallest c that passes"""
    assert bool(torch.isfinite(got).all()), "%s: gradient entries left unwritten or not finite" % what
    ratio = LC.worst_ratio(got.cpu().double(), LC.reference(case, k)[1], LC.unit_of(case, k), factor)
    print("%s: needs c = %.3f" % (what, ratio))
    assert ratio <= C_DEVICE, "%s: c = %.3f" % (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# stand-alone BCE-Dice
# ---------------------------------------------------------------------------------------------------------------------------
ALONE_ENTRIES = (L.LOSS_ENTRY_BCE_DICE_FWD, L.LOSS_ENTRY_BCE_DICE_BWD)


@pytest.mark.parametrize("case", LC.ALONE_CASES, ids=LC.case_id)
def test_standalone_module(case):
    """nunet_amd.losses.BCEDiceLoss, forward and backward (its workspace comes from torch.empty)"""
    _, n, per, _, _ = case
    assert_regime(ALONE_ENTRIES, LC.REGIME[case], n, per)
    x, t = LC.build(case)
    xd = x.to(DEV).requires_grad_(True)
    loss = nunet_amd.losses.BCEDiceLoss()(xd, t.to(DEV))
    loss.backward()
    print("%s: loss - ref = %.2e" % (LC.case_id(case), float(loss.detach()) - LC.reference(case)[0]))
    loss_close(float(loss.detach()), LC.reference(case)[0])
    check_gradient(xd.grad, case, 0, "module " + LC.case_id(case))


def test_standalone_module_takes_4d_and_non_contiguous_inputs():
    """[N, 4, h, w] as a four-class head hands it over, and the same values as a non-contiguous view (the wrapper copies): the
    loss and the gradient are those of [N, per]"""
    case = ("alone", 3, 2240, 1, "rand")
    x, t = LC.build(case)
    shape = (3, 4, 20, 28)
    crit = nunet_amd.losses.BCEDiceLoss()
    xd = x.reshape(shape).to(DEV).requires_grad_(True)
    loss = crit(xd, t.reshape(shape).to(DEV))
    loss.backward()
    loss_close(float(loss.detach()), LC.reference(case)[0])
    check_gradient(xd.grad.reshape(3, -1), case, 0, "[N, 4, h, w]")
    leaf = x.reshape(shape).transpose(2, 3).contiguous().to(DEV).requires_grad_(True)      # stored [N, 4, w, h]
    tv = t.reshape(shape).transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
    view = leaf.transpose(2, 3)
    assert not view.is_contiguous() and not tv.is_contiguous() and torch.equal(view.detach().cpu(), x.reshape(shape))
    loss2 = crit(view, tv)
    loss2.backward()
    assert torch.equal(bits(loss2.detach().reshape(1)), bits(loss.detach().reshape(1)))
    assert torch.equal(bits(leaf.grad.transpose(2, 3).contiguous()), bits(xd.grad))


def _raw_alone(xd, td, poison, gscale=None):
    """nunet_bce_dice_fwd + _bwd on a workspace of exactly the stated size, with the workspace, the loss and the gradient filled
    with `poison` beforehand -> (loss [1], workspace head [3 N + 1], dx [N, per])"""
    lib = L.lib()
    n, per = xd.shape
    need = lib.nunet_bce_dice_ws_bytes(n)
    assert need % 4 == 0
    ws = torch.full((need // 4,), poison, device=DEV)
    loss, dx = torch.full((1,), poison, device=DEV), torch.full((n, per), poison, device=DEV)
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    L.check(lib.nunet_bce_dice_fwd(L.ptr(xd), L.ptr(td), n, per, L.ptr(ws), need, L.ptr(loss), L.stream()), "nunet_bce_dice_fwd")
    L.check(lib.nunet_bce_dice_bwd(L.ptr(xd), L.ptr(td), n, per, L.ptr(ws), need, L.ptr(gs), L.ptr(dx), L.stream()), "nunet_bce_dice_bwd")
    torch.cuda.synchronize()
    return loss, ws[:3 * n + 1].clone(), dx


@pytest.mark.parametrize("case", LC.ALONE_CASES, ids=LC.case_id)
def test_standalone_raw_entries(case):
    """The C entries on NaN-filled buffers: the loss, the per-image sums the workspace documents (ws[3 n .. 3 n + 2] = I, P, T,
    include/nunet.h), every pixel of the gradient, the upstream scales 0.25 (the bits of the unscaled gradient times 0.25) and
    0.37, and a second run on a differently poisoned workspace (bit-identical: no slab is read that no block wrote).

    The smallest c each case needs, MI355X | the fp32 emulation on the CPU (test_bce_dice_cpu.py):
    (N x per, "rand" unless a pattern is named)
        2x1 0.000 | 0.000        3x255 0.569 | 0.569      2x1025 1.030 | 1.072      3x2240 1.143 | 1.143
        2x65536 1.371 | 1.377    2x65537 1.319 | 1.319    1x1048579 1.440 | 1.441   33x300 1.176 | 1.168
        3x9216: empty_full 1.308 | 1.308, saturated 0.000 | 0.000, wide 1.406 | 1.405, beyond_exp 1.179 | 1.187,
        soft 1.303 | 1.303, zeros 0.000 | 0.000
    (gscale 0.37: within 0.01 of these.) The worst |loss - ref| / max(1, |ref|) was 1.0e-7 (1.8e-6 on the loss of 19.8 of "beyond_exp"), against the 2e-6 allowed;
    the worst relative error of a per-image sum 1.3e-7 (I of 1x1048579)."""
    _, n, per, _, _ = case
    assert_regime(ALONE_ENTRIES, LC.REGIME[case], n, per)
    x, t = LC.build(case)
    ref_loss, _, I, P, T = LC.reference(case)
    xd, td = x.to(DEV), t.to(DEV)
    loss, head, dx = _raw_alone(xd, td, NAN)
    print("%s: loss - ref = %.2e" % (LC.case_id(case), float(loss) - ref_loss))
    loss_close(float(loss), ref_loss)
    sums = head[:3 * n].cpu().double().reshape(n, 3)
    tiny = 2.0 ** -126 * per
    for col, (ref, atol) in enumerate(((I, tiny), (P, tiny), (T, 0.0))):
        err = (sums[:, col] - ref).abs()
        print("  %s: worst relative error %.2e" % ("IPT"[col], float((err / ref.abs().clamp(min=1e-300)).max())))
        assert bool((err <= 2e-6 * ref.abs() + atol).all()), ("IPT"[col], sums[:, col], ref)
    check_gradient(dx, case, 0, "raw " + LC.case_id(case))
    # upstream scales
    _, _, dx25 = _raw_alone(xd, td, NAN, 0.25)
    normal = dx.abs() >= 2.0 ** -100
    assert torch.equal(bits(dx25)[normal], bits(dx * 0.25)[normal]) and bool(torch.isfinite(dx25).all())
    _, _, dx37 = _raw_alone(xd, td, NAN, 0.37)
    check_gradient(dx37, case, 0, "raw, gscale 0.37, " + LC.case_id(case), 0.37)
    # another poison
    loss2, head2, dx2 = _raw_alone(xd, td, 1e30)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(head2), bits(head)) and torch.equal(bits(dx2), bits(dx))


# ---------------------------------------------------------------------------------------------------------------------------
# fused loss step
# ---------------------------------------------------------------------------------------------------------------------------
def _step(xd, td, poison, meters, scale=None, calls=1):
    """nunet_loss_step (or _scaled, with `scale` on the device) with the BCE-Dice loss on a poisoned workspace of exactly the
    stated size -> (loss_out [heads + 1], dx [heads, N, per])"""
    lib = L.lib()
    heads, n, per = xd.shape
    need = lib.nunet_loss_step_ws_bytes(n, per, heads, L.LOSS_BCE_DICE)
    assert need % 4 == 0 and need > 0
    ws = torch.full((need // 4,), poison, device=DEV)
    dl, lo = torch.full((heads, n, per), poison, device=DEV), torch.full((heads + 1,), poison, device=DEV)
    thr = nunet_amd.metrics.iou_logit_threshold()
    for _ in range(calls):
        if scale is None:
            L.check(lib.nunet_loss_step(L.ptr(xd), L.ptr(td), n, per, heads, L.LOSS_BCE_DICE, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters),
                                        thr, L.stream()), "nunet_loss_step")
        else:
            sc = torch.full((1,), scale, device=DEV)
            L.check(lib.nunet_loss_step_scaled(L.ptr(xd), L.ptr(td), n, per, heads, L.LOSS_BCE_DICE, L.ptr(ws), need, L.ptr(dl), L.ptr(lo),
                                               L.ptr(meters), thr, L.ptr(sc), L.stream()), "nunet_loss_step_scaled")
    torch.cuda.synchronize()
    return lo, dl


def host_iou_counts(x, t):
    """(intersection, union) of `sigmoid(x) > 0.5` and `t > 0.5` as oracle.iou_counts forms them, the fp32 sigmoid on the host;
    the input is zero-padded to a multiple of 256 so that every element takes torch's vectorised path (its scalar tail can
    differ from it by an ulp, metrics.iou_logit_threshold)"""
    x, t = x.reshape(-1), t.reshape(-1)
    xp = torch.zeros((x.numel() + 255) // 256 * 256)
    xp[:x.numel()] = x
    a = (torch.sigmoid(xp)[:x.numel()] > 0.5).numpy()
    b = t.numpy() > 0.5
    return int((a & b).sum()), int((a | b).sum())


@pytest.mark.parametrize("case", LC.FUSED_CASES, ids=LC.case_id)
def test_fused_step(case):
    """nunet_loss_step, BCE-Dice kind, against fp64 (not against the stand-alone device loss): the loss of every head and their
    mean, every pixel of d mean / d logits, the IoU counts of the LAST head exactly, the meters accumulated over two calls from
    nonzero values, and meters == NULL on another poison bit for bit.

    The smallest c each case needs over its heads, MI355X | the fp32 emulation on the CPU (test_bce_dice_cpu.py):
    (N x per, one head and "rand" unless named otherwise)
        2x1 0.000 | 0.000        3x257 1.065 | 1.065      3x2240 1.094 | 1.094      2x16384 1.474 | 1.475
        2x16385 1.269 | 1.269    2x65537 1.331 | 1.331    1x300 0.503 | 0.503       4x300 1.137 | 1.153
        5x300 0.682 | 0.682      16x300 1.242 | 1.258     17x300 0.938 | 0.938      33x300 1.122 | 1.093
        5x16385: 2 heads 1.337 | 1.337, 4 heads 1.394 | 1.394, 8 heads 1.430 | 1.430
        3x16385: empty_full 1.416 | 1.416, saturated 0.000 | 0.000, wide 1.427 | 1.427, beyond_exp 1.215 | 1.215,
        soft 1.230 | 1.236, zeros 0.000 | 0.000
    The worst |loss - ref| / max(1, |ref|) was 1.1e-7 (2x65537; 6.8e-7 on the loss of 19.4 of "beyond_exp")."""
    _, n, per, heads, _ = case
    assert_regime((L.LOSS_ENTRY_LOSS_STEP,), LC.REGIME[case], n, per, heads)
    x, t = LC.build(case)
    xd, td = x.to(DEV), t.to(DEV)
    meters = torch.zeros(4, dtype=torch.float64, device=DEV)
    meters.copy_(torch.tensor([2.0, 3.0, -1.0, -1.0], dtype=torch.float64))
    lo, dl = _step(xd, td, NAN, meters, calls=2)
    got = lo.tolist()
    refs = [LC.reference(case, k)[0] for k in range(heads)]
    for k in range(heads):
        loss_close(got[k], refs[k])
    loss_close(got[heads], sum(refs) / heads)
    print("%s: worst |loss - ref| = %.2e" % (LC.case_id(case), max(abs(a - b) for a, b in zip(got, refs))))
    worst = max(check_gradient(dl[k], case, k, "step %s head %d" % (LC.case_id(case), k), 1.0 / heads) for k in range(heads))
    print("step %s: needs c = %.3f over its heads" % (LC.case_id(case), worst))
    inter, union = host_iou_counts(x[-1], t)
    if case == LC.EDGE_CASE:
        assert host_iou_counts(x[-1, 0, :235], torch.ones(235))[0] not in (0, 235)        # the edge values fall on both sides
    m = meters.tolist()
    assert (m[2], m[3]) == (inter, union), (m, inter, union)
    assert abs(m[0] - (2.0 + 2 * got[heads])) < 1e-12
    assert abs(m[1] - (3.0 + 2 * (inter + 1e-5) / (union + 1e-5))) < 1e-12
    lo2, dl2 = _step(xd, td, -3e38, None)
    assert torch.equal(bits(lo2), bits(lo)) and torch.equal(bits(dl2), bits(dl))


@pytest.mark.parametrize("case", LC.SOFT_UNIFORM_CASES, ids=LC.case_id)
def test_uniform_soft_targets(case):
    """Targets uniform in [0, 1], through the raw stand-alone entries and the loss step: the loss, the per-image sums and every
    pixel of the gradient within 1e-6 of its addends' magnitudes plus the c = 4 term (loss_cases' docstring: at such targets
    the two gradient terms can cancel, which the hard-label bound of the other cases does not allow for).
    Worst |dx - ref| / m, measured on an MI355X | the fp32 emulation: stand-alone 3x9216 1.75e-7 | 1.66e-7, loss step 3x16385
    1.94e-7 | 1.84e-7; the c term was not needed (c = 0.000). The hard-label bound would need c = 2.47 and 2.06 there."""
    kind, n, per, _, _ = case
    assert_regime(ALONE_ENTRIES if kind == "alone" else (L.LOSS_ENTRY_LOSS_STEP,), LC.REGIME[case], n, per)
    x, t = LC.build(case)
    ref_loss, ref_dx, I, P, T = LC.reference(case)
    xd, td = x.to(DEV), t.to(DEV)
    if kind == "alone":
        loss, head, dx = _raw_alone(xd, td, NAN)
        sums = head[:3 * n].cpu().double().reshape(n, 3)
        for col, ref in enumerate((I, P, T)):
            assert bool(((sums[:, col] - ref).abs() <= 2e-6 * ref.abs()).all()), ("IPT"[col], sums[:, col], ref)
    else:
        lo, dl = _step(xd, td, NAN, None)
        loss, dx = lo[:1], dl[0]
        assert torch.equal(bits(lo[1:]), bits(lo[:1]))
    loss_close(float(loss), ref_loss)
    assert bool(torch.isfinite(dx).all())
    m = LC.addend_magnitudes(LC.head(case, 0), t)
    ratio = LC.worst_ratio(dx.cpu().double(), ref_dx, LC.unit_of(case), rel=m)
    print("%s: needs c = %.3f by the addends' magnitudes (worst |dx - ref| / m = %.2e); loss - ref = %.2e"
          % (LC.case_id(case), ratio, float(((dx.cpu().double() - ref_dx).abs() / m).max()), float(loss) - ref_loss))
    assert ratio <= C_DEVICE


@pytest.mark.parametrize("case", [("fused", 3, 2240, 1, "rand"), ("fused", 5, 16385, 2, "rand")], ids=LC.case_id)
def test_fused_step_scaled(case):
    """nunet_loss_step_scaled: a scale of 1024 gives the bits of the unscaled gradient times 1024, a scale of 1 the bits of the
    unscaled entry; the losses and the meters stay unscaled"""
    x, t = LC.build(case)
    xd, td = x.to(DEV), t.to(DEV)
    outs = []
    for scale in (None, 1.0, 1024.0):
        meters = torch.zeros(4, dtype=torch.float64, device=DEV)
        outs.append(_step(xd, td, NAN, meters, scale) + (meters.clone(),))
    (lo, dl, m), (lo1, dl1, m1), (lok, dlk, mk) = outs
    assert torch.equal(bits(dl1), bits(dl)) and torch.equal(bits(dlk), bits(dl * 1024.0))
    assert bool(torch.isfinite(dl).all()) and float(dl.abs().min()) * 1024 >= 2.0 ** -126
    assert torch.equal(bits(lo1), bits(lo)) and torch.equal(bits(lok), bits(lo))
    assert torch.equal(m1, m) and torch.equal(mk, m)


def test_fused_step_size_limit():
    """One image of 2^24 pixels, the largest the loss step takes (its per-image IoU counts pass through fp32): t = 1 everywhere,
    x = +1 except 12345 pixels of -1, so the counts must be exactly 2^24 - 12345 and 2^24 and the loss has an fp64 closed form
    (two distinct pixel values). 2^24 + 1 is refused with a message and writes nothing.

    Measured on an MI355X: loss 0.312586188 against 0.312588151, a difference of -1.96e-6 where 2e-6 is allowed. It is the
    kernel's, not the test's: every thread of bce_dice_partial_kernel<true> adds 1024 pixels one after the other in fp32, and with
    all of them equal (0.7310586) the roundings do not average out: sum p comes out 5.2e-6 too large and the BCE sum 3.4e-6, as an
    fp32 evaluation of the same summation order on the CPU reproduces to three digits. The workload's largest images
    (512 x 512) take 16 trips per thread."""
    import math
    per = 2 ** 24
    assert_regime((L.LOSS_ENTRY_LOSS_STEP,), (64, 1024, 1024), 1, per)
    g = torch.Generator().manual_seed(12345)
    x = torch.ones(per + 1)
    x[torch.randperm(per, generator=g)[:12345]] = -1
    xd, td = x.to(DEV).reshape(1, 1, per + 1), torch.ones(1, per + 1).to(DEV)
    lib = L.lib()
    need = lib.nunet_loss_step_ws_bytes(1, per, 1, L.LOSS_BCE_DICE)
    assert lib.nunet_loss_step_ws_bytes(1, per + 1, 1, L.LOSS_BCE_DICE) == need
    ws = torch.full((need // 4,), NAN, device=DEV)
    dl, lo = torch.full((per + 1,), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    meters = torch.zeros(4, dtype=torch.float64, device=DEV)
    meters.copy_(torch.tensor([2.0, 3.0, -1.0, -1.0], dtype=torch.float64))
    thr = nunet_amd.metrics.iou_logit_threshold()
    info = L.LossLaunchInfo()
    assert lib.nunet_loss_launch_info(L.LOSS_ENTRY_LOSS_STEP, 1, per + 1, 1, C.byref(info)) == -1
    rc = lib.nunet_loss_step(L.ptr(xd), L.ptr(td), 1, per + 1, 1, L.LOSS_BCE_DICE, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters), thr, L.stream())
    assert rc == -1 and b"image too large" in lib.nunet_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(lo).all()) and bool(torch.isnan(ws).all())
    assert meters.tolist() == [2.0, 3.0, -1.0, -1.0]
    L.check(lib.nunet_loss_step(L.ptr(xd), L.ptr(td), 1, per, 1, L.LOSS_BCE_DICE, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters), thr, L.stream()),
            "nunet_loss_step")
    torch.cuda.synchronize()
    a, b = per - 12345, 12345
    sum_p = a / (1 + math.exp(-1.0)) + b / (1 + math.exp(1.0))                   # I == P: t = 1
    bce = a * math.log1p(math.exp(-1.0)) + b * (1 + math.log1p(math.exp(-1.0)))
    ref = 0.5 * bce / per + 1 - (2 * sum_p + 1e-5) / (sum_p + per + 1e-5)
    got = lo.tolist()
    print("2^24: loss %.9f, closed form %.9f, difference %.2e" % (got[0], ref, got[0] - ref))
    m = meters.tolist()
    assert (m[2], m[3]) == (per - 12345, per), m
    assert bool(torch.isfinite(dl[:per]).all()) and bool(torch.isnan(dl[per:]).all())
    assert got[1] == got[0]
    loss_close(got[0], ref)


# ---------------------------------------------------------------------------------------------------------------------------
# IoU counts
# ---------------------------------------------------------------------------------------------------------------------------
# n -> (gx, most trips, fewest trips): 256 blocks of 256 threads at the most, so threads stride from n > 65536 on
IOU_CASES = {1: (1, 1, 0), 63: (1, 1, 0), 65: (1, 1, 0), 257: (1, 2, 1), 1025: (2, 3, 2), 262144: (256, 4, 4), 262145: (256, 5, 4),
             2 ** 20 + 3: (256, 17, 16)}


@pytest.mark.parametrize("n", sorted(IOU_CASES))
def test_iou_counts(n):
    """nunet_iou_counts equals the host expression exactly, from zero and accumulated onto [7, 11]: one wave, a partial second
    wave, several blocks (cross-block atomics), the block cap and the stride loop past it. The logits hold the
    sigmoid-threshold edge values (NaN and both infinities among them) at the front and, where they fit twice, at the back."""
    i = launch_info(L.LOSS_ENTRY_IOU_COUNTS, 1, n)
    assert (i.grid_x, i.trips_max, i.trips_min, i.grid_y, i.grid_z, i.block) == IOU_CASES[n] + (1, 1, 256)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.where(torch.rand(n, generator=g) < 0.5, 1.0, 1e-7)
    t = (torch.rand(n, generator=g) < 0.4).float()
    edges = torch.cat([torch.from_numpy(LC.iou_edges()), torch.tensor([float("inf"), float("-inf"), NAN])]).roll(3)
    k = min(n, edges.numel())
    x[:k] = edges[:k]
    if n >= 2 * edges.numel():
        x[-edges.numel():] = edges
    inter, union = host_iou_counts(x, t)
    assert n < 63 or 0 < inter < union < n
    xd, td = x.to(DEV), t.to(DEV)
    counts = nunet_amd.metrics.iou_counts(xd, td)
    assert counts.tolist() == [inter, union]
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    counts.copy_(torch.tensor([7, 11]))
    nunet_amd.metrics.iou_counts(xd, td, counts)
    assert counts.tolist() == [7 + inter, 11 + union]


# ---------------------------------------------------------------------------------------------------------------------------
# mask export
# ---------------------------------------------------------------------------------------------------------------------------
# n -> (gx, most trips, fewest trips) over the n / 4 vector items; the n % 4 tail is written by threads 0 .. 2 of block 0
U8_BIG = 2 ** 21 + 4 * 256 * 3 + 1
U8_CASES = {1: (1, 0, 0), 2: (1, 0, 0), 3: (1, 0, 0), 5: (1, 1, 0), 1023: (1, 1, 0), U8_BIG: (2048, 2, 1)}


def _u8_inputs(n):
    thr = nunet_amd.metrics.sigmoid_u8_thresholds(torch.device(DEV)).cpu()
    special = torch.tensor([NAN, float("-inf"), float("inf")])
    edges = torch.cat([special, thr[:1], thr[-1:], thr, torch.nextafter(thr, torch.tensor(-1e9)), torch.nextafter(thr, torch.tensor(1e9)),
                       torch.tensor([-100.0, 100.0, 0.0, -0.0, 20.0])])
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 4
    k = min(n, edges.numel())
    x[:k] = edges[:k]
    if n >= 2 * edges.numel():
        x[-edges.numel():] = edges.flip(0)          # NaN is the last element: the tail thread's
    xp = torch.zeros((n + 255) // 256 * 256)
    xp[:n] = torch.where(torch.isfinite(x), x, torch.zeros(()))
    ref = torch.from_numpy((torch.sigmoid(xp).numpy() * np.float32(255)).astype("uint8"))[:n].clone()
    ref[torch.isnan(x) | (x == float("-inf"))] = 0          # the header's contract, not the host's cast
    ref[x == float("inf")] = 255
    return x, ref, thr


@pytest.mark.parametrize("n", sorted(U8_CASES))
def test_sigmoid_u8(n):
    """nunet_sigmoid_u8 into a buffer of exactly n bytes between guard bands, byte-exact against the host expression
    `(sigmoid(x) * 255).astype('uint8')` with NaN -> 0, -inf -> 0, +inf -> 255 as include/nunet.h states: n < 4 (the tail alone),
    n % 4 of 1, 2 and 3, and a size past the grid cap whose threads take a second trip. The inputs hold all 255 thresholds and
    their two fp32 neighbours wherever n allows."""
    i = launch_info(L.LOSS_ENTRY_SIGMOID_U8, 1, n)
    assert (i.grid_x, i.trips_max, i.trips_min, i.items, i.block) == U8_CASES[n] + (n // 4, 256)
    if n == U8_BIG:
        assert i.grid_x == 2048 and i.items > i.grid_x * i.block and n % 4 == 1           # past the cap
    x, ref, _ = _u8_inputs(n)
    assert n < 1023 or (int(ref.max()) == 255 and int(ref.min()) == 0 and len(torch.unique(ref)) == 256)
    xd = x.to(DEV)
    thr = nunet_amd.metrics.sigmoid_u8_thresholds(torch.device(DEV))
    out = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    L.check(L.lib().nunet_sigmoid_u8(L.ptr(xd), L.ptr(thr), L.ptr(out), n, L.stream()), "nunet_sigmoid_u8")
    got = out.cpu()
    assert torch.equal(got, ref), (int((got != ref).sum()), (got != ref).nonzero()[:8].flatten().tolist())


def test_sigmoid_u8_refuses_misaligned_pointers():
    """logits 4 bytes off a 16-byte boundary, the output 1 byte off a 4-byte boundary: NUNET_EINVAL with a message, the output
    untouched (the vector loads and the packed 4-byte stores need the alignment)"""
    n = 1023
    x, ref, _ = _u8_inputs(n)
    lib = L.lib()
    thr = nunet_amd.metrics.sigmoid_u8_thresholds(torch.device(DEV))
    xd = torch.zeros(n + 4, device=DEV)
    xd[1:n + 1] = x.to(DEV)
    out = torch.full((n + 4,), 0x5A, dtype=torch.uint8, device=DEV)
    assert xd.data_ptr() % 16 == 0 and out.data_ptr() % 4 == 0
    assert lib.nunet_sigmoid_u8(L.ptr(xd, 4), L.ptr(thr), L.ptr(out), n, L.stream()) == -1
    assert b"sigmoid_u8" in lib.nunet_last_error() and b"aligned" in lib.nunet_last_error()
    assert lib.nunet_sigmoid_u8(L.ptr(xd), L.ptr(thr), L.ptr(out, 1), n, L.stream()) == -1
    assert b"sigmoid_u8" in lib.nunet_last_error() and b"aligned" in lib.nunet_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    xa = torch.zeros(n, device=DEV)
    xa.copy_(x)
    L.check(lib.nunet_sigmoid_u8(L.ptr(xa), L.ptr(thr), L.ptr(out), n, L.stream()), "aligned pointers are accepted")
    assert torch.equal(out[:n].cpu(), ref) and bool((out[n:] == 0x5A).all())
