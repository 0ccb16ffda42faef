"""BCEWithLogitsLoss, the reference's third `--loss` (trains.py:27-28,210-211), on the MI355X: the stand-alone pair
nunet_bce_logits_fwd / _bwd and nunet_amd.losses.BCEWithLogitsLoss, the loss step's kind NUNET_LOSS_BCE_LOGITS, TrainStep with it
against the generic autograd path through torch's own loss, the reference's trajectories and train.py end to end.

The cases, the fp64 reference (torch's binary_cross_entropy_with_logits on the CPU) and the per-element gradient bound are those
of tests/bce_logits_cases.py, pinned on the CPU by tests/test_bce_logits_cpu.py; every kernel case first asserts, from the
library's own nunet_loss_launch_info, the launch regime it is named for. The gradient criterion is that bound with c = 4 on
every element - twice what the fp32 emulation on the CPU is held to - uniform soft targets included; the loss is held to
2e-6 max(1, |ref|). The smallest c and the loss error of every case are printed before they are asserted."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.trainer import TrainStep, cosine_lr  # noqa: E402
from conftest import load_golden  # noqa: E402
import loss_cases as LC  # noqa: E402
import bce_logits_cases as BC  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_DEVICE = 4.0
NAN = float("nan")
KIND = L.LOSS_BCE_LOGITS
ALONE_ENTRIES = (L.LOSS_ENTRY_BCE_LOGITS_FWD, L.LOSS_ENTRY_BCE_LOGITS_BWD)
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor, chosen without timing


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate with a torch factory - the loss module's workspace included - sits between
    guard bands that are checked after the test (conftest.py)"""
    yield


def bits(a):
    return a.view(torch.int32)


def assert_regime(entries, claim, n_img, per_or_n, heads=1):
    """claim = (gx, most trips, fewest trips) as the case list states it; the library answers from the launch's own expressions"""
    for entry in entries:
        i = L.LossLaunchInfo()
        L.check(L.lib().nunet_loss_launch_info(entry, n_img, per_or_n, heads, C.byref(i)), "nunet_loss_launch_info")
        assert (i.grid_x, i.trips_max, i.trips_min) == tuple(claim), (entry, (i.grid_x, i.trips_max, i.trips_min), claim)
        assert (i.grid_y, i.grid_z, i.block) == ((n_img, heads, 256) if entry == L.LOSS_ENTRY_LOSS_STEP else (1, 1, 256))


def loss_close(got, ref):
    assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (got, ref, got - ref)


def check_gradient(got, case, k, what, factor=1.0):
    """got: device gradient of head k, any shape; every element within factor * bound(c = 4). -> the smallest c that passes"""
    assert bool(torch.isfinite(got).all()), "%s: gradient entries left unwritten or not finite" % what
    ref = BC.reference(case, k)[1]
    ratio = BC.worst_ratio(got.cpu().double().reshape(ref.shape), ref, BC.unit_of(case, k), factor)
    print("%s: needs c = %.3f" % (what, ratio))
    assert ratio <= C_DEVICE, "%s: c = %.3f" % (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# stand-alone pair
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_alone(xd, td, poison, gscale=None, byte_offset=0):
    """nunet_bce_logits_fwd + _bwd over the n elements that start `byte_offset` bytes into xd and td, on a workspace of exactly the
    stated size; the workspace, the loss and the gradient are filled with `poison` beforehand -> (loss [1], dx [n])"""
    lib = L.lib()
    n = xd.numel() - byte_offset // 4
    need = lib.nunet_bce_logits_ws_bytes(n)
    assert need % 4 == 0 and need > 0
    ws = torch.full((need // 4,), poison, device=DEV)
    loss, dx = torch.full((1,), poison, device=DEV), torch.full((xd.numel(),), poison, device=DEV)
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    L.check(lib.nunet_bce_logits_fwd(L.ptr(xd, byte_offset), L.ptr(td, byte_offset), n, L.ptr(ws), need, L.ptr(loss), L.stream()), "nunet_bce_logits_fwd")
    L.check(lib.nunet_bce_logits_bwd(L.ptr(xd, byte_offset), L.ptr(td, byte_offset), n, L.ptr(gs), L.ptr(dx, byte_offset), L.stream()), "nunet_bce_logits_bwd")
    torch.cuda.synchronize()
    return loss, dx


def _check_raw_alone(case, xd, td, byte_offset=0):
    """what test_standalone_raw_entries states, on device buffers whose first byte_offset bytes are not part of the case"""
    skip = byte_offset // 4
    what = "raw %s%s" % (LC.case_id(case), ", %d bytes off" % byte_offset if byte_offset else "")
    ref_loss = BC.reference(case)[0]
    loss, dx = _raw_alone(xd, td, NAN, None, byte_offset)
    print("%s: (loss - ref) / max(1, |ref|) = %.2e" % (what, (float(loss) - ref_loss) / max(1.0, abs(ref_loss))))
    loss_close(float(loss), ref_loss)
    assert bool(torch.isnan(dx[:skip]).all())
    check_gradient(dx[skip:], case, 0, what)
    # upstream scales
    _, dx25 = _raw_alone(xd, td, NAN, 0.25, byte_offset)
    normal = dx[skip:].abs() >= 2.0 ** -100
    assert torch.equal(bits(dx25[skip:])[normal], bits(dx[skip:] * 0.25)[normal]) and bool(torch.isfinite(dx25[skip:]).all())
    _, dx37 = _raw_alone(xd, td, NAN, 0.37, byte_offset)
    check_gradient(dx37[skip:], case, 0, what + ", gscale 0.37", 0.37)
    # another poison
    loss2, dx2 = _raw_alone(xd, td, 1e30, None, byte_offset)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(dx2[skip:]), bits(dx[skip:]))


@pytest.mark.parametrize("case", BC.ALONE_CASES, ids=LC.case_id)
def test_standalone_raw_entries(case):
    """The C entries on NaN-filled buffers and a workspace of exactly nunet_bce_logits_ws_bytes(n): the loss, every element of
    the gradient, the upstream scales 0.25 (the bits of the unscaled gradient times 0.25 wherever that is normal) and 0.37, and
    a second run on a differently poisoned workspace (bit-identical: no partial is read that no block wrote). Sizes: one
    element, one partial block, a second block with one element, n % 4 of 1, 2 and 3, the block cap exactly, cap plus one
    (a second trip for one thread), 64 and 65 trips; the six patterns and uniform soft targets on 3 x 9216.

    The smallest c each case needs, MI355X | the fp32 emulation on the CPU (test_bce_logits_cpu.py); n, "rand" unless a pattern
    is named:
        1 0.000 | 0.000          255 0.936 | 0.936        257 0.607 | 0.607        1022 1.359 | 1.359
        1023 1.009 | 1.009       65536 1.317 | 1.317      65537 1.377 | 1.377      4194307 1.426 | 1.426
        3x9216: empty_full 1.307 | 1.307, saturated 0.000 | 0.000, wide 1.406 | 1.406, beyond_exp 1.195 | 1.195,
        soft 1.307 | 1.307, zeros 0.000 | 0.000, soft_uniform 1.620 | 1.438
    (gscale 0.37: within 0.01 of these; 4 bytes off a 16-byte boundary: the aligned figures.) The worst
    |loss - ref| / max(1, |ref|) was 8.8e-8 (65536), against the 2e-6 allowed."""
    n = BC.count(case)
    assert_regime(ALONE_ENTRIES, BC.REGIME[case], 1, n)
    x, t = LC.build(case)
    _check_raw_alone(case, x.reshape(-1).to(DEV), t.reshape(-1).to(DEV))


def test_standalone_pointers_four_bytes_off_a_16_byte_boundary():
    """logits, targets and the gradient start 4 bytes past a 16-byte boundary: nothing is refused, the element before the
    first stays untouched, the results are those of the aligned call bit for bit"""
    case = ("alone", 1, BC.MISALIGNED_SIZE, 1, "rand")
    assert case in BC.ALONE_CASES
    x, t = LC.build(case)
    xd, td = torch.zeros(x.numel() + 1, device=DEV), torch.zeros(x.numel() + 1, device=DEV)
    xd[1:] = x.reshape(-1).to(DEV)
    td[1:] = t.reshape(-1).to(DEV)
    assert xd.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    _check_raw_alone(case, xd, td, 4)
    loss_a, dx_a = _raw_alone(x.reshape(-1).to(DEV), t.reshape(-1).to(DEV), NAN)
    loss_m, dx_m = _raw_alone(xd, td, NAN, None, 4)
    assert torch.equal(bits(loss_m), bits(loss_a)) and torch.equal(bits(dx_m[1:]), bits(dx_a))


@pytest.mark.parametrize("case", BC.ALONE_CASES, ids=LC.case_id)
def test_standalone_module(case):
    """nunet_amd.losses.BCEWithLogitsLoss, forward and backward (its workspace comes from torch.empty)"""
    assert_regime(ALONE_ENTRIES, BC.REGIME[case], 1, BC.count(case))
    x, t = LC.build(case)
    xd = x.to(DEV).requires_grad_(True)
    loss = nunet_amd.losses.BCEWithLogitsLoss()(xd, t.to(DEV))
    loss.backward()
    loss_close(float(loss.detach()), BC.reference(case)[0])
    check_gradient(xd.grad, case, 0, "module " + LC.case_id(case))


def test_standalone_module_takes_4d_and_non_contiguous_inputs():
    """[N, 4, h, w] as a four-class head hands it over, and the same values as a non-contiguous view (the wrapper copies): the
    loss and the gradient are those of the contiguous call bit for bit; an upstream gradient other than 1 scales it"""
    case = ("fused", 3, 2240, 1, "rand")
    assert case in BC.FUSED_CASES
    x, t = LC.head(case, 0), LC.build(case)[1]
    shape = (3, 4, 20, 28)
    crit = nunet_amd.losses.BCEWithLogitsLoss()
    xd = x.reshape(shape).to(DEV).requires_grad_(True)
    loss = crit(xd, t.reshape(shape).to(DEV))
    (loss * 0.5).backward()
    loss_close(float(loss.detach()), BC.reference(case)[0])
    check_gradient(xd.grad, case, 0, "[N, 4, h, w], half the loss", 0.5)
    xd.grad = None
    crit(xd, t.reshape(shape).to(DEV)).backward()
    check_gradient(xd.grad, case, 0, "[N, 4, h, w]")
    leaf = x.reshape(shape).transpose(2, 3).contiguous().to(DEV).requires_grad_(True)      # stored [N, 4, w, h]
    tv = t.reshape(shape).transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
    view = leaf.transpose(2, 3)
    assert not view.is_contiguous() and not tv.is_contiguous() and torch.equal(view.detach().cpu(), x.reshape(shape))
    loss2 = crit(view, tv)
    loss2.backward()
    assert torch.equal(bits(loss2.detach().reshape(1)), bits(loss.detach().reshape(1)))
    assert torch.equal(bits(leaf.grad.transpose(2, 3).contiguous()), bits(xd.grad))
    with pytest.raises(L.NunetError):
        crit(xd, t.reshape(3, -1).to(DEV))


# ---------------------------------------------------------------------------------------------------------------------------
# loss step, kind NUNET_LOSS_BCE_LOGITS
# ---------------------------------------------------------------------------------------------------------------------------
def _step(xd, td, poison, meters, scale=None, calls=1):
    """nunet_loss_step (or _scaled, with `scale` on the device) with the BCE_LOGITS kind on a poisoned workspace of exactly the
    stated size -> (loss_out [heads + 1], dx [heads, N, per])"""
    lib = L.lib()
    heads, n, per = xd.shape
    need = lib.nunet_loss_step_ws_bytes(n, per, heads, KIND)
    assert need % 4 == 0 and need > 0
    ws = torch.full((need // 4,), poison, device=DEV)
    dl, lo = torch.full((heads, n, per), poison, device=DEV), torch.full((heads + 1,), poison, device=DEV)
    thr = nunet_amd.metrics.iou_logit_threshold()
    for _ in range(calls):
        if scale is None:
            L.check(lib.nunet_loss_step(L.ptr(xd), L.ptr(td), n, per, heads, KIND, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters),
                                        thr, L.stream()), "nunet_loss_step")
        else:
            sc = torch.full((1,), scale, device=DEV)
            L.check(lib.nunet_loss_step_scaled(L.ptr(xd), L.ptr(td), n, per, heads, KIND, L.ptr(ws), need, L.ptr(dl), L.ptr(lo),
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


@pytest.mark.parametrize("case", BC.FUSED_CASES, ids=LC.case_id)
def test_fused_step(case):
    """nunet_loss_step, BCE_LOGITS kind, against fp64: the loss of every head and their mean, every element of
    d mean / d logits at factor 1 / heads, the IoU counts of the LAST head exactly, the meters accumulated over two calls from
    nonzero values, and meters == NULL on another poison bit for bit. Uniform soft targets run under the same bound.

    The smallest c each case needs over its heads, MI355X | the fp32 emulation on the CPU (test_bce_logits_cpu.py);
    N x per, one head and "rand" unless named otherwise:
        2x1 0.000 | 0.000        3x257 1.082 | 1.082      3x2240 1.108 | 1.108      2x16384 1.477 | 1.477
        2x16385 1.277 | 1.277    2x65537 1.339 | 1.339    1x300 0.593 | 0.593       4x300 1.168 | 1.168
        5x300 0.751 | 0.751      16x300 1.269 | 1.269     17x300 0.949 | 0.949      33x300 1.139 | 1.086
        5x16385: 2 heads 1.341 | 1.341, 4 heads 1.403 | 1.403, 8 heads 1.436 | 1.436
        3x16385: empty_full 1.419 | 1.419, saturated 0.000 | 0.000, wide 1.428 | 1.428, beyond_exp 1.223 | 1.223,
        soft 1.245 | 1.245, zeros 0.000 | 0.000, soft_uniform 1.609 | 1.593
    The worst |loss - ref| / max(1, |ref|) was 1.1e-7 (2x16385)."""
    _, n, per, heads, _ = case
    assert_regime((L.LOSS_ENTRY_LOSS_STEP,), BC.REGIME[case], n, per, heads)
    x, t = LC.build(case)
    xd, td = x.to(DEV), t.to(DEV)
    meters = torch.zeros(4, dtype=torch.float64, device=DEV)
    meters.copy_(torch.tensor([2.0, 3.0, -1.0, -1.0], dtype=torch.float64))
    lo, dl = _step(xd, td, NAN, meters, calls=2)
    got = lo.tolist()
    refs = [BC.reference(case, k)[0] for k in range(heads)]
    print("%s: worst |loss - ref| / max(1, |ref|) = %.2e" % (LC.case_id(case), max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got, refs))))
    for k in range(heads):
        loss_close(got[k], refs[k])
    loss_close(got[heads], sum(refs) / heads)
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


@pytest.mark.parametrize("case", [("fused", 3, 2240, 1, "rand"), ("fused", 5, 16385, 2, "rand")], ids=LC.case_id)
def test_fused_step_scaled(case):
    """nunet_loss_step_scaled: a scale of 1024 gives the bits of the unscaled gradient times 1024, a scale of 1 the bits of the
    unscaled entry; the losses and the meters stay unscaled"""
    assert case in BC.FUSED_CASES
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
    """One image of 2^24 elements, the largest the loss step takes (its per-image IoU counts pass through fp32): t = 1 everywhere,
    x = +1 except 12345 elements of -1, so the counts must be exactly 2^24 - 12345 and 2^24 and the loss has an fp64 closed form
    (two distinct values). 2^24 + 1 is refused with "image too large" and writes nothing. The loss is held to 1e-5 relative:
    every thread adds 1024 elements one after the other in fp32, the loop shape for which tests/test_bce_dice_gpu.py documents
    5.2e-6 on a sum of equal values; this is twice that.

    Measured on an MI355X: loss 0.313998580 against 0.313997507, 3.42e-6 relative - the 3.4e-6 that
    tests/test_bce_dice_gpu.py::test_fused_step_size_limit reports for the BCE sum of the same values in the same loop."""
    per = 2 ** 24
    assert_regime((L.LOSS_ENTRY_LOSS_STEP,), (64, 1024, 1024), 1, per)
    g = torch.Generator().manual_seed(12345)
    x = torch.ones(per + 1)
    x[torch.randperm(per, generator=g)[:12345]] = -1
    xd, td = x.to(DEV).reshape(1, 1, per + 1), torch.ones(1, per + 1).to(DEV)
    lib = L.lib()
    need = lib.nunet_loss_step_ws_bytes(1, per, 1, KIND)
    ws = torch.full((need // 4,), NAN, device=DEV)
    dl, lo = torch.full((per + 1,), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    meters = torch.zeros(4, dtype=torch.float64, device=DEV)
    meters.copy_(torch.tensor([2.0, 3.0, -1.0, -1.0], dtype=torch.float64))
    thr = nunet_amd.metrics.iou_logit_threshold()
    rc = lib.nunet_loss_step(L.ptr(xd), L.ptr(td), 1, per + 1, 1, KIND, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters), thr, L.stream())
    assert rc == -1 and b"image too large" in lib.nunet_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(lo).all()) and bool(torch.isnan(ws).all())
    assert meters.tolist() == [2.0, 3.0, -1.0, -1.0]
    L.check(lib.nunet_loss_step(L.ptr(xd), L.ptr(td), 1, per, 1, KIND, L.ptr(ws), need, L.ptr(dl), L.ptr(lo), L.ptr(meters), thr, L.stream()),
            "nunet_loss_step")
    torch.cuda.synchronize()
    a, b = per - 12345, 12345
    ref = (a * math.log1p(math.exp(-1.0)) + b * (1 + math.log1p(math.exp(-1.0)))) / per
    got = lo.tolist()
    print("2^24: loss %.9f, closed form %.9f, relative difference %.2e" % (got[0], ref, (got[0] - ref) / ref))
    m = meters.tolist()
    assert (m[2], m[3]) == (per - 12345, per), m
    assert bool(torch.isfinite(dl[:per]).all()) and bool(torch.isnan(dl[per:]).all())
    pos, neg = (1 / (1 + math.exp(-1.0)) - 1) / per, (1 / (1 + math.exp(1.0)) - 1) / per
    want = torch.where(xd.reshape(-1)[:per] > 0, torch.tensor(pos, dtype=torch.float64, device=DEV), torch.tensor(neg, dtype=torch.float64, device=DEV))
    assert float(((dl[:per].double() - want) / want).abs().max()) < 1e-6
    assert got[1] == got[0]
    assert abs(got[0] - ref) <= 1e-5 * abs(ref), (got[0], ref)


# ---------------------------------------------------------------------------------------------------------------------------
# TrainStep
# ---------------------------------------------------------------------------------------------------------------------------
def _module(st, ncls=1, ds=False):
    m = nunet_amd.archs.NestedUNet(ncls, 3, ds)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.clone() for k, v in st.items()})
    return m.to(DEV).train()


def _batch(synth, n, hw, ncls, seed):
    img, msk = synth.synth_batch(n, hw, hw, 3, ncls, seed=seed)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)


@pytest.mark.parametrize("ds,ncls,graph", [(False, 1, False), (False, 1, True), (True, 1, False), (True, 1, True), (True, 4, True)])
def test_bce_logits_inside_the_fused_step(ds, ncls, graph, synth):
    """BCEWithLogitsLoss as a TrainStep loss, eager and captured, with deep supervision and four classes: one fp32 step against
    the generic path - module forward -> torch.nn.BCEWithLogitsLoss() (torch's own kernel, the reference's own expression,
    trains.py:210-211) -> backward -> torch.optim.SGD. The bounds of test_lovasz_hinge_inside_the_fused_step.
    Measured on an MI355X: every gradient tensor equal to the generic path's (N * per * heads is a power of two in all five
    cases, so both sides scale sigmoid(x) - t exactly), the losses equal to the seven digits printed."""
    n, hw = 4, 32
    torch.manual_seed(5)
    sd = {k: v.clone() for k, v in nunet_amd.archs.NestedUNet(ncls, 3, ds).state_dict().items()}
    x, t = _batch(synth, n, hw, ncls, 31)
    # generic path
    m0 = _module(sd, ncls, ds)
    crit = torch.nn.BCEWithLogitsLoss()
    out = m0(x)
    outs = out if ds else [out]
    losses = [crit(o, t) for o in outs]
    loss = sum(losses) / len(losses)
    loss.backward()
    g0 = {k: p.grad.detach().clone() for k, p in m0.named_parameters()}
    iou0 = nunet_amd.metrics.iou_score(outs[-1], t)
    opt = torch.optim.SGD(m0.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt.step()
    # fused step
    m1 = _module(sd, ncls, ds)
    ts = TrainStep(m1, (n, 3, hw, hw), lr=1e-2, momentum=0.9, weight_decay=1e-4, loss="BCEWithLogitsLoss", use_graph=graph)
    assert ts.loss_kind == KIND and ts.heads == len(outs)
    if graph:
        ts.capture(x, t)
    ts.reset_meters()
    ts.step(x, t)
    tl, ti = ts.epoch_stats()
    lo = ts.loss_out.tolist()
    losses, loss = [float(v.detach()) for v in losses], float(loss.detach())
    for k, lk in enumerate(losses):
        assert abs(lo[k] - lk) < 2e-6 * max(1.0, abs(lk)), (k, lo[k], lk)
    assert abs(tl - loss) < 2e-6 * max(1.0, abs(loss))
    assert abs(ti - iou0) < 1e-12
    worst = 0.0
    for k, p in m1.named_parameters():
        ref = g0[k]
        worst = max(worst, float((p.grad - ref).norm()) / max(float(ref.norm()), 1e-30))
        assert float((p.grad - ref).norm()) <= 1e-5 * float(ref.norm()) + 1e-9, k
    print("ds %s, K %d, graph %s: loss %.7f vs %.7f, worst relative gradient difference %.2e" % (ds, ncls, graph, tl, loss, worst))
    for (k, p), q in zip(m1.named_parameters(), m0.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) < 1e-6, k


def test_unknown_loss_is_still_refused(synth):
    with pytest.raises(L.NunetError):
        TrainStep(_module(synth.closed_form_state(1, 3, False, True)), (2, 3, 32, 32), loss="BCELoss")


def test_scaling_and_clipping_leave_the_step_bit_identical(synth):
    """loss_scale 1024 (a power of two, never grown here) next to clip_grad_norm 1.0, fp32: after 2 captured steps the
    parameters are bit-identical to those of the same TrainStep without scaling. (Measured on an MI355X: 0 of 122 tensors
    differ.)"""
    st = synth.closed_form_state(1, 3, False, True)
    data = [_batch(synth, 4, 32, 1, s) for s in (21, 22)]
    res = []
    for ls in (None, dict(init_scale=1024., growth_interval=1000)):
        m = _module(st)
        ts = TrainStep(m, (4, 3, 32, 32), lr=1e-2, loss="BCEWithLogitsLoss", loss_scale=ls, clip_grad_norm=1.0, **GRAPH)
        ts.capture(*data[0])
        for x, t in data:
            ts.step(x, t)
        torch.cuda.synchronize()
        if ls is not None:
            assert ts.scaler_stats() == (1024.0, 0)
        res.append({k: p.detach().clone() for k, p in m.named_parameters()})
    diff = {k: float((res[1][k].double() - res[0][k].double()).norm() / res[0][k].double().norm().clamp(min=1e-30)) for k in res[0]}
    worst = max(diff, key=diff.get)
    print("scaled vs unscaled: %d of %d tensors differ, worst relative difference %.2e (%s)"
          % (sum(not torch.equal(res[1][k], res[0][k]) for k in res[0]), len(res[0]), diff[worst], worst))
    for k in res[0]:
        assert torch.equal(bits(res[1][k]), bits(res[0][k])), (k, diff[k])


@pytest.mark.parametrize("tag,ds,ncls", [("k1", False, 1), ("ds_k4", True, 4)])
def test_trajectory_against_reference(tag, ds, ncls, synth):
    """8 captured fp32 SGD steps + cosine schedule against the reference's own run with nn.BCEWithLogitsLoss
    (tests/golden/make_golden_bce_logits.py), one class and four classes under deep supervision: lr to 1e-12, every step's
    loss within 1e-4, IoU within 5e-3; then the evaluation forward and nunet_amd.losses.BCEWithLogitsLoss, val_loss within 1e-4.
    With this loss the reference's own fp32-vs-fp64 spread stays <= 2.4e-6 in loss through all eight steps, so no step gets
    the 2e-2 band of tests/test_net_gpu.py::test_trajectory_against_reference.

    Measured on an MI355X, |loss - golden| per step: one class 0, 6.0e-8, 0, 2.4e-7, 6.6e-7, 7.7e-7, 1.1e-6, 9.5e-7; four
    classes under deep supervision at most 1.2e-7; every IoU and val_iou equal to the golden's, val_loss within 6.0e-8."""
    g = load_golden("trajectory_bcelogits_n4_32x32")
    m = _module(synth.closed_form_state(ncls, 3, ds, True), ncls, ds)
    batches = [_batch(synth, 4, 32, ncls, 1234 + k) for k in range(8)]
    ts = TrainStep(m, (4, 3, 32, 32), lr=1e-3, momentum=0.9, weight_decay=1e-4, loss="BCEWithLogitsLoss", **GRAPH)
    ts.capture(*batches[0])
    step, dev = 0, []
    for ep in range(4):
        lr = cosine_lr(1e-3, 1e-5, ep, 4)
        ts.set_lr(lr)
        for _ in range(2):
            ts.reset_meters()
            ts.step(*batches[step])
            loss, iou = ts.epoch_stats()
            dev.append((abs(lr - g["lr_" + tag][step]), abs(loss - g["loss_" + tag][step]), abs(iou - g["iou_" + tag][step])))
            step += 1
    m.eval()
    x, t = _batch(synth, 4, 32, ncls, 99)
    crit = nunet_amd.losses.BCEWithLogitsLoss()
    with torch.no_grad():
        o = m(x)
        outs = o if ds else [o]
        vloss = float(sum(crit(v, t) for v in outs) / len(outs))
    viou = nunet_amd.metrics.iou_score(outs[-1], t)
    print("%s: worst |loss - golden| %.2e (per step %s), worst |iou - golden| %.2e, |val_loss - golden| %.2e, |val_iou - golden| %.2e"
          % (tag, max(d[1] for d in dev), " ".join("%.1e" % d[1] for d in dev), max(d[2] for d in dev), abs(vloss - float(g["val_loss_" + tag])),
             abs(viou - float(g["val_iou_" + tag]))))
    for k, (dlr, dloss, diou) in enumerate(dev):
        assert dlr < 1e-12 and dloss < 1e-4 and diou < 5e-3, (k, dlr, dloss, diou)
    assert abs(vloss - float(g["val_loss_" + tag])) < 1e-4


@pytest.mark.parametrize("extra", [[], ["--num_classes", "4", "--deep_supervision", "True"]], ids=["k1", "k4_ds"])
def test_train_py_runs_the_fused_step(extra, tmp_path):
    """train.py --loss BCEWithLogitsLoss for 2 epochs on a small synthetic set (the default bf16 and, for one class, the uint8
    device pipeline), as a child process under a time limit: it takes the fused step and logs a finite loss and val_iou."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--loss", "BCEWithLogitsLoss", "--epochs", "2", "--train_size", "64",
           "--val_size", "32", "--input_h", "32", "--input_w", "32", "-b", "8", "--name", "bcel_e2e"] + extra
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "=> fused training step (TrainStep): SGD, BCEWithLogitsLoss" in r.stdout, r.stdout[-2000:]
    rows = open(tmp_path / "models" / "bcel_e2e" / "log.csv").read().strip().splitlines()
    head = rows[0].split(",")
    assert len(rows) == 3
    for row in rows[1:]:
        rec = dict(zip(head, row.split(",")))
        assert math.isfinite(float(rec["loss"])) and math.isfinite(float(rec["val_iou"])) and float(rec["loss"]) > 0, rec
