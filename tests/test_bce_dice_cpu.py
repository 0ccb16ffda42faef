"""CPU-side checks of tests/loss_cases.py, the module the BCE-Dice GPU tests (tests/test_bce_dice_gpu.py) stand on: its fp64
reference reproduces the reference goldens and the numpy restatement, every case claims the launch regime the kernels' grid
formulas give it, and an fp32 evaluation of the kernels' formulas stays within the per-pixel gradient bound with c = 2 - half of
what the GPU test allows the device."""
import numpy as np
import pytest
import torch

import loss_cases as LC
from conftest import load_golden

C_EMULATION = 2.0


def test_reference_reproduces_the_goldens():
    """the goldens hold the reference's own fp32 results: loss to 2e-6, gradient at the tolerance tests/test_ops_gpu.py holds the
    device to; oracle.bce_dice_loss_np (numpy, no torch) agrees with the fp64 reference to rounding"""
    from oracle import nunet_oracle as O
    g = load_golden("small_ops")
    for tag in ("k1", "k4"):
        x, t = torch.from_numpy(g["x_" + tag]), torch.from_numpy(g["t_" + tag])
        n = x.shape[0]
        loss, dx, I, P, T = LC.oracle(x.reshape(n, -1), t.reshape(n, -1))
        assert abs(loss - float(g["loss_" + tag])) < 2e-6
        np.testing.assert_allclose(dx.numpy().reshape(x.shape), g["dx_" + tag], atol=2e-9, rtol=2e-4)
        assert abs(loss - O.bce_dice_loss_np(x.numpy(), t.numpy())) < 1e-13
        assert loss == LC.oracle(x.reshape(n, -1).contiguous(), t.reshape(n, -1))[0]


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_case_claims_the_regime_the_grid_formulas_give(case):
    kind, n, per, heads, pattern = case
    assert LC.REGIME[case] == LC.expected_regime(kind, per), (LC.REGIME[case], LC.expected_regime(kind, per))
    x, t = LC.build(case)
    assert tuple(t.shape) == (n, per) and tuple(x.shape) == ((heads, n, per) if kind == "fused" else (n, per))
    assert x.dtype == torch.float32 and t.dtype == torch.float32
    assert LC.build(case)[0] is x                      # cached: one tensor per case


def test_case_list_reaches_every_regime():
    """what the list is for, stated on the claimed figures: stand-alone gx of 1, 2 and the cap with even and uneven trips and a
    fifth trip; fused gx of 1, 2, 9 and the cap with one, two and five trips; the owning block's image counts; heads up to 8"""
    alone = {LC.REGIME[c] for c in LC.ALONE_CASES}
    fused = {LC.REGIME[c] for c in LC.FUSED_CASES}
    assert {(1, 1, 0), (2, 3, 2), (3, 3, 2), (64, 4, 4), (64, 5, 4), (64, 65, 64), (1, 2, 1), (9, 4, 4)} <= alone
    assert {(1, 1, 0), (2, 1, 0), (9, 1, 0), (64, 1, 1), (64, 2, 1), (64, 5, 4)} <= fused
    assert {c[1] for c in LC.FUSED_CASES if c[2] == 300} == {1, 4, 5, 16, 17, 33}
    assert {c[3] for c in LC.FUSED_CASES} == {1, 2, 4, 8}
    assert max(c[1] for c in LC.ALONE_CASES) == 33
    assert LC.EDGE_CASE in LC.FUSED_CASES
    assert len(set(LC.CASES)) == len(LC.CASES)
    for kind, shape in (("alone", LC.ALONE_PATTERN_SHAPE), ("fused", LC.FUSED_PATTERN_SHAPE)):
        assert {c[4] for c in LC.CASES if c[0] == kind and c[1:3] == shape[:2]} >= set(LC.PATTERNS)


def test_patterns_are_what_they_are_named_for():
    for case in (c for c in LC.CASES if c[4] != "rand"):
        x, t = LC.build(case)
        x = x.reshape(-1, *t.shape)
        pattern, per = case[4], case[2]
        if pattern == "empty_full":
            assert not t[0].any() and bool((t[1] == 1).all())
        elif pattern == "saturated":
            assert bool((x[:, 0] == -30).all() and (x[:, 1] == 30).all() and (x[:, 2] == -30).all())
            assert t.sum(1).tolist() == [0, per, per]
            D = float(torch.sigmoid(x[0, 0].double()).sum()) + 1e-5
            assert 1e-5 < D < 1.03e-5 and 1 / D ** 2 > 9e9
        elif pattern == "wide":
            assert 35 < float(x.std()) < 45 and float(x.abs().max()) > 120
        elif pattern == "beyond_exp":
            assert bool((x[:, 0] == -95).all() and (x[:, 1] == 95).all() and (x[:, 2, :per // 2] == -88.5).all())
            assert bool(torch.isinf(torch.exp(-x[:, 0])).all())            # past the fp32 exp range
        elif pattern == "soft":
            soft = (t > 0) & (t < 1)
            assert bool((t[soft] > 0.5).all()) and bool((x[-1][soft] < 0).all()) and 0.15 * t.numel() < int(soft.sum())
            assert bool((t == 0).any()) and bool((t == 1).any())
        elif pattern == "zeros":
            assert not x.any()
    x, _ = LC.build(LC.EDGE_CASE)
    assert np.array_equal(x[-1, 0, :235].numpy(), LC.iou_edges(), equal_nan=False)


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_fp32_emulation_stays_within_the_bound(case):
    """c = 2 for the kernels' formulas in fp32 with the host's exp / log1p and torch's sums; the ratio printed is the smallest c
    that would pass. The loss and the per-image sums at the figures the GPU test uses."""
    _, t = LC.build(case)
    per = case[2]
    for k in range(case[3]):
        x = LC.head(case, k)
        ref_loss, ref_dx, I, P, T = LC.reference(case, k)
        loss, dx, i32, p32, t32 = LC.emulate_fp32(x, t)
        ratio = LC.worst_ratio(dx.double(), ref_dx, LC.unit_of(case, k))
        print("%s head %d: emulation needs c = %.3f; |loss - ref| = %.2e" % (LC.case_id(case), k, ratio, abs(loss - ref_loss)))
        assert ratio <= C_EMULATION
        assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))
        tiny = 2.0 ** -126 * per
        for got, ref, atol in ((i32, I, tiny), (p32, P, tiny), (t32, T, 0.0)):
            assert bool(((got.double() - ref).abs() <= 2e-6 * ref.abs() + atol).all())


@pytest.mark.parametrize("case", LC.SOFT_UNIFORM_CASES, ids=LC.case_id)
def test_fp32_emulation_on_uniform_soft_targets(case):
    """targets uniform in [0, 1]: the two gradient terms cancel at some pixels, so the relative part of the bound is taken of the
    addends' magnitudes (loss_cases' docstring); c = 2 as everywhere. Printed beside it: the c the hard-label bound would need,
    the reason the "soft" pattern is not this one."""
    assert LC.REGIME[case] == LC.expected_regime(case[0], case[2]) and case not in LC.CASES
    x, t = LC.head(case, 0), LC.build(case)[1]
    assert 0 <= float(t.min()) < 0.01 and 0.99 < float(t.max()) <= 1 and len(torch.unique(t)) > case[2]
    ref_loss, ref_dx, I, P, T = LC.reference(case)
    loss, dx, i32, p32, t32 = LC.emulate_fp32(x, t)
    ratio = LC.worst_ratio(dx.double(), ref_dx, LC.unit_of(case), rel=LC.addend_magnitudes(x, t))
    m = LC.addend_magnitudes(x, t)
    print("%s: emulation needs c = %.3f by the addends' magnitudes (worst |dx - ref| / m = %.2e), %.3f by the hard-label bound; |loss - ref| = %.2e"
          % (LC.case_id(case), ratio, float(((dx.double() - ref_dx).abs() / m).max()), LC.worst_ratio(dx.double(), ref_dx, LC.unit_of(case)),
             abs(loss - ref_loss)))
    assert ratio <= C_EMULATION
    assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))
    for got, ref in ((i32, I), (p32, P), (t32, T)):
        assert bool(((got.double() - ref).abs() <= 2e-6 * ref.abs()).all())


def test_launch_info_query_on_the_host():
    """nunet_loss_launch_info needs no GPU: it gives every case the regime the list claims, covers the items
    (trips_min <= items / threads <= trips_max, one apart at the most) over a sweep of sizes, and refuses what the entries refuse"""
    import ctypes as C
    from nunet_amd import _lib as L
    lib = L.lib()
    o = L.LossLaunchInfo()
    for case in LC.CASES:
        kind, n, per, heads, _ = case
        for entry in ((L.LOSS_ENTRY_BCE_DICE_FWD, L.LOSS_ENTRY_BCE_DICE_BWD) if kind == "alone" else (L.LOSS_ENTRY_LOSS_STEP,)):
            assert lib.nunet_loss_launch_info(entry, n, per, heads, C.byref(o)) == 0
            assert (o.grid_x, o.trips_max, o.trips_min) == LC.REGIME[case] and (o.grid_y, o.grid_z, o.block, o.items) == (n, heads, 256, per)
    caps = {L.LOSS_ENTRY_BCE_DICE_FWD: 64, L.LOSS_ENTRY_BCE_DICE_BWD: 64, L.LOSS_ENTRY_LOSS_STEP: 64, L.LOSS_ENTRY_IOU_COUNTS: 256,
            L.LOSS_ENTRY_SIGMOID_U8: 2048}
    for entry, cap in caps.items():
        for size in [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16384, 16385, 65536, 65537, 262144, 262145, 2 ** 21, 2 ** 21 + 3073, 2 ** 24]:
            assert lib.nunet_loss_launch_info(entry, 2, size, 1, C.byref(o)) == 0
            threads = o.grid_x * o.block
            assert 1 <= o.grid_x <= cap and o.items == (size // 4 if entry == L.LOSS_ENTRY_SIGMOID_U8 else size)
            assert o.trips_min * threads <= o.items <= o.trips_max * threads and o.trips_max - o.trips_min <= 1
            assert o.grid_x == cap or o.trips_max <= (4 if entry in (L.LOSS_ENTRY_BCE_DICE_FWD, L.LOSS_ENTRY_BCE_DICE_BWD, L.LOSS_ENTRY_IOU_COUNTS) else 1)
    EINVAL = -1
    assert lib.nunet_loss_launch_info(L.LOSS_ENTRY_LOSS_STEP, 1, 2 ** 24 + 1, 1, C.byref(o)) == EINVAL and b"too large" in lib.nunet_last_error()
    assert lib.nunet_loss_launch_info(L.LOSS_ENTRY_BCE_DICE_FWD, 1, 2 ** 24 + 1, 1, C.byref(o)) == 0
    for bad in ((7, 1, 5, 1), (-1, 1, 5, 1), (L.LOSS_ENTRY_LOSS_STEP, 1, 5, 9), (L.LOSS_ENTRY_LOSS_STEP, 1, 5, 0), (L.LOSS_ENTRY_BCE_DICE_BWD, 0, 5, 1),
                (L.LOSS_ENTRY_IOU_COUNTS, 1, 0, 1)):
        assert lib.nunet_loss_launch_info(*bad, C.byref(o)) == EINVAL and lib.nunet_last_error()
    assert lib.nunet_loss_launch_info(L.LOSS_ENTRY_IOU_COUNTS, 1, 5, 1, None) == EINVAL
