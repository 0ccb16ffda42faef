"""The Lovasz-hinge test inputs (tests/lovasz_cases.py) and their fp64 reference, pinned before any device is involved: the
constructed errors survive fp32 exactly and are distinct inside every image, and oracle.lovasz_hinge - which differences
1 - I/U in fp64 as the reference does in fp32 - agrees with the increments' closed form, which has no cancellation."""
import numpy as np
import pytest
import torch

import lovasz_cases as LC

ALL = LC.CASES + [(LC.FUSED_SHAPE, "p30-head%d" % q) for q in range(LC.FUSED_HEADS)]


def _build(case):
    shape, pattern = case
    if pattern.startswith("p30-head"):                   # the heads of the fused-entry test: one target, a draw of errors each
        return LC.build(shape, "p30", int(pattern[8:]), ("p30", 0)), LC.reference(shape, "p30", int(pattern[8:]), ("p30", 0))
    return LC.build(shape, pattern), LC.reference(shape, pattern)


@pytest.mark.parametrize("case", ALL, ids=LC.case_id)
def test_cases_are_exact_in_fp32_and_tie_free_and_the_oracle_matches_the_closed_form(case):
    (x, t, e), (ref_loss, ref_dx) = _build(case)
    n = x.shape[0]
    x, t = x.reshape(n, -1), t.reshape(n, -1)
    assert x.dtype == torch.float32 and t.dtype == torch.float32 and set(t.unique().tolist()) <= {0.0, 1.0}
    e32 = 1.0 - x * (2.0 * t - 1.0)                      # the device's expression, in fp32
    assert e32.dtype == torch.float32 and torch.equal(e32.double(), e)
    for i in range(n):
        assert torch.unique(e32[i]).numel() == e.shape[1]
    if case[1] == "all_nonpos":
        assert float(e.max()) == 0.0
    elif e.shape[1] >= 3:
        assert bool((e == 0).any(1).all()) and bool((e < 0).any(1).all()) and bool((e > 0).any(1).all())
    loss, dx, zero = LC.closed_form(e, t)
    ref = ref_dx.numpy()
    assert abs(ref_loss - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.array_equal(ref == 0, zero)                # exact zeros exactly where the closed form says: e <= 0, or I == 0
    assert np.array_equal(np.signbit(ref[~zero]), t.numpy()[~zero] > 0.5)
    worst = LC.worst_rel(ref, dx)
    print("%s: oracle vs closed form, worst relative difference %.2e over %d nonzero entries" % (LC.case_id(case), worst, int((~zero).sum())))
    np.testing.assert_allclose(ref[~zero], dx[~zero], rtol=1e-8, atol=0)
    if case[1] == "all_nonpos":
        assert ref_loss == 0.0 and not ref.any()


@pytest.mark.parametrize("shape", LC.TIE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tie_cases_have_ties(shape):
    x, t = LC.build_ties(shape, "init")
    assert not x.any() and 0 < float(t.mean()) < 1
    x, t = LC.build_ties(shape, "quarter")
    assert torch.equal(x * 4, torch.round(x * 4))
    e = (1.0 - x * (2.0 * t - 1.0)).reshape(shape[0], -1)
    for i in range(shape[0]):
        vals, counts = torch.unique(e[i], return_counts=True)
        mixed = sum(1 for v in vals[counts > 1] if 0 < float(t.reshape(shape[0], -1)[i][e[i] == v].mean()) < 1)
        assert mixed >= 8 and bool((vals == 0).any())
