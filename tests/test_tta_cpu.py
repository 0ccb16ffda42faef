"""Host-only checks of test-time augmentation: the numpy restatement tests/tta_cases.py (what tests/test_tta_gpu.py holds the
kernels to) is self-consistent and agrees with the geometry the input pipeline's tests pin, the two C entries are declared and
bound, and EvalStep refuses a bad tta / tta_merge before it touches the device."""
import os
import re

import numpy as np
import pytest

import nunet_amd
from nunet_amd import _lib as L
from nunet_amd import trainer as T
import pipeline_cases as P
import tta_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("code", TC.ALL_CODES)
def test_unview_inverts_view(code):
    for h, w in ((5, 5), (1, 1)) + (((3, 7), (6, 1)) if not code & 1 else ()):
        x = TC.ramp(2, 3, h, w)
        v = TC.view(x, code)
        assert v.shape == ((2, 3, w, h) if code & 1 else (2, 3, h, w))
        assert np.array_equal(TC.unview(v, code), x)
        assert np.array_equal(TC.view(TC.unview(x.reshape(v.shape), code), code), x.reshape(v.shape))


def test_the_named_sets_hold_distinct_maps():
    """"d4" is the eight distinct maps of a square, "flips" four distinct maps of any rectangle, and the sets EvalStep runs are
    those of the restatement; every code 8 .. 15 repeats a map of 0 .. 7 (which is why "d4" stops at 7)."""
    assert T.TTA_SETS == {"flips": TC.FLIPS, "d4": TC.D4}
    sq, rect = TC.ramp(1, 1, 4, 4), TC.ramp(1, 1, 3, 5)
    assert len({TC.view(sq, c).tobytes() for c in TC.D4}) == 8
    assert len({TC.view(rect, c).tobytes() for c in TC.FLIPS}) == 4
    assert {TC.view(sq, c).tobytes() for c in TC.ALL_CODES} == {TC.view(sq, c).tobytes() for c in TC.D4}


@pytest.mark.parametrize("h,w", [(5, 5), (3, 7), (7, 3), (1, 6)])
def test_view_is_the_pipeline_geometry(h, w):
    """view() on CHW planes equals pipeline_cases' expected output (HWC, uint8 ramp) for every code the shape admits"""
    u = np.arange(h * w * 3).astype(np.uint8).reshape(h, w, 3)          # (at most 63 values: every byte distinct)
    for code in P.codes_for(h, w):
        exp = P.ref_geometry(u, code).astype(np.float32).transpose(2, 0, 1)
        got = TC.view(u.astype(np.float32).transpose(2, 0, 1), code)
        assert np.array_equal(got, exp), code


def test_merges_of_one_identity_view():
    x = TC.planted_logits((1, 1, 4, 6), -8, 8, 3, specials=False)
    assert np.array_equal(TC.merge_logit([x], [0]).view(np.uint32), x.view(np.uint32))
    assert np.abs(TC.merge_prob64([x], [0]) - x).max() < 1e-5          # logit(sigmoid(x)) = x up to the fp32 input's own rounding
    z = np.full((1, 1, 2, 2), -0.0, np.float32)
    assert np.signbit(TC.merge_logit([z, z], [0, 4])).all()             # the sum starts from the first view: -0 + -0


def test_entries_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nunet.h")).read()
    for name, nargs in (("nunet_dihedral_nchw", 8), ("nunet_tta_merge", 11)):
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "%s is not declared in include/nunet.h" % name
        assert len(m.group(1).split(",")) == nargs
        assert name in L._SIG and len(L._SIG[name][1]) == nargs
    assert re.search(r"NUNET_TTA_LOGIT\s*=\s*0\s*,\s*NUNET_TTA_PROB\s*=\s*1", hdr)
    assert (L.TTA_LOGIT, L.TTA_PROB) == (0, 1)
    assert T.TTA_MERGES == {"logit": L.TTA_LOGIT, "prob": L.TTA_PROB}
    mk = open(os.path.join(ROOT, "pytorch_nested-unet_amd", "csrc", "Makefile")).read()
    assert "tta.hip" in mk


def test_tta_codes():
    assert T.tta_codes(None, 32, 48) is None
    assert T.tta_codes("flips", 32, 48) == (0, 4, 8, 12)
    assert T.tta_codes("d4", 32, 32) == (0, 1, 2, 3, 4, 5, 6, 7)
    assert T.tta_codes([2, 14], 32, 48) == (2, 14)
    assert T.tta_codes((0,), 32, 48) == (0,)


@pytest.mark.parametrize("kw,shape,match", [
    (dict(tta="rot"), (2, 3, 32, 32), "is not one of"),
    (dict(tta=()), (2, 3, 32, 32), "empty"),
    (dict(tta=(0, 16)), (2, 3, 32, 32), "outside 0 .. 15"),
    (dict(tta=(-1,)), (2, 3, 32, 32), "outside 0 .. 15"),
    (dict(tta=(1.0,)), (2, 3, 32, 32), "outside 0 .. 15"),
    (dict(tta=4), (2, 3, 32, 32), "is not one of"),
    (dict(tta="d4"), (2, 3, 32, 48), "H == W"),
    (dict(tta=(0, 7)), (2, 3, 32, 48), "H == W"),
    (dict(tta="flips", tta_merge="mean"), (2, 3, 32, 32), "tta_merge"),
    (dict(tta_merge="probs"), (2, 3, 32, 32), "tta_merge"),
])
def test_evalstep_refuses_before_touching_the_device(kw, shape, match):
    """a module on the CPU: anything past the argument checks would raise something else (there is no CPU path)"""
    model = nunet_amd.archs.NestedUNet(1, 3)
    with pytest.raises(L.NunetError, match=match):
        T.EvalStep(model, shape, **kw)
