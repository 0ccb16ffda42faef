"""Test-time augmentation on the MI355X: nunet_dihedral_nchw and nunet_tta_merge against the numpy restatement
tests/tta_cases.py, EvalStep(tta=...) against the manual composition (the module's own eval forward on torch.rot90 /
torch.flip views, un-viewed and merged in fp32 in order), and val.py --tta / train.py --val_tta end to end.

Equalities are equalities of BITS, with two exceptions that carry their own bound:
  * the PROB merge is held, in logit space, to 2 * e32 + 2^-20 of the fp64 definition, e32 being what the SAME formula costs
    in fp32 numpy on the same case (the device's expf / logf may be an ulp or two off numpy's; the floor covers e32 == 0);
  * dice is compared the way tests/test_eval_gpu.py compares it (4e-6 of the fp64 restatement on the same logits).
Every figure is printed before it is asserted.

    python tests/test_tta_gpu.py --record profiles/tta_parity.json      writes the PROB maxima of prob_parity()"""
import functools
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.metrics import iou_logit_threshold, sigmoid_masks_u8  # noqa: E402
from nunet_amd.trainer import EvalStep  # noqa: E402
from nunet_amd.utils import AverageMeter  # noqa: E402
import eval_cases as EC  # noqa: E402
import tta_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DICE_REL = 4e-6                      # tests/test_eval_gpu.py
COUNTS = ("tp", "fp", "fn", "tn")
NUNET_EINVAL = -1


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate with a torch factory - EvalStep's included - sits between guard bands that are
    checked after the test (conftest.py)"""
    yield


def dev(a):
    """numpy -> a device tensor allocated through torch.empty (inside guard bands while the fixture is active)"""
    a = np.ascontiguousarray(a)
    t = torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=DEV)
    t.copy_(torch.from_numpy(a))
    return t


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dihedral(src, code):
    n, c, h, w = src.shape
    dst = torch.full((n, c, w, h) if code & 1 else (n, c, h, w), float("nan"), device=DEV)
    L.check(L.lib().nunet_dihedral_nchw(L.ptr(src), n, c, h, w, code, L.ptr(dst), L.stream()), "nunet_dihedral_nchw")
    return dst


def merge(views, codes, hw, mode, acc=None):
    """successive nunet_tta_merge calls in index order into an accumulator poisoned with NaN (no pre-zeroing is relied on)"""
    n, k = views[0].shape[:2]
    if acc is None:
        acc = torch.full((n, k) + tuple(hw), float("nan"), device=DEV)
    for i, (v, c) in enumerate(zip(views, codes)):
        L.check(L.lib().nunet_tta_merge(L.ptr(v), n, k, hw[0], hw[1], c, mode, i, len(codes), L.ptr(acc), L.stream()), "nunet_tta_merge")
    return acc


# -- 1. nunet_dihedral_nchw ---------------------------------------------------------------------------------------------------------
# edge tiles on both axes (33), a plane smaller than a tile, more than one tile per plane (64), several planes; the last square
# shape has 1030 planes x 4 tiles = 4120 items, past the 4096-workgroup cap: some workgroups take a second trip
SQUARE = [(3, 2, 33, 33), (1, 1, 1, 1), (2, 1, 31, 31), (1, 5, 64, 64)]
RECT = [(2, 3, 16, 48), (1, 1, 33, 7)]
DIHEDRAL_CASES = [(s, c) for s in SQUARE for c in TC.ALL_CODES] + [(s, c) for s in RECT for c in TC.EVEN_CODES] + [((1030, 1, 33, 33), c) for c in (3, 6)]


@pytest.mark.parametrize("shape,code", DIHEDRAL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "code%d" % v)
def test_dihedral(shape, code):
    x = TC.ramp(*shape)
    got = dihedral(dev(x), code).cpu().numpy()
    exp = TC.view(x, code)
    assert got.shape == exp.shape
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(got != exp)[:4]


def test_dihedral_moves_bits():
    """a bit copy: NaN payloads, infinities, denormals and -0 arrive as they are"""
    raw = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0x7F7FFFFF, 0x3F800000, 0x807FFFFF], dtype=np.uint32)
    x = np.resize(raw, 2 * 33 * 33).reshape(1, 2, 33, 33).view(np.float32)
    for code in (0, 5, 10):
        got = dihedral(dev(x), code).cpu().numpy()
        assert np.array_equal(bits(got), bits(TC.view(x, code)))


def test_bad_arguments_launch_nothing():
    lib, st = L.lib(), L.stream()
    src = dev(TC.ramp(1, 2, 8, 8))
    rect = dev(TC.ramp(1, 2, 8, 12))
    out = torch.full((1, 2, 8, 12), 7.0, device=DEV)
    s, r, o = L.ptr(src), L.ptr(rect), L.ptr(out)
    bad_dihedral = [(None, 1, 2, 8, 8, 0, o), (s, 1, 2, 8, 8, 0, None), (s, 0, 2, 8, 8, 0, o), (s, 1, 0, 8, 8, 0, o), (s, 1, 2, 0, 8, 0, o),
                    (s, 1, 2, 8, -1, 0, o), (s, 1, 2, 8, 8, 16, o), (s, 1, 2, 8, 8, -1, o), (r, 1, 2, 8, 12, 1, o), (r, 1, 2, 8, 12, 7, o),
                    (o, 1, 2, 8, 12, 4, o)]
    for a in bad_dihedral:
        assert lib.nunet_dihedral_nchw(*a, st) == NUNET_EINVAL, a
        assert b"dihedral_nchw" in lib.nunet_last_error()
    # (view, N, K, H, W, code, mode, view_index, views, acc)
    bad_merge = [(None, 1, 2, 8, 12, 0, 0, 0, 1, o), (r, 1, 2, 8, 12, 0, 0, 0, 1, None), (r, 0, 2, 8, 12, 0, 0, 0, 1, o), (r, 1, -2, 8, 12, 0, 0, 0, 1, o),
                 (r, 1, 2, 0, 12, 0, 0, 0, 1, o), (r, 1, 2, 8, 0, 0, 0, 0, 1, o), (r, 1, 2, 8, 12, 16, 0, 0, 1, o), (r, 1, 2, 8, 12, -4, 0, 0, 1, o),
                 (r, 1, 2, 8, 12, 3, 0, 0, 1, o), (r, 1, 2, 8, 12, 0, 2, 0, 1, o), (r, 1, 2, 8, 12, 0, -1, 0, 1, o), (r, 1, 2, 8, 12, 0, 0, -1, 1, o),
                 (r, 1, 2, 8, 12, 0, 0, 1, 1, o), (r, 1, 2, 8, 12, 0, 0, 4, 4, o), (r, 1, 2, 8, 12, 0, 0, 0, 0, o), (r, 1, 2, 8, 12, 0, 1, 0, -3, o),
                 (o, 1, 2, 8, 12, 0, 0, 0, 1, o)]
    for a in bad_merge:
        assert lib.nunet_tta_merge(*a, st) == NUNET_EINVAL, a
        assert b"tta_merge" in lib.nunet_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -- 2. round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,codes", [((2, 2, 33, 33), TC.ALL_CODES), ((2, 2, 16, 48), TC.EVEN_CODES)], ids=["33x33", "16x48"])
def test_round_trip(shape, codes):
    """the view, merged alone (views = 1, LOGIT: x / 1), is the source bit for bit: the merge undoes what the view did"""
    x = TC.planted_logits(shape, -20, 20, 11, specials=False)
    xd = dev(x)
    for code in codes:
        back = merge([dihedral(xd, code)], [code], shape[2:], L.TTA_LOGIT).cpu().numpy()
        assert np.array_equal(bits(back), bits(x)), code


# -- 3. merges ----------------------------------------------------------------------------------------------------------------------
MERGE_CASES = [("d4", TC.D4, (2, 2, 33, 33)), ("flips", TC.FLIPS, (2, 1, 16, 48))]


def _views(codes, shape, lo, hi, specials):
    """one tensor of logits per view, in the view's frame: independent draws in the SOURCE frame (nothing cancels by symmetry),
    each taken to its view, so that the planted values of all views meet at the same source pixels"""
    return [TC.view(TC.planted_logits(shape, lo, hi, 100 + i, specials), c) for i, c in enumerate(codes)]


@pytest.mark.parametrize("name,codes,shape", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_logit(name, codes, shape):
    views = _views(codes, shape, -20, 20, True)
    exp = TC.merge_logit(views, codes)
    vd = [dev(v) for v in views]
    got = merge(vd, codes, shape[2:], L.TTA_LOGIT).cpu().numpy()
    nan = np.isnan(exp)
    zero = exp == 0
    assert nan.sum() == 2 and np.isposinf(exp).any() and np.isneginf(exp).any() and np.signbit(exp[zero]).sum() == 1 and zero.sum() == 3, \
        "the planted values did not survive into the case"
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(exp)[~nan]), np.argwhere((bits(got) != bits(exp)) & ~nan)[:4]
    again = merge(vd, codes, shape[2:], L.TTA_LOGIT).cpu().numpy()
    assert np.array_equal(bits(again), bits(got))


def prob_parity():
    """{case: figures} of the PROB merge against merge_prob64, in logit space, next to fp32 numpy's error on the same case"""
    out = {}
    for name, codes, shape in MERGE_CASES:
        views = _views(codes, shape, -8, 8, False)
        ref = TC.merge_prob64(views, codes)
        e32 = float(np.abs(TC.merge_prob32(views, codes).astype(np.float64) - ref).max())
        vd = [dev(v) for v in views]
        got = merge(vd, codes, shape[2:], L.TTA_PROB).cpu().numpy()
        again = merge(vd, codes, shape[2:], L.TTA_PROB).cpu().numpy()
        out[name] = {"shape": list(shape), "codes": list(codes), "finite": bool(np.isfinite(got).all()),
                     "repeatable": bool(np.array_equal(bits(got), bits(again))),
                     "device_max_abs_err": float(np.abs(got.astype(np.float64) - ref).max()), "numpy_fp32_max_abs_err": e32,
                     "bound": 2 * e32 + 2.0 ** -20, "max_abs_merged_logit": float(np.abs(ref).max())}
    return out


def test_merge_prob():
    """Measured on an MI355X (profiles/tta_parity.json), max |merged logit - fp64| device / fp32 numpy:
        d4    [2, 2, 33, 33]   1.026e-06 / 1.026e-06   (bound 3.006e-06)
        flips [2, 1, 16, 48]   1.628e-05 / 1.628e-05   (bound 3.352e-05)"""
    for name, f in prob_parity().items():
        print("PROB %s: device max err %.3e, fp32 numpy max err %.3e, bound %.3e" % (name, f["device_max_abs_err"], f["numpy_fp32_max_abs_err"], f["bound"]))
        assert f["finite"] and f["repeatable"], (name, f)
        assert f["device_max_abs_err"] <= f["bound"], (name, f)


def test_merge_prob_saturated():
    """All logits +30: every fp32 sigmoid is 1, the mean is clamped to 1 - 2^-23 and the merged logit is finish(1 - 2^-23) =
    log(1 - 2^-23) + 23 log 2 = 15.94238...: finite. Bound against the fp64 value: logf within 1 ulp of a term of 1.2e-7,
    log1pf within 2 ulp of 15.94 and the subtraction's rounding, half an ulp - 2.5 ulp(15.94) = 2.5 * 2^-20 (the accuracy
    the OpenCL specification asks of log and log1p); and one value everywhere."""
    codes, shape = TC.FLIPS, (2, 1, 16, 48)
    vd = [torch.full(shape, 30.0, device=DEV) for _ in codes]
    got = merge(vd, codes, shape[2:], L.TTA_PROB).cpu().numpy()
    want = float(TC.finish_prob(np.float64(TC.P_HI), np.float64))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("saturated: merged logit %.9g, finish(1 - 2^-23) = %.9g, max err %.3e" % (got.flat[0], want, err))
    assert np.isfinite(got).all() and len(np.unique(bits(got))) == 1
    assert err <= 2.5 * 2.0 ** -20
    neg = merge([torch.full(shape, -120.0, device=DEV) for _ in codes], codes, shape[2:], L.TTA_PROB).cpu().numpy()
    assert np.isfinite(neg).all() and abs(float(neg.flat[0]) + want) <= 2.5 * 2.0 ** -20      # the lower clamp: p = 2^-23


# -- 4. EvalStep(tta=...) -----------------------------------------------------------------------------------------------------------
def tview(x, code):
    """tta_cases.view with torch calls, on the device"""
    out = torch.rot90(x, code & 3, (2, 3))
    if code & 4:
        out = out.flip(3)
    if code & 8:
        out = out.flip(2)
    return out.contiguous()


def _model(ncls, ds):
    st = nunet_amd.synth.closed_form_state(ncls, 3, ds, False)
    m = nunet_amd.archs.NestedUNet(ncls, 3, ds, dtype="fp32")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


def manual_logits(model, xb, codes, depth=None):
    """[heads, n, K, H, W] fp32 numpy: the module's own eval forward on every view, un-viewed and merged in fp32 in order"""
    views = []
    with torch.no_grad():
        for c in codes:
            out = model(tview(xb, c)) if depth is None else model(tview(xb, c), depth=depth)
            heads = list(out) if isinstance(out, (list, tuple)) else [out]
            views.append(torch.stack(heads).cpu().numpy())
    return TC.merge_logit(views, codes)


def manual_pass(model, x, t, codes, n, loss, thr, depth=None):
    """the validation loop of train.py validate() on the merged logits -> (result dict with "heads", [merged logits per batch])"""
    crit = getattr(nunet_amd.losses, loss)()
    M = nunet_amd.metrics
    names = ("loss", "iou", "dice", "acc")
    avg = {nm: AverageMeter() for nm in names}
    heads_avg, counts, heads_counts, merged_all = None, None, None, []
    for k in range(0, x.size(0), n):
        xb, tb = x[k:k + n].contiguous(), t[k:k + n].contiguous()
        merged = manual_logits(model, xb, codes, depth)
        merged_all.append(merged)
        md = torch.from_numpy(merged).to(DEV)
        nh, nb = md.size(0), xb.size(0)
        if heads_avg is None:
            heads_avg = [{nm: AverageMeter() for nm in names} for _ in range(nh)]
            heads_counts = [{nm: [0] * tb.size(1) for nm in COUNTS} for _ in range(nh)]
        per = [crit(md[j], tb) for j in range(nh)]
        avg["loss"].update((sum(per) / nh).item() if nh > 1 else per[0].item(), nb)
        for j in range(nh):
            r = EC.restate(md[j].cpu(), tb.cpu(), thr)
            iou, dice, acc = EC.batch_values(r, md[j].numel())
            assert iou == M.iou_from_counts(M.iou_counts(md[j].contiguous(), tb))
            for nm, v in (("loss", per[j].item()), ("iou", iou), ("dice", dice), ("acc", acc)):
                heads_avg[j][nm].update(v, nb)
            for nm in COUNTS:
                heads_counts[j][nm] = [a + b for a, b in zip(heads_counts[j][nm], r[nm])]
            if j == nh - 1:
                for nm, v in (("iou", iou), ("dice", dice), ("acc", acc)):
                    avg[nm].update(v, nb)
    out = {nm: avg[nm].avg for nm in names}
    out["counts"] = heads_counts[-1]
    out["heads"] = [dict({nm: h[nm].avg for nm in names}, counts=c) for h, c in zip(heads_avg, heads_counts)]
    return out, merged_all


def check_fields(what, got, want):
    print("%s: loss %.9g (manual %.9g) iou %.9g (%.9g) dice %.9g (%.9g) acc %.9g (%.9g)"
          % (what, got["loss"], want["loss"], got["iou"], want["iou"], got["dice"], want["dice"], got["acc"], want["acc"]))
    assert got["loss"] == want["loss"] and got["iou"] == want["iou"] and got["acc"] == want["acc"], (what, got, want)
    assert abs(got["dice"] - want["dice"]) <= DICE_REL * abs(want["dice"]), (what, got["dice"], want["dice"])
    assert {nm: list(v) for nm, v in got["counts"].items()} == want["counts"], what


def step_logits(ev, x, t):
    """begin() / step() by hand over the split -> [logits [heads, nb, K, H, W] numpy per batch]"""
    out = []
    ev.begin()
    for k in range(0, x.size(0), ev.n):
        ev.step(x[k:k + ev.n], t[k:k + ev.n])
        out.append(ev._last.logits.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def _case(tag):
    """-> (model, x, t, tta, codes, loss, EvalStep kwargs), built once and shared: do not write to them.
    A: NestedUNet(1, 3, deep_supervision=True), [2, 3, 32, 32], "d4", per_head;  B: NestedUNet(2, 3), [2, 3, 32, 48], "flips"."""
    ncls, ds, h, w, tta, kw = {"A": (1, True, 32, 32, "d4", dict(per_head=True)), "B": (2, False, 32, 48, "flips", {})}[tag]
    model = _model(ncls, ds)
    img, msk = nunet_amd.synth.synth_split(5, h, w, 3, ncls, seed=2000)
    x, t = torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)
    return model, x, t, tta, {"d4": TC.D4, "flips": TC.FLIPS}[tta], "BCEDiceLoss", kw


@pytest.mark.parametrize("tag", ["A", "B"])
def test_eval_step_tta_is_the_manual_composition(tag):
    """5 images at n = 2 (2, 2 and an eager tail of 1), captured: the merged logits of every batch and every head are the manual
    composition's bit for bit, result() (and its per-head entries) are the losses / metrics of those logits, the eager form
    agrees with the captured one in every bit and a second pass repeats the first."""
    model, x, t, tta, codes, loss, kw = _case(tag)
    thr = iou_logit_threshold()
    shape = (2, 3) + tuple(x.shape[2:])
    want, merged = manual_pass(model, x, t, codes, 2, loss, thr)
    ev = EvalStep(model, shape, loss=loss, tta=tta, **kw)
    assert ev.tta == codes
    got_logits = step_logits(ev, x, t)
    got = ev.result()
    assert ev.main.graph is not None and ev.tail.n == 1 and ev.tail.graph is None
    assert tuple(ev.logits.shape) == (ev.heads, 2, t.size(1)) + tuple(x.shape[2:]) and tuple(ev.last_logits.shape) == (1, t.size(1)) + tuple(x.shape[2:])
    for b, (g, m) in enumerate(zip(got_logits, merged)):
        assert g.shape == m.shape
        assert np.array_equal(bits(g), bits(m)), (tag, "batch", b, float(np.abs(g - m).max()))
    assert got["samples"] == 5
    check_fields(tag, got, want)
    if kw.get("per_head"):
        assert len(got["heads"]) == 4
        for j, (gh, wh) in enumerate(zip(got["heads"], want["heads"])):
            check_fields("%s head %d" % (tag, j + 1), gh, wh)
    assert repr(ev.evaluate(x, t)) == repr(got)
    eager = EvalStep(model, shape, loss=loss, tta=tta, use_graph=False, **kw)
    eager_logits = step_logits(eager, x, t)
    assert eager.main.graph is None and repr(eager.result()) == repr(got)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(eager_logits, got_logits))


def test_eval_step_tta_identity_is_the_plain_step():
    model, x, t, _, _, loss, _ = _case("B")
    shape = (2, 3) + tuple(x.shape[2:])
    plain, ident = EvalStep(model, shape, loss=loss), EvalStep(model, shape, loss=loss, tta=(0,))
    a, b = step_logits(plain, x, t), step_logits(ident, x, t)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
    assert repr(plain.result()) == repr(ident.result())
    assert not hasattr(plain.main, "x_view") and ident.main.x_view.shape == plain.main.x.shape


def test_eval_step_tta_one_by_one():
    """The five images of case B in a pass at n = 2 (2, 2 and the eager tail of 1) and one by one through an EvalStep of n = 1:
    the same merged logits bit for bit, image by image (at this shape no layer of the fp32 forward splits its reduction by N),
    and the same counts."""
    model, x, t, tta, codes, loss, _ = _case("B")
    shape = (2, 3) + tuple(x.shape[2:])
    both = EvalStep(model, shape, loss=loss, tta=tta)
    pair = np.concatenate(step_logits(both, x, t), axis=1)
    single = EvalStep(model, (1,) + shape[1:], loss=loss, tta=tta)
    one = np.concatenate(step_logits(single, x, t), axis=1)
    assert one.shape == pair.shape == (1, 5, 2, 32, 48)
    print("n = 1 against n = 2: max |difference| of the merged logits %.3e" % float(np.abs(one - pair).max()))
    assert np.array_equal(bits(one), bits(pair))
    r1, r2 = single.result(), both.result()
    assert r1["samples"] == r2["samples"] == 5 and r1["counts"] == r2["counts"]


def test_eval_step_tta_with_depth_and_weights():
    """depth=2 and weights= under "flips": the manual composition through model(x, depth=2), and through a second module that
    owns the other weights"""
    model, x, t, _, _, loss, _ = _case("A")
    thr = iou_logit_threshold()
    shape = (2, 3, 32, 32)
    want, merged = manual_pass(model, x, t, TC.FLIPS, 2, loss, thr, depth=2)
    ev = EvalStep(model, shape, loss=loss, tta="flips", depth=2)
    got_logits = step_logits(ev, x, t)
    assert ev.heads == 1 and all(np.array_equal(bits(g), bits(m)) for g, m in zip(got_logits, merged))
    check_fields("depth 2", ev.result(), want)
    other = _model(1, True)
    with torch.no_grad():
        other.final4.weight.mul_(-0.75)
        other.conv0_0.conv1.weight.mul_(1.25)
    want, merged = manual_pass(other, x, t, TC.FLIPS, 2, loss, thr)
    eng = other.engine()
    ev = EvalStep(model, shape, loss=loss, tta="flips", weights=(eng.flat_params, eng.bnbuf))
    got_logits = step_logits(ev, x, t)
    assert ev.heads == 4 and all(np.array_equal(bits(g), bits(m)) for g, m in zip(got_logits, merged))
    check_fields("weights", ev.result(), want)


# -- 5. drivers ---------------------------------------------------------------------------------------------------------------------
def test_val_py_tta(tmp_path):
    """train.py --val_tta flips for one epoch at 32 x 32 as a child process under a time limit, then val.py --tta flips on its
    checkpoint: IoU / Dice / Acc lines, and every mask file is the JPEG of sigmoid_masks_u8 of the manually merged logits, byte
    for byte; --full_res true --tta flips and train.py --val_tta flips --eval_step false exit non-zero with their message."""
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--epochs", "1", "--train_size", "8", "--val_size", "6", "--batch_size", "4",
            "--input_h", "32", "--input_w", "32", "--name", "tta_e2e", "--val_tta", "flips"]
    r = subprocess.run(base, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "test-time augmentation flips (4 views)" in r.stdout
    val = [sys.executable, os.path.join(ROOT, "val.py"), "--name", "tta_e2e", "--tta", "flips"]
    v = subprocess.run(val, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert v.returncode == 0, (v.stdout[-3000:], v.stderr[-3000:])
    lines = [ln for ln in v.stdout.strip().split("\n") if ln]
    assert "tta: flips (4 views, merged as logit)" in lines
    assert [ln.split(":")[0] for ln in lines[-3:]] == ["IoU", "Dice", "Acc"], lines[-5:]
    assert all(math.isfinite(float(ln.split(":")[1])) for ln in lines[-3:])
    # the masks: the checkpoint through the manual composition, in val.py's batches (4 and a tail of 2)
    model = nunet_amd.archs.NestedUNet(1, 3, False)
    model.load_state_dict(torch.load(os.path.join(str(tmp_path), "models", "tta_e2e", "model.pth"), map_location="cpu"))
    model = model.to(DEV).eval()
    img, _ = nunet_amd.synth.synth_split(6, 32, 32, 3, 1, seed=2000)
    x = torch.from_numpy(img).to(DEV)
    out_dir = os.path.join(str(tmp_path), "outputs", "tta_e2e", "0")
    assert sorted(os.listdir(out_dir)) == ["val_%04d.jpg" % i for i in range(6)]
    for k in (0, 4):
        merged = manual_logits(model, x[k:k + 4].contiguous(), TC.FLIPS)[-1]
        masks = sigmoid_masks_u8(torch.from_numpy(merged).to(DEV)).cpu().numpy()
        for i in range(masks.shape[0]):
            buf = io.BytesIO()
            Image.fromarray(masks[i, 0]).save(buf, format="JPEG")
            assert open(os.path.join(out_dir, "val_%04d.jpg" % (k + i)), "rb").read() == buf.getvalue(), k + i
    f = subprocess.run(val + ["--full_res", "true"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert f.returncode != 0 and "--full_res true does not combine with --tta flips" in f.stdout, (f.stdout[-2000:], f.stderr[-2000:])
    e = subprocess.run(base + ["--eval_step", "false"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert e.returncode != 0 and "--val_tta flips" in e.stderr and "--eval_step true" in e.stderr, (e.stdout[-2000:], e.stderr[-2000:])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, help="write prob_parity() here as JSON")
    a = ap.parse_args()
    figures = prob_parity()
    torch.cuda.synchronize()
    print(json.dumps(figures))
    os.makedirs(os.path.dirname(a.record) or ".", exist_ok=True)
    with open(a.record, "w") as f:
        json.dump(figures, f, indent=1)
        f.write("\n")
