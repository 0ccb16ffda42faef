"""Host-side checks of the validation step (no GPU): the fp64 restatement of tests/eval_cases.py against the reference's own
numbers (tests/golden/eval_metrics.npz), the device structs' layout, the workspace queries, the launch geometry of
nunet_seg_metrics against the regime table, and every refusal of nunet_seg_metrics / nunet_eval_step - argument checks come
before any HIP call, so they are testable here with pointers that are never dereferenced."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

import nunet_amd
from nunet_amd import _lib as L
from nunet_amd.metrics import iou_logit_threshold, scores_from_counts

import eval_cases as EC
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUNET_OK, NUNET_EINVAL = 0, -1
P = lambda k=1: C.c_void_p(4096 * k)        # an aligned non-null pointer the refused call never touches


@pytest.fixture(scope="module")
def lib():
    return L.lib()


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_restatement_against_the_reference(case):
    """iou_score's value is a quotient of integer counts in double: the restatement equals it EXACTLY (which also pins the
    logit threshold to the reference's fp32 `sigmoid(x) > 0.5`, edge values included). dice_coef sums in float32 (numpy's
    pairwise sum: blocks of 128 elements on 8 accumulators, then a tree - under 16 + log2(n / 128) roundings per sum, 2^-24
    each, three sums and three fp32 operations): within 1e-6 relative of the fp64 restatement."""
    g = load_golden("eval_metrics")
    n, k, hw, pattern = case
    iou, dice, acc = EC.batch_values(EC.reference(case, iou_logit_threshold()), n * k * hw)
    assert iou == float(g["iou_" + EC.case_id(case)])
    ref = float(g["dice_" + EC.case_id(case)])
    if pattern == "nan":
        assert math.isnan(ref) and math.isnan(dice)
    else:
        assert abs(dice - ref) <= 1e-6 * abs(ref), (dice, ref)
    if pattern == "all_background":
        assert iou == 1.0 and acc == 1.0
    assert 0.0 <= acc <= 1.0


@pytest.mark.parametrize("tag", list(EC.NET))
def test_meter_restatement_against_the_reference(tag):
    """The AverageMeter restatement over the reference's per-batch values (batches of 4, 4, 2) gives the reference's averages.
    dice_coef returns a numpy float32, so the reference's meter of it runs in float32 (three products, two sums, a division:
    2^-22 relative); every other value is a python float and the meter a double."""
    g = load_golden("eval_metrics")
    names = ["bcedice", "bcelogits", "iou", "dice", "acc"] + (["lovasz"] if EC.NET[tag][0] == 1 else [])
    for nm in names:
        m = EC.Meter()
        for v, cnt in zip(g["%s_batches_%s" % (nm, tag)].tolist(), (4, 4, 2)):
            m.update(v, cnt)
        assert m.count == EC.NET_SPLIT[0]
        assert abs(m.avg - float(g["%s_%s" % (nm, tag)])) <= (2.0 ** -22 if nm == "dice" else 1e-12) * abs(m.avg), nm


def test_struct_layout():
    assert C.sizeof(L.SegSums) == 448
    assert C.sizeof(L.EvalMeters) == 512
    assert L.EvalMeters.tp.offset == 64 and L.EvalMeters.soft_i.offset == 64 + 4 * 64
    assert L.SegSums.fp.offset == 64 and L.SegSums.soft_t.offset == 448 - 64
    assert L.EVAL_MAX_CLASSES == EC.MAX_CLASSES == 8


def test_workspace_queries(lib):
    up = lambda v: (v + 255) // 256 * 256
    for n, k, hw in list(EC.SHAPES) + [(16, 1, 96 * 96)]:
        seg = lib.nunet_seg_metrics_ws_bytes(n, k, hw)
        assert seg == n * k * 64 * 40        # one {3 doubles, 4 uint32} entry per possible block of every plane
        for heads in (1, 4):
            for kind in (L.LOSS_BCE_DICE, L.LOSS_BCE_LOGITS) + ((L.LOSS_LOVASZ_HINGE,) if k == 1 else ()):
                head = {L.LOSS_BCE_DICE: lib.nunet_bce_dice_ws_bytes(n), L.LOSS_BCE_LOGITS: lib.nunet_bce_logits_ws_bytes(n * k * hw),
                        L.LOSS_LOVASZ_HINGE: lib.nunet_lovasz_ws_bytes(n, hw)}[kind]
                unit = up(n * hw * 4) if kind == L.LOSS_LOVASZ_HINGE else 0
                assert lib.nunet_eval_step_ws_bytes(n, k, hw, heads, kind) == heads * up(head) + unit + up(seg) + 512
    for bad in ((0, 1, 10), (1, 0, 10), (1, 9, 10), (1, 1, 0)):
        assert lib.nunet_seg_metrics_ws_bytes(*bad) == 0
        assert lib.nunet_eval_step_ws_bytes(*bad, 1, 0) == 0
    assert lib.nunet_eval_step_ws_bytes(1, 1, 10, 0, 0) == 0 and lib.nunet_eval_step_ws_bytes(1, 1, 10, 9, 0) == 0


@pytest.mark.parametrize("shape", list(EC.SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_launch_info_against_the_regime_table(lib, shape):
    n, k, hw = shape
    info = L.LossLaunchInfo()
    assert lib.nunet_seg_metrics_launch_info(n, k, hw, C.byref(info)) == NUNET_OK
    assert (info.grid_x, info.trips_max, info.trips_min) == EC.SHAPES[shape] == EC.expected_regime(hw)
    assert (info.grid_y, info.grid_z, info.block, info.items) == (k, n, 256, hw)


def test_final_workgroup_regimes():
    """the table reaches both regimes of the one-workgroup launch: every partial of a class in one trip, and a second trip"""
    trips = {s: EC.final_trips(s[0], s[2]) for s in EC.SHAPES}
    assert trips[(33, 8, 300)] == 1 and 33 * 8 > 256
    assert trips[(5, 1, 16384)] == 2
    assert set(trips.values()) == {1, 2}


def _refused(lib, rc, *words):
    assert rc == NUNET_EINVAL
    msg = lib.nunet_last_error()
    assert msg and all(w in msg for w in words), msg


def test_launch_info_refusals(lib):
    info = L.LossLaunchInfo()
    _refused(lib, lib.nunet_seg_metrics_launch_info(1, 1, 10, None), b"null")
    _refused(lib, lib.nunet_seg_metrics_launch_info(0, 1, 10, C.byref(info)), b"N = 0")
    _refused(lib, lib.nunet_seg_metrics_launch_info(1, 9, 10, C.byref(info)), b"9 classes")
    _refused(lib, lib.nunet_seg_metrics_launch_info(1, 1, 2 ** 24 + 1, C.byref(info)), b"pixels")
    assert lib.nunet_seg_metrics_launch_info(1, 8, 2 ** 24, C.byref(info)) == NUNET_OK and info.trips_max == 1024


def test_seg_metrics_refusals(lib):
    thr = iou_logit_threshold()
    ws = lib.nunet_seg_metrics_ws_bytes(2, 1, 300)
    call = lambda x=P(1), t=P(2), n=2, k=1, hw=300, w=P(3), wb=ws, out=P(4): lib.nunet_seg_metrics(x, t, n, k, hw, thr, w, wb, out, 0, None)
    _refused(lib, call(k=0), b"seg_metrics", b"0 classes")
    _refused(lib, call(k=9), b"seg_metrics", b"9 classes")
    _refused(lib, call(hw=2 ** 24 + 1), b"seg_metrics", b"pixels")
    _refused(lib, call(hw=0), b"seg_metrics", b"pixels")
    _refused(lib, call(n=0), b"seg_metrics", b"N = 0")
    _refused(lib, call(wb=ws - 1), b"seg_metrics", b"workspace", str(ws).encode())
    for name in ("x", "t", "w", "out"):
        _refused(lib, call(**{name: None}), b"seg_metrics", b"null pointer")
    _refused(lib, call(w=C.c_void_p(4100)), b"seg_metrics", b"aligned")


def test_eval_step_refusals(lib):
    thr = iou_logit_threshold()

    def call(x=P(1), t=P(2), n=2, k=1, hw=300, heads=1, kind=L.LOSS_BCE_DICE, w=P(3), wb=None, lo=P(4), m=P(5)):
        if wb is None:
            wb = lib.nunet_eval_step_ws_bytes(n, k, hw, heads, kind)
        return lib.nunet_eval_step(x, t, n, k, hw, heads, kind, w, wb, lo, m, thr, None)
    _refused(lib, call(k=0), b"eval_step", b"0 classes")
    _refused(lib, call(k=9), b"eval_step", b"9 classes")
    _refused(lib, call(hw=2 ** 24 + 1), b"eval_step", b"pixels")
    _refused(lib, call(heads=0), b"eval_step", b"0 heads")
    _refused(lib, call(heads=9), b"eval_step", b"9 heads")
    _refused(lib, call(kind=3), b"eval_step", b"loss_kind 3")
    _refused(lib, call(k=2, kind=L.LOSS_LOVASZ_HINGE), b"eval_step", b"Lovasz", b"one class")
    _refused(lib, call(hw=2 ** 22 + 1, kind=L.LOSS_LOVASZ_HINGE), b"eval_step", b"Lovasz", b"2^22")
    for kind in (L.LOSS_BCE_DICE, L.LOSS_LOVASZ_HINGE, L.LOSS_BCE_LOGITS):
        need = lib.nunet_eval_step_ws_bytes(2, 1, 300, 4, kind)
        _refused(lib, call(heads=4, kind=kind, wb=need - 1), b"eval_step", b"workspace", str(need).encode())
    for name in ("x", "t", "w", "lo", "m"):
        _refused(lib, call(**{name: None}), b"eval_step", b"null pointer")
    _refused(lib, call(w=C.c_void_p(4096 + 128)), b"eval_step", b"aligned")


def test_scores_from_counts():
    s = scores_from_counts([3, 0], [1, 0], [2, 0], [4, 10])
    assert s["iou"] == ([0.5, 1.0], 0.5) and s["dice"] == ([6 / 9, 1.0], 6 / 9)
    assert s["accuracy"] == ([0.7, 1.0], 17 / 20)
    assert s["sensitivity"][0][0] == 0.6 and math.isnan(s["sensitivity"][0][1]) and s["sensitivity"][1] == 0.6
    assert s["specificity"] == ([0.8, 1.0], 14 / 15)
    assert s["precision"][0][0] == 0.75 and math.isnan(s["precision"][0][1])
    assert list(s) == ["iou", "dice", "accuracy", "sensitivity", "specificity", "precision"]


def test_metric_docstrings_name_what_they_restate():
    m = nunet_amd.metrics
    assert "numeric_score" in m.seg_counts.__doc__ and "oracle" in m.seg_counts.__doc__
    assert "Acc" in m.pixel_accuracy.__doc__ and "oracle" in m.pixel_accuracy.__doc__
    assert "metrics.py:21-29" in m.dice_coef.__doc__


def test_train_py_help_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--eval_step" in r.stdout and "--val_metrics" in r.stdout
