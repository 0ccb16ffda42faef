"""The validation step on the MI355X: nunet_seg_metrics, nunet_eval_step, the new nunet_amd.metrics functions, EvalStep against
the module loop it replaces and against the reference's own validation numbers, and train.py --val_metrics end to end.

Cases, regimes and the fp64 restatement are those of tests/eval_cases.py (pinned against the reference on the CPU by
tests/test_eval_cpu.py). Bounds: integer counts, IoU and accuracy are EXACT; soft sums within 2e-6 |ref| (the bound
tests/test_bce_dice_gpu.py puts on the same fp32-sigmoid sums); batch dice within 4e-6 relative of fp64 (2e-6 on the
numerator, 2e-6 on the denominator) and within 4e-6 + 2^-24 of the reference's float32 value. Every figure is printed before
it is asserted."""
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
from nunet_amd.metrics import iou_logit_threshold  # noqa: E402
from nunet_amd.trainer import EvalStep  # noqa: E402
from nunet_amd.utils import AverageMeter  # noqa: E402
from conftest import load_golden  # noqa: E402
import eval_cases as EC  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOFT_REL = 2e-6
DICE_REL = 4e-6
DICE_REL_GOLDEN = 4e-6 + 2.0 ** -24
KINDS = {"BCEDiceLoss": L.LOSS_BCE_DICE, "LovaszHingeLoss": L.LOSS_LOVASZ_HINGE, "BCEWithLogitsLoss": L.LOSS_BCE_LOGITS}
COUNTS = ("tp", "fp", "fn", "tn")
SOFTS = ("soft_i", "soft_p", "soft_t")


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate with a torch factory - EvalStep's arenas and workspaces included - sits between
    guard bands that are checked after the test (conftest.py)"""
    yield


@pytest.fixture(scope="module")
def thr():
    return iou_logit_threshold()


@pytest.fixture(scope="module")
def golden():
    return load_golden("eval_metrics")


def _seg(xd, td, case, thr, poison, sums=None, accumulate=0):
    """nunet_seg_metrics on a workspace of exactly the stated size filled with `poison` -> the device sums buffer"""
    lib = L.lib()
    n, k, hw, _ = case
    need = lib.nunet_seg_metrics_ws_bytes(n, k, hw)
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8,), poison, dtype=torch.float64, device=DEV)
    if sums is None:
        sums = torch.full((C.sizeof(L.SegSums),), 0xEE, dtype=torch.uint8, device=DEV)
    L.check(lib.nunet_seg_metrics(L.ptr(xd), L.ptr(td), n, k, hw, thr, L.ptr(ws), need, L.ptr(sums), accumulate, L.stream()), "nunet_seg_metrics")
    torch.cuda.synchronize()
    return sums


def _check_soft(what, got, ref, pattern):
    for nm in SOFTS:
        for c, (g, r) in enumerate(zip(getattr(got, nm), ref[nm])):
            if math.isnan(r):
                assert math.isnan(g), (what, nm, c, g)
                continue
            rel = abs(g - r) / abs(r) if r else abs(g)
            if rel > 0.25 * SOFT_REL:
                print("%s: %s[%d] off by %.2e relative" % (what, nm, c, rel))
            assert abs(g - r) <= SOFT_REL * abs(r), (what, nm, c, g, r)
            if nm == "soft_t" and pattern != "soft":
                assert g == r, (what, "soft_t of hard labels is a sum of ones", c, g, r)


def _check_dice(what, dice, case, thr, golden):
    ref = EC.batch_values(EC.reference(case, thr), case[0] * case[1] * case[2])[1]
    gold = float(golden["dice_" + EC.case_id(case)])
    if math.isnan(ref):
        assert math.isnan(dice)
        return
    print("%s: dice %.9g, (dice - fp64) / fp64 = %.2e, (dice - reference) / reference = %.2e" % (what, dice, (dice - ref) / ref, (dice - gold) / gold))
    assert abs(dice - ref) <= DICE_REL * abs(ref)
    assert abs(dice - gold) <= DICE_REL_GOLDEN * abs(gold)


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_seg_metrics(case, thr, golden):
    """Every launch regime of the table and the five patterns on 3 x 1 x 16385: counts exact per class, their sums equal to
    nunet_iou_counts' intersection and union, soft sums within 2e-6 |ref| (soft_t exact for hard labels; NaN logits leave NaN
    sums and exact counts), the classes >= K zeroed, accumulate = 1 adds, and a second run on a differently poisoned
    workspace is bit-identical (no partial is read that no block wrote)."""
    n, k, hw, pattern = case
    lib = L.lib()
    if pattern == "rand":
        info = L.LossLaunchInfo()
        L.check(lib.nunet_seg_metrics_launch_info(n, k, hw, C.byref(info)), "nunet_seg_metrics_launch_info")
        assert (info.grid_x, info.trips_max, info.trips_min) == EC.SHAPES[(n, k, hw)]
    x, t = EC.build(case)
    xd, td = x.to(DEV), t.to(DEV)
    ref = EC.reference(case, thr)
    sums = _seg(xd, td, case, thr, float("nan"))
    got = L.read_struct(sums, L.SegSums)
    what = EC.case_id(case)
    for nm in COUNTS:
        assert list(getattr(got, nm))[:k] == ref[nm], (what, nm)
    for nm in COUNTS + SOFTS:
        assert all(v == 0 for v in list(getattr(got, nm))[k:]), (what, nm, "classes >= K")
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    L.check(lib.nunet_iou_counts(L.ptr(xd), L.ptr(td), xd.numel(), thr, L.ptr(counts), L.stream()), "nunet_iou_counts")
    inter, union = counts.tolist()
    assert (sum(got.tp), sum(got.tp) + sum(got.fp) + sum(got.fn)) == (inter, union)
    assert sum(sum(getattr(got, nm)) for nm in COUNTS) == n * k * hw
    _check_soft(what, got, ref, pattern)
    iou, dice, acc = EC.batch_values({nm: list(getattr(got, nm)) for nm in COUNTS + SOFTS}, n * k * hw)
    assert iou == float(golden["iou_" + what])
    if pattern == "all_background":
        assert iou == 1.0
    _check_dice(what, dice, case, thr, golden)
    # accumulate
    twice = L.read_struct(_seg(xd, td, case, thr, 1e300, sums.clone(), 1), L.SegSums)
    for nm in COUNTS:
        assert list(getattr(twice, nm)) == [2 * v for v in getattr(got, nm)]
    for nm in SOFTS:
        for a, b in zip(getattr(twice, nm)[:k], getattr(got, nm)[:k]):
            assert a == b + b or (math.isnan(a) and math.isnan(b))
    # another poison
    again = _seg(xd, td, case, thr, 1e300)
    assert torch.equal(again, sums)


@pytest.mark.parametrize("case", [(2, 1, 1, "rand"), (33, 8, 300, "rand")], ids=EC.case_id)
def test_seg_metrics_writes_one_slab(case, thr):
    """nunet_seg_metrics launches the one-slab form of the kernel that nunet_eval_step_heads runs with up to four slabs: on a
    workspace of exactly nunet_seg_metrics_ws_bytes between two NaN bands of a slab's size and more (what a second slab would
    overwrite), the bands keep every bit and the sums equal the restatement."""
    lib = L.lib()
    n, k, hw, pattern = case
    need = lib.nunet_seg_metrics_ws_bytes(n, k, hw)
    assert need > 0 and need % 8 == 0
    band = need // 8 + 512
    buf = torch.full((2 * band + need // 8,), float("nan"), dtype=torch.float64, device=DEV)
    before = buf.view(torch.int64).clone()
    x, t = EC.build(case)
    xd, td = x.to(DEV), t.to(DEV)
    sums = torch.full((C.sizeof(L.SegSums),), 0xEE, dtype=torch.uint8, device=DEV)
    L.check(lib.nunet_seg_metrics(L.ptr(xd), L.ptr(td), n, k, hw, thr, L.ptr(buf, 8 * band), need, L.ptr(sums), 0, L.stream()), "nunet_seg_metrics")
    torch.cuda.synchronize()
    after = buf.view(torch.int64)
    assert torch.equal(after[:band], before[:band]), "write before the workspace"
    assert torch.equal(after[band + need // 8:], before[band + need // 8:]), "write past the workspace"
    got, ref = L.read_struct(sums, L.SegSums), EC.reference(case, thr)
    for nm in COUNTS:
        assert list(getattr(got, nm))[:k] == ref[nm], nm
    for nm in COUNTS + SOFTS:
        assert all(v == 0 for v in list(getattr(got, nm))[k:]), (nm, "classes >= K")
    _check_soft(EC.case_id(case), got, ref, pattern)


def _heads_of(case, heads):
    """logits [heads, N, K, hw]: the last head is the case's own tensor, the others are deterministic variations of it"""
    x, t = EC.build(case)
    return torch.stack([x * (0.5 + 0.25 * j) + 0.1 * (heads - 1 - j) for j in range(heads - 1)] + [x]), t


def _standalone_loss(xd, td, n, k, hw, kind):
    """head loss by the stand-alone entry the matching losses.* module calls -> fp32 [1] on the device"""
    lib = L.lib()
    loss = torch.full((1,), float("nan"), device=DEV)
    if kind == L.LOSS_BCE_DICE:
        ws = torch.empty((lib.nunet_bce_dice_ws_bytes(n) + 3) // 4, device=DEV)
        L.check(lib.nunet_bce_dice_fwd(L.ptr(xd), L.ptr(td), n, k * hw, L.ptr(ws), L.nbytes(ws), L.ptr(loss), L.stream()), "bce_dice_fwd")
    elif kind == L.LOSS_BCE_LOGITS:
        ws = torch.empty((lib.nunet_bce_logits_ws_bytes(n * k * hw) + 3) // 4, device=DEV)
        L.check(lib.nunet_bce_logits_fwd(L.ptr(xd), L.ptr(td), n * k * hw, L.ptr(ws), L.nbytes(ws), L.ptr(loss), L.stream()), "bce_logits_fwd")
    else:
        ws = torch.empty(lib.nunet_lovasz_ws_bytes(n, hw), dtype=torch.uint8, device=DEV)
        unit = torch.empty(n * hw, device=DEV)
        L.check(lib.nunet_lovasz_hinge_fwd(L.ptr(xd), L.ptr(td), n, hw, L.ptr(ws), L.nbytes(ws), L.ptr(unit), L.ptr(loss), L.stream()), "lovasz_hinge_fwd")
    return loss


SEQUENCES = {"k1": [(3, 1, 257, "rand"), (2, 1, 16385, "rand"), (3, 1, 16385, "edges")], "k4": [(3, 4, 300, "rand"), (3, 4, 300, "rand"), (3, 4, 300, "rand")]}


@pytest.mark.parametrize("heads", [1, 4, 8])    # (8: above nunet_eval_step_heads' limit, the last-head form alone reaches it)
@pytest.mark.parametrize("loss,seq", [("BCEDiceLoss", "k1"), ("BCEDiceLoss", "k4"), ("BCEWithLogitsLoss", "k1"), ("BCEWithLogitsLoss", "k4"),
                                      ("LovaszHingeLoss", "k1")])
def test_eval_step(heads, loss, seq, thr, golden):
    """Three calls on one zeroed meters struct (batches of 3, 2 and 3 images for one class): every head's loss has the bits of
    the stand-alone entry, the mean is the fp32 left-to-right sum divided once by heads, the batch IoU and accuracy equal the
    restatement, the batch dice is within 4e-6 of fp64 and 4e-6 + 2^-24 of the reference's value, and after the third call the
    meters are the double-precision AverageMeter of the batch values (1e-12) and the sums of the counts."""
    lib, kind = L.lib(), KINDS[loss]
    meters = torch.zeros(C.sizeof(L.EvalMeters), dtype=torch.uint8, device=DEV)
    avg = {nm: EC.Meter() for nm in ("loss", "iou", "dice", "acc")}
    tot = {nm: [0] * 8 for nm in COUNTS}
    for call, case in enumerate(SEQUENCES[seq]):
        n, k, hw, _ = case
        x, t = _heads_of(case, heads)
        xd, td = x.to(DEV), t.to(DEV)
        need = lib.nunet_eval_step_ws_bytes(n, k, hw, heads, kind)
        assert need > 0 and need % 8 == 0
        ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)
        loss_out = torch.full((heads + 1,), float("nan"), device=DEV)
        L.check(lib.nunet_eval_step(L.ptr(xd), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need, L.ptr(loss_out), L.ptr(meters), thr, L.stream()),
                "nunet_eval_step")
        alone = torch.cat([_standalone_loss(xd[j], td, n, k, hw, kind) for j in range(heads)])
        torch.cuda.synchronize()
        assert torch.equal(loss_out[:heads].view(torch.int32), alone.view(torch.int32)), (loss_out.tolist(), alone.tolist())
        lo = loss_out.cpu().numpy()
        mean = np.float32(lo[0])
        for j in range(1, heads):
            mean = np.float32(mean + lo[j])
        mean = np.float32(mean / np.float32(heads))
        assert lo[heads] == mean and math.isfinite(float(mean)), (lo, mean)
        m = L.read_struct(meters, L.EvalMeters)
        ref = EC.reference(case, thr)
        iou, dice, acc = EC.batch_values(ref, n * k * hw)
        assert (m.last_iou, m.last_acc) == (iou, acc)
        _check_dice("%s h%d call %d" % (loss, heads, call), m.last_dice, case, thr, golden)
        for nm, v in (("loss", float(lo[heads])), ("iou", m.last_iou), ("dice", m.last_dice), ("acc", m.last_acc)):
            avg[nm].update(v, n)
        for nm in COUNTS:
            tot[nm] = [a + b for a, b in zip(tot[nm], ref[nm] + [0] * (8 - k))]
    m = L.read_struct(meters, L.EvalMeters)
    assert m.samples == avg["loss"].count == sum(c[0] for c in SEQUENCES[seq])
    for nm, got in (("loss", m.loss_sum), ("iou", m.iou_sum), ("dice", m.dice_sum), ("acc", m.acc_sum)):
        assert abs(got - avg[nm].sum) <= 1e-12 * abs(avg[nm].sum), (nm, got, avg[nm].sum)
    for nm in COUNTS:
        assert list(getattr(m, nm)) == tot[nm]


@pytest.mark.parametrize("case", [(3, 1, 257, "rand"), (3, 4, 300, "rand"), (2, 8, 300, "rand"), (3, 1, 16385, "edges"), (3, 1, 16385, "soft")], ids=EC.case_id)
def test_metrics_module(case, thr, golden):
    """nunet_amd.metrics.dice_coef / seg_counts / pixel_accuracy on [N, K, H, W] tensors: dice against the reference's value
    and the restatement, counts and accuracy exact, seg_counts accumulating into the buffer handed back."""
    M = nunet_amd.metrics
    n, k, hw, _ = case
    x, t = EC.build(case)
    xd, td = x.reshape(n, k, hw, 1).to(DEV), t.reshape(n, k, hw, 1).to(DEV)
    ref = EC.reference(case, thr)
    d = M.dice_coef(xd, td)
    assert isinstance(d, float)
    _check_dice("dice_coef " + EC.case_id(case), d, case, thr, golden)
    c = M.seg_counts(xd, td)
    assert [q.tolist() for q in c] == [ref[nm] for nm in COUNTS]
    c2 = M.seg_counts(xd, td, c.sums)
    assert [q.tolist() for q in c2] == [[2 * v for v in ref[nm]] for nm in COUNTS]
    acc = M.pixel_accuracy(xd, td)
    assert acc == EC.batch_values(ref, n * k * hw)[2]
    assert M.iou_score(xd, td) == float(golden["iou_" + EC.case_id(case)])
    s = M.scores_from_counts(*[ref[nm] for nm in COUNTS])
    assert s["accuracy"][1] == acc


# ---------------------------------------------------------------------------------------------------------------------------
# EvalStep
# ---------------------------------------------------------------------------------------------------------------------------
def _model(synth, ncls, ds, dtype):
    st = synth.closed_form_state(ncls, 3, ds, False)
    m = nunet_amd.archs.NestedUNet(ncls, 3, ds, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV)


def _split(synth, ncls):
    n, h, w, cin, seed = EC.NET_SPLIT
    img, msk = synth.synth_split(n, h, w, cin, ncls, seed=seed)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)


def _module_loop(model, x, t, loss, ds, thr):
    """the validation loop this project ran before EvalStep (train.py validate(): reference trains.py:150-188 through the module
    and the stand-alone loss and IoU entries) -> (loss, iou) as it returned them, (dice, acc) by the restatement on its logits"""
    crit = getattr(nunet_amd.losses, loss)()
    avg = {nm: AverageMeter() for nm in ("loss", "iou", "dice", "acc")}
    model.eval()
    with torch.no_grad():
        for k in range(0, x.size(0), EC.NET_BATCH):
            xb, tb = x[k:k + EC.NET_BATCH].contiguous(), t[k:k + EC.NET_BATCH].contiguous()
            out = model(xb)
            if ds:
                lv = sum(crit(o, tb) for o in out) / len(out)
                last = out[-1]
            else:
                lv = crit(out, tb)
                last = out
            avg["loss"].update(lv.item(), xb.size(0))
            avg["iou"].update(nunet_amd.metrics.iou_from_counts(nunet_amd.metrics.iou_counts(last.contiguous(), tb)), xb.size(0))
            _, dice, acc = EC.batch_values(EC.restate(last.cpu(), tb.cpu(), thr), last.numel())
            avg["dice"].update(dice, xb.size(0))
            avg["acc"].update(acc, xb.size(0))
    return {nm: avg[nm].avg for nm in avg}


def _same(a, b):
    return all(a[nm] == b[nm] for nm in ("loss", "iou", "dice", "acc")) and a["counts"] == b["counts"]


@pytest.mark.parametrize("ncls,ds,loss,dtype", [(1, False, "BCEDiceLoss", "fp32"), (4, True, "BCEWithLogitsLoss", "fp32"),
                                                (1, True, "LovaszHingeLoss", "fp32"), (1, False, "BCEDiceLoss", "bf16")],
                         ids=["fp32-k1", "fp32-k4-ds-bcelogits", "fp32-k1-ds-lovasz", "bf16-k1"])
def test_eval_step_against_the_module_loop(ncls, ds, loss, dtype, synth, thr):
    """EvalStep.evaluate over 10 images in batches of 4 (4, 4 and an eager tail of 2): loss and iou are BIT-EQUAL to the module
    loop's, acc equals the restatement on the module path's logits and dice is within 4e-6 of it; the captured and the eager
    form agree in every bit, a second pass repeats the first, and after an in-place change of a parameter the next pass
    follows it (the repack) - again to the module loop's bits."""
    model = _model(synth, ncls, ds, dtype)
    x, t = _split(synth, ncls)
    shape = (EC.NET_BATCH, 3) + tuple(x.shape[2:])
    for trial in range(2):
        want = _module_loop(model, x, t, loss, ds, thr)
        if trial == 0:
            ev = EvalStep(model, shape, loss=loss)
            eager = EvalStep(model, shape, loss=loss, use_graph=False)
        got = ev.evaluate(x, t)
        assert ev.main.graph is not None and eager.main.graph is None and ev.tail.n == 2 and ev.tail.graph is None
        print("%s %s trial %d: loss %.9g iou %.9g dice %.9g acc %.9g; (dice - restated) / restated = %.2e"
              % (loss, dtype, trial, got["loss"], got["iou"], got["dice"], got["acc"], (got["dice"] - want["dice"]) / want["dice"]))
        assert got["loss"] == want["loss"] and got["iou"] == want["iou"], (got, want)
        assert got["acc"] == want["acc"]
        assert abs(got["dice"] - want["dice"]) <= DICE_REL * abs(want["dice"])
        assert got["samples"] == 10 and math.isfinite(got["loss"])
        assert sum(sum(got["counts"][nm]) for nm in COUNTS) == 10 * ncls * 32 * 32
        assert _same(eager.evaluate(x, t), got)
        assert _same(ev.evaluate(x, t), got)
        assert tuple(ev.logits.shape) == (4 if ds else 1, 4, ncls, 32, 32) and tuple(ev.last_logits.shape) == (2, ncls, 32, 32)
        if trial == 0:
            first = got
            with torch.no_grad():
                (model.final4 if ds else model.final).weight.mul_(-0.75)
                model.conv0_0.conv1.weight.mul_(1.25)
    assert got["loss"] != first["loss"] and got["counts"] != first["counts"]


def test_eval_step_refuses_a_rehomed_engine(synth):
    model = _model(synth, 1, False, "fp32")
    x, t = _split(synth, 1)
    ev = EvalStep(model, (4, 3, 32, 32), use_graph=False)
    ev.evaluate(x, t)
    model.cpu().to(DEV)          # the parameters leave the engine's arenas
    with pytest.raises(L.NunetError, match="re-homed"):
        ev.evaluate(x, t)
    with pytest.raises(L.NunetError, match="num_classes must be 1"):
        EvalStep(_model(synth, 4, False, "fp32"), (4, 3, 32, 32), loss="LovaszHingeLoss")


@pytest.mark.parametrize("tag,loss", [("k1", "BCEDiceLoss"), ("k4ds", "BCEWithLogitsLoss")])
def test_eval_step_against_the_reference_network(tag, loss, synth, golden):
    """fp32 EvalStep against the reference NestedUNet's own validation pass (tests/golden/make_golden_eval.py: eval mode,
    closed-form weights and running statistics, 10 images in batches of 4, 4, 2), with the bands tests/test_bce_logits_gpu.py
    holds the evaluation forward to: loss within 1e-4, IoU and accuracy within 5e-3, dice within 1e-4 (logits are held to 1e-4
    and the sigmoid is 1/4-Lipschitz).

    Measured on an MI355X, |value - golden| for loss, iou, dice, acc:
        k1   (BCEDiceLoss)                   3.8e-07, 0, 9.0e-09, 0
        k4ds (BCEWithLogitsLoss, 4 heads)    7.6e-07, 8.3e-06, 6.1e-08, 2.4e-05"""
    ncls, ds = EC.NET[tag]
    model = _model(synth, ncls, ds, "fp32")
    x, t = _split(synth, ncls)
    got = EvalStep(model, (EC.NET_BATCH, 3, 32, 32), loss=loss).evaluate(x, t)
    key = {"BCEDiceLoss": "bcedice", "BCEWithLogitsLoss": "bcelogits"}[loss]
    dev = {nm: abs(got[nm] - float(golden["%s_%s" % (key if nm == "loss" else nm, tag)])) for nm in ("loss", "iou", "dice", "acc")}
    print("%s: loss %.9g (golden %.9g); |value - golden|: loss %.2e, iou %.2e, dice %.2e, acc %.2e"
          % (tag, got["loss"], float(golden["%s_%s" % (key, tag)]), dev["loss"], dev["iou"], dev["dice"], dev["acc"]))
    assert dev["loss"] < 1e-4 and dev["iou"] < 5e-3 and dev["acc"] < 5e-3 and dev["dice"] < 1e-4, dev


def test_train_py_val_metrics(tmp_path):
    """train.py --val_metrics true for one epoch at 32 x 32, as a child process under a time limit: validation goes through the
    captured EvalStep, log.csv's header ends in val_dice,val_acc and the values are finite fractions; then val.py on the saved
    checkpoint prints the same IoU, a Dice and an Acc line and writes one mask per image."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--val_metrics", "true", "--epochs", "1", "--train_size", "32", "--val_size", "20",
           "--input_h", "32", "--input_w", "32", "-b", "8", "--name", "evalstep_e2e"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "captured validation step (EvalStep)" in r.stdout
    rows = open(os.path.join(str(tmp_path), "models", "evalstep_e2e", "log.csv")).read().strip().split("\n")
    assert rows[0] == "epoch,lr,loss,iou,val_loss,val_iou,images_per_sec,val_dice,val_acc" and len(rows) == 2
    rec = dict(zip(rows[0].split(","), rows[1].split(",")))
    for nm in ("val_loss", "val_iou", "val_dice", "val_acc"):
        assert math.isfinite(float(rec[nm])), rec
    assert 0.0 <= float(rec["val_dice"]) <= 1.0 and 0.0 <= float(rec["val_acc"]) <= 1.0
    # val.py on the checkpoint that run saved: the same step, the IoU line as before, the Dice and Acc lines behind it
    assert os.path.exists(os.path.join(str(tmp_path), "models", "evalstep_e2e", "model.pth")), r.stdout[-2000:]
    v = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--name", "evalstep_e2e"], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=600)
    assert v.returncode == 0, (v.stdout[-3000:], v.stderr[-3000:])
    tail = [ln for ln in v.stdout.strip().split("\n") if ln][-3:]
    assert [ln.split(":")[0] for ln in tail] == ["IoU", "Dice", "Acc"], tail
    assert tail[0] == "IoU: %.4f" % float(rec["val_iou"]), (tail, rec)       # the weights of the only epoch: the pass train.py ran
    assert all(math.isfinite(float(ln.split(":")[1])) for ln in tail)
    assert len(os.listdir(os.path.join(str(tmp_path), "outputs", "evalstep_e2e", "0"))) == 20
