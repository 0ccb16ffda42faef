"""Metrics of every head in one validation step: nunet_eval_step_heads, EvalStep(per_head=True), EvalStep(depth=L) and
val.py --depth / --per_head on the MI355X.

Everything here is an EQUALITY of bits: the head dimension of the segmentation sums keeps nunet_seg_metrics' partition of the
pixels over workgroups and its summation order per head, so head k's meters are those of a one-head nunet_eval_step on head
k's logits, and `loss_out` / `meters` are those of nunet_eval_step on all heads. nunet_eval_step itself is held to the fp64
restatement and the reference by tests/test_eval_gpu.py."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.metrics import iou_logit_threshold  # noqa: E402
from nunet_amd.trainer import EvalStep  # noqa: E402
import eval_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"BCEDiceLoss": L.LOSS_BCE_DICE, "LovaszHingeLoss": L.LOSS_LOVASZ_HINGE, "BCEWithLogitsLoss": L.LOSS_BCE_LOGITS}
MSZ = C.sizeof(L.EvalMeters)
CASES = [(3, 1, 257, "rand"), (3, 4, 300, "rand"), (2, 8, 300, "rand"), (3, 1, 16385, "edges")]


@pytest.fixture(autouse=True)
def _canaries(guard_bands):
    """every device buffer these tests allocate with a torch factory sits between guard bands checked after the test (conftest.py)"""
    yield


@pytest.fixture(scope="module")
def thr():
    return iou_logit_threshold()


def _batches(case, heads):
    """two batches of (logits [4, N, K, hw], target [N, K, hw]) on the device: the case's own tensor as the last head, the other
    heads deterministic variations of it that the metrics tell apart (a scaled and shifted copy; the negated tensor and a
    copy moved by one pixel, which keep the case's values around the sigmoid threshold); the second batch reverses the
    pixels and flips a third of the labels"""
    assert heads == 4
    x, t = EC.build(case)
    hs = torch.stack([x * 0.75 + 0.4, -x, x.roll(1, -1), x])
    t2 = torch.where(torch.arange(t.numel()).reshape(t.shape) % 3 == 0, 1.0 - t, t)
    return [(hs.to(DEV), t.to(DEV)), (hs.flip(-1).contiguous().to(DEV), t2.contiguous().to(DEV))]


def _eval_step(xd, td, case, heads, kind, thr, meters):
    lib = L.lib()
    n, k, hw, _ = case
    need = lib.nunet_eval_step_ws_bytes(n, k, hw, heads, kind)
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)
    loss_out = torch.full((heads + 1,), float("nan"), device=DEV)
    L.check(lib.nunet_eval_step(L.ptr(xd), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need, L.ptr(loss_out), L.ptr(meters), thr, L.stream()),
            "nunet_eval_step")
    return loss_out


def _bytes(t):
    return t.cpu().numpy().tobytes()


# each loss kind that admits the case's class count (the Lovasz hinge takes one class)
CASE_LOSSES = [(c, nm) for c in CASES for nm in KINDS if nm != "LovaszHingeLoss" or c[1] == 1]


@pytest.mark.parametrize("case,loss", CASE_LOSSES, ids=lambda v: EC.case_id(v) if isinstance(v, tuple) else v)
def test_eval_step_heads(case, loss, thr):
    """heads = 4 (and 1) over two consecutive batches on zeroed meters: loss_out and meters byte for byte those of
    nunet_eval_step, head_meters[k] byte for byte the meters of a one-head nunet_eval_step on head k's logits; the workspace is
    exactly the stated size, filled with NaN (no pre-zeroing is relied on); one byte less launches nothing."""
    n, k, hw, _ = case
    kind = KINDS[loss]
    lib = L.lib()
    for heads in (4, 1):
        meters = torch.zeros(MSZ, dtype=torch.uint8, device=DEV)
        head_meters = torch.zeros(heads * MSZ, dtype=torch.uint8, device=DEV)
        ref_meters = torch.zeros(MSZ, dtype=torch.uint8, device=DEV)
        ref_head = [torch.zeros(MSZ, dtype=torch.uint8, device=DEV) for _ in range(heads)]
        need = lib.nunet_eval_step_heads_ws_bytes(n, k, hw, heads, kind)
        assert need > 0 and need % 8 == 0
        for call, (xd, td) in enumerate(_batches(case, 4)):
            xd = xd[4 - heads:].contiguous()
            ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)
            loss_out = torch.full((heads + 1,), float("nan"), device=DEV)
            # one byte short: NUNET_EINVAL before the first launch, the outputs keep their bits
            snap = (_bytes(loss_out), _bytes(meters), _bytes(head_meters))
            rc = lib.nunet_eval_step_heads(L.ptr(xd), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need - 1, L.ptr(loss_out), L.ptr(meters),
                                           L.ptr(head_meters), thr, L.stream())
            assert rc == -1 and b"nunet_eval_step_heads_ws_bytes" in lib.nunet_last_error()
            torch.cuda.synchronize()
            assert snap == (_bytes(loss_out), _bytes(meters), _bytes(head_meters))
            assert bool(torch.isnan(ws).all())
            L.check(lib.nunet_eval_step_heads(L.ptr(xd), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need, L.ptr(loss_out), L.ptr(meters),
                                              L.ptr(head_meters), thr, L.stream()), "nunet_eval_step_heads")
            want_loss = _eval_step(xd, td, case, heads, kind, thr, ref_meters)
            one = [_eval_step(xd[j:j + 1].contiguous(), td, case, 1, kind, thr, ref_head[j]) for j in range(heads)]
            torch.cuda.synchronize()
            assert _bytes(loss_out) == _bytes(want_loss), (call, loss_out.tolist(), want_loss.tolist())
            assert _bytes(meters) == _bytes(ref_meters), call
            for j in range(heads):
                got = head_meters[j * MSZ:(j + 1) * MSZ]
                assert _bytes(got) == _bytes(ref_head[j]), (call, j)
                assert _bytes(one[j])[:4] == _bytes(loss_out)[4 * j:4 * j + 4]
        m = L.read_struct(meters, L.EvalMeters)
        hm = [L.read_struct(head_meters[j * MSZ:(j + 1) * MSZ], L.EvalMeters) for j in range(heads)]
        assert m.samples == 2 * n and all(h.samples == 2 * n for h in hm)
        assert all(math.isfinite(h.loss_sum) for h in hm)
        print("%s %s heads=%d: iou per head %s, of the step %.9g" % (EC.case_id(case), loss, heads, ["%.9g" % (h.iou_sum / h.samples) for h in hm],
                                                                     m.iou_sum / m.samples))
        # the last head is the one the step itself scores: equal in everything but the loss (the step's is the head mean)
        last = hm[-1]
        assert (last.iou_sum, last.dice_sum, last.acc_sum, list(last.tp), list(last.soft_i)) == (m.iou_sum, m.dice_sum, m.acc_sum, list(m.tp), list(m.soft_i))
        if heads == 1:
            assert _bytes(head_meters) == _bytes(meters)
        elif case[3] == "rand":
            assert len({h.iou_sum for h in hm}) > 1      # the heads are told apart


# ---------------------------------------------------------------------------------------------------------------------------
# EvalStep on the network
# ---------------------------------------------------------------------------------------------------------------------------
def _model(ncls, dtype):
    st = nunet_amd.synth.closed_form_state(ncls, 3, True, False)
    m = nunet_amd.archs.NestedUNet(ncls, 3, True, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    return m.to(DEV).eval()


HEAD_FIELDS = ("loss", "iou", "dice", "acc", "counts", "per_class")


def _same(a, b):
    """exact equality of two results or fields (repr round-trips a float; per_class may hold NaN for an empty class)"""
    return repr(a) == repr(b)


NET_SHAPE = (2, 3, 32, 32)      # 5 images in batches of 2: 2, 2 and an eager tail of 1


@functools.lru_cache(maxsize=None)
def _net(ncls, dtype):
    """-> (model, x, t, loss name, today's EvalStep result, the per_head step, its result): built once per (K, dtype) and
    shared between the tests below - do not write to them"""
    model = _model(ncls, dtype)
    img, msk = nunet_amd.synth.synth_split(5, 32, 32, 3, ncls, seed=2000)
    x, t = torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)
    loss = "BCEDiceLoss" if ncls == 1 else "BCEWithLogitsLoss"
    today = EvalStep(model, NET_SHAPE, loss=loss).evaluate(x, t)
    ph = EvalStep(model, NET_SHAPE, loss=loss, per_head=True)
    return model, x, t, loss, today, ph, ph.evaluate(x, t)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("ncls", [1, 4])
def test_eval_step_per_head(ncls, dtype):
    """per_head=True: the top-level fields are today's EvalStep's exactly, "heads" lists four dicts, a second pass repeats
    the first, and head 4 is the head the step itself scores (with its own loss, not the head mean)"""
    model, x, t, loss, today, ph, got = _net(ncls, dtype)
    assert ph.main.graph is not None and ph.tail.n == 1 and ph.heads == 4
    assert list(got)[:len(today)] == list(today) and list(got)[-1] == "heads" and len(got) == len(today) + 1
    for nm in today:
        assert _same(got[nm], today[nm]), (nm, got[nm], today[nm])
    assert len(got["heads"]) == 4 and all(tuple(h) == HEAD_FIELDS for h in got["heads"])
    assert _same(got, ph.evaluate(x, t))
    for nm in ("iou", "dice", "acc", "counts"):
        assert got["heads"][3][nm] == today[nm]
    assert len({h["loss"] for h in got["heads"]}) == 4


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("ncls", [1, 4])
def test_eval_step_depth(ncls, dtype, depth):
    """EvalStep(depth=L) reports exactly entry L - 1 of the per-head table; captured and eager agree exactly; last_logits are
    model(xb, depth=L) for the eager tail batch and for the captured static batch"""
    model, x, t, loss, _, _, got = _net(ncls, dtype)
    d = depth
    ev = EvalStep(model, NET_SHAPE, loss=loss, depth=d)
    r = ev.evaluate(x, t)
    assert ev.heads == 1 and ev.depth == d and ev.main.pl.depth == d and ev.tail.pl.depth == d and ev.main.graph is not None
    assert tuple(ev.logits.shape) == (1, 2, ncls, 32, 32)
    with torch.no_grad():
        assert torch.equal(ev.last_logits, model(x[4:5].contiguous(), depth=d))       # the tail batch ran last
    head = got["heads"][d - 1]
    print("K=%d %s depth %d: loss %.9g iou %.9g dice %.9g acc %.9g" % (ncls, dtype, d, r["loss"], r["iou"], r["dice"], r["acc"]))
    for nm in HEAD_FIELDS:
        assert _same(r[nm], head[nm]), (d, nm, r[nm], head[nm])
    assert r["samples"] == 5 and math.isfinite(r["loss"])
    eager = EvalStep(model, NET_SHAPE, loss=loss, depth=d, use_graph=False)
    assert _same(eager.evaluate(x, t), r) and eager.main.graph is None
    ev.begin()
    ev.step(x[:2], t[:2])
    with torch.no_grad():
        assert torch.equal(ev.last_logits, model(x[:2].contiguous(), depth=d))        # the captured static batch


def test_eval_step_argument_rules():
    model = _model(1, "fp32")
    shape = (2, 3, 32, 32)
    with pytest.raises(L.NunetError, match="per_head"):
        EvalStep(model, shape, depth=2, per_head=True)
    with pytest.raises(L.NunetError, match="depth"):
        EvalStep(model, shape, depth=5)
    plain = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).eval()
    with pytest.raises(L.NunetError, match="deep_supervision"):
        EvalStep(plain, shape, per_head=True)
    with pytest.raises(L.NunetError, match="deep_supervision"):
        EvalStep(plain, shape, depth=2)
    with pytest.raises(L.NunetError, match="UNet"):
        EvalStep(nunet_amd.archs.UNet(1, 3).to(DEV).eval(), shape, depth=2)
    assert "heads" not in EvalStep(model, shape, use_graph=False).evaluate(torch.zeros(2, 3, 32, 32, device=DEV), torch.zeros(2, 1, 32, 32, device=DEV))


def test_val_py_depth_and_per_head(tmp_path):
    """train.py --deep_supervision true for one epoch at 32 x 32 as a child process under a time limit, then val.py --depth 2
    --per_head true on its checkpoint: the IoU it prints for depth 2 is the head-2 line of the per-head table, one mask per
    validation image is written; on a checkpoint trained without deep supervision val.py --depth 2 exits non-zero with the
    error line."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "train.py"), "--epochs", "1", "--train_size", "8", "--val_size", "6", "--batch_size", "4",
            "--input_h", "32", "--input_w", "32"]
    r = subprocess.run(base + ["--deep_supervision", "true", "--name", "prune_e2e"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    v = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--name", "prune_e2e", "--depth", "2", "--per_head", "true"], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=600)
    assert v.returncode == 0, (v.stdout[-3000:], v.stderr[-3000:])
    lines = [ln for ln in v.stdout.strip().split("\n") if ln]
    print("\n".join(lines[-10:]))
    assert "depth: 2" in lines
    iou = [ln for ln in lines if ln.startswith("IoU: ")]
    assert len(iou) == 1
    table = [ln.split() for ln in lines[lines.index("depth: 2"):] if re.match(r"^\s*[1-4]\s", ln)]
    assert [row[0] for row in table] == ["1", "2", "3", "4"] and all(len(row) == 5 for row in table), table
    assert all(math.isfinite(float(v)) for row in table for v in row[1:])
    assert iou[0] == "IoU: " + table[1][1], (iou, table)
    masks = os.listdir(os.path.join(str(tmp_path), "outputs", "prune_e2e", "0"))
    assert sorted(masks) == ["val_%04d.jpg" % i for i in range(6)]
    # a checkpoint trained without deep supervision: one error line, non-zero status, before any GPU work
    r2 = subprocess.run(base + ["--name", "prune_e2e_plain"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, (r2.stdout[-3000:], r2.stderr[-3000:])
    for extra in (["--depth", "2"], ["--per_head", "true"]):
        v2 = subprocess.run([sys.executable, os.path.join(ROOT, "val.py"), "--name", "prune_e2e_plain"] + extra, cwd=str(tmp_path), env=env,
                            capture_output=True, text=True, timeout=600)
        assert v2.returncode != 0, v2.stdout[-2000:]
        errs = [ln for ln in v2.stdout.split("\n") if ln.startswith("error:")]
        assert len(errs) == 1 and "--deep_supervision true" in errs[0], v2.stdout[-2000:]
