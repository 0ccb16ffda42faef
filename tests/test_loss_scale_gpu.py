"""Dynamic loss scaling inside the fused step on the MI355X (TrainStep(loss_scale=...)): fp16 gradient fidelity against the fp32
path, scale 1 as the identity, a power-of-two scale in fp32, overflow / skip / backoff against torch.amp.GradScaler on the eager
path, growth across graph replays, the state round trip, and train.py --loss_scale dynamic end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import loss_scale as LS  # noqa: E402
from nunet_amd.trainer import TrainStep  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor, chosen without timing


def _module(st, ncls=1, dtype="fp32"):
    m = nunet_amd.archs.NestedUNet(ncls, 3, False, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.clone() for k, v in st.items()})
    return m.to(DEV).train()


def _batches(synth, n, hw, ncls, seeds):
    out = []
    for s in seeds:
        img, msk = synth.synth_batch(n, hw, hw, 3, ncls, seed=s)
        out.append((torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)))
    return out


def _grads(ts, model):
    return {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters()}


def _bn_fed_bias(name):
    """conv biases that feed a BatchNorm: their gradient is analytically zero"""
    return name.endswith(("conv1.bias", "conv2.bias"))


def _state(ts):
    eng = ts.eng
    out = [eng.flat_params, eng.bnbuf, eng.nbt, ts.meters, eng.flat_grads] + ts.opt_state
    return [t.detach().clone() for t in out]


@pytest.mark.parametrize("n,hw,ncls", [(4, 256, 1), (2, 512, 4)])
def test_fp16_gradient_fidelity(synth, n, hw, ncls):
    """fp16 storage keeps activation gradients in fp16; without scaling most of them are subnormal or zero at these
    geometries. Step-0 p.grad of an fp16 TrainStep with and without loss_scale="dynamic" against the fp32 path's from the same
    state and batch (lr = 0, so every step sees the same parameters; conv biases feeding a BatchNorm left out): the median
    per-tensor rel-L2 must be <= 0.15 with scaling (the issue's bound was 0.2) and at most half of the unscaled figure.
    Measured on the MI355X (median / p90; step 0 was not skipped at either geometry):
      256x256 bs4, 1 class:    scaled 0.093 / 0.16, unscaled 0.32 / 1.21
      512x512 bs2, 4 classes:  scaled 0.090 / 0.16, unscaled 1.40 / 5.63"""
    st = synth.closed_form_state(ncls, 3, False, True)
    (x, t), = _batches(synth, n, hw, ncls, [77])
    ref_m = _module(st, ncls, "fp32")
    ref = TrainStep(ref_m, (n, 3, hw, hw), lr=0.0, use_graph=False)
    ref.step(x, t)
    print("executor_choice", ref.executor_choice)
    g32 = _grads(ref, ref_m)
    del ref, ref_m
    med = {}
    for scaled in (False, True):
        m = _module(st, ncls, "fp16")
        ts = TrainStep(m, (n, 3, hw, hw), lr=0.0, use_graph=False, loss_scale="dynamic" if scaled else None)
        print("executor_choice", ts.executor_choice)
        used = 0
        for k in range(6):
            ts.step(x, t)
            if not scaled or ts.scaler_stats()[1] == 0:
                break
            ts.reset_meters()
            used = k + 1
        assert not scaled or ts.scaler_stats()[1] == 0, "every step overflowed"
        g = _grads(ts, m)
        rel = [float((g[k] - g32[k]).norm() / g32[k].norm()) for k in g32 if not _bn_fed_bias(k) and float(g32[k].norm()) > 0]
        med[scaled] = float(np.median(rel))
        print("%dx%d bs%d %d classes: scaled=%s step %d median rel-L2 %.4f p90 %.4f" % (hw, hw, n, ncls, scaled, used, med[scaled],
                                                                                   float(np.percentile(rel, 90))))
        del ts, m
        torch.cuda.empty_cache()
    assert med[True] <= 0.15, med
    assert med[True] <= 0.5 * med[False], med


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
@pytest.mark.parametrize("fused_update", [0, 2])
def test_scale_one_is_the_identity(synth, dtype, optimizer, fused_update):
    """loss_scale=dict(init_scale=1, growth_interval=1e9): after 3 graph steps parameters, gradients, optimiser state, BN buffers
    and meters are bit-identical to loss_scale=None."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [11, 12, 13])
    res = []
    for ls in (None, dict(init_scale=1.0, growth_interval=10 ** 9)):
        m = _module(st, 1, dtype)
        ts = TrainStep(m, (4, 3, 64, 64), lr=1e-2, optimizer=optimizer, fused_update=fused_update, loss_scale=ls, **GRAPH)
        ts.capture(*data[0])
        print("executor_choice", ts.executor_choice)
        for x, t in data:
            ts.step(x, t)
        torch.cuda.synchronize()
        res.append(_state(ts))
        if ls is not None:
            assert ts.scaler_stats() == (1.0, 0)
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), k


def test_power_of_two_scale_fp32(synth):
    """fp32, init_scale 1024: parameters after 3 steps within 1e-6 relative of the unscaled run (not bit-identical: the
    fixed-point BatchNorm sums are not scale-equivariant in their lowest bits)."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [21, 22, 23])
    res = []
    for ls in (None, dict(init_scale=1024.0)):
        m = _module(st)
        ts = TrainStep(m, (4, 3, 64, 64), lr=1e-2, loss_scale=ls, **GRAPH)
        ts.capture(*data[0])
        print("executor_choice", ts.executor_choice)
        for x, t in data:
            ts.step(x, t)
        torch.cuda.synchronize()
        res.append({k: p.detach().double().cpu() for k, p in m.named_parameters()})
    worst = max(float((res[1][k] - res[0][k]).norm() / res[0][k].norm()) for k in res[0] if float(res[0][k].norm()) > 0)
    assert worst <= 1e-6, worst


def _eager_grad_scaler(st, data, steps, init_scale, lr, momentum, wd):
    """torch.amp.GradScaler("cuda") + torch.optim.SGD driving the eager path (same model, state and batches): (scale, skipped)."""
    m = _module(st, 1, "fp16")
    crit = nunet_amd.losses.BCEDiceLoss()
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    skipped = 0
    for k in range(steps):
        x, t = data[k % len(data)]
        opt.zero_grad()
        scaler.scale(crit(m(x), t)).backward()
        scaler.step(opt)
        s0 = scaler.get_scale()
        scaler.update()
        skipped += int(scaler.get_scale() < s0)
    return scaler.get_scale(), skipped


@pytest.mark.parametrize("executor", [dict(segmented=False, schedule="lanes"), dict(segmented="flags", schedule="list")])
@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
def test_overflow_skips_and_backs_off(synth, executor, optimizer):
    """fp16, init_scale 2^40: every stored gradient overflows at first. A skipped step leaves parameters, momentum / Adam moments
    and Adam's t bit-unchanged and halves the scale; steps resume once the scale has backed off. The per-step skip flags, fed to
    the host rule, reproduce every reported scale; SGD's final scale and skip count equal torch.amp.GradScaler's on the eager
    path."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [31])
    init, steps = 2.0 ** 40, 30
    m = _module(st, 1, "fp16")
    ts = TrainStep(m, (4, 3, 64, 64), lr=1e-2, momentum=0.9, weight_decay=1e-4, optimizer=optimizer, loss_scale=dict(init_scale=init),
                   **executor)
    ts.capture(*data[0])
    print("executor_choice", ts.executor_choice, executor)
    cfg = ts.scaler_cfg
    scale, tracker, skipped, clean = init, 0, 0, 0
    for k in range(steps):
        before = [t.clone() for t in [ts.eng.flat_params] + ts.opt_state]
        ts.step(*data[k % len(data)])
        s_dev, sk = ts.scaler_stats()
        found = sk - skipped
        assert found in (0, 1)
        skipped = sk
        scale, tracker = LS.update_scale(scale, tracker, found, cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"])
        assert s_dev == scale, (k, s_dev, scale)
        after = [ts.eng.flat_params] + ts.opt_state
        if found:
            assert all(torch.equal(a, b) for a, b in zip(before, after)), k
        else:
            assert not torch.equal(before[0], after[0]), k
            clean += 1
    print("final scale %g, %d skipped, %d clean" % (scale, skipped, clean))
    assert skipped >= 5 and clean >= 5
    if optimizer == "Adam":
        assert float(ts.adam_step) == clean
        assert torch.isfinite(ts.exp_avg).all() and torch.isfinite(ts.exp_avg_sq).all()
    else:
        assert _eager_grad_scaler(st, data, steps, init, 1e-2, 0.9, 1e-4) == (scale, skipped)


def test_growth_across_replays(synth):
    """fp32, growth_interval 2: the scale doubles every 2 steps of the SAME captured graph."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 2, 32, 1, [41, 42])
    m = _module(st)
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-3, loss_scale=dict(init_scale=1.0, growth_interval=2), **GRAPH)
    ts.capture(*data[0])
    print("executor_choice", ts.executor_choice)
    g = ts.g_fb
    seen = []
    for k in range(8):
        ts.step(*data[k % 2])
        seen.append(ts.scaler_stats())
    assert ts.g_fb is g
    assert seen == [(2.0 ** ((k + 1) // 2), 0) for k in range(8)], seen
    assert ts.scaler_state_dict()["_growth_tracker"] == 0


def test_state_round_trip(synth):
    """scaler_state_dict() + optimizer_state_dict() (+ the module's state) saved mid-run and loaded into a fresh TrainStep: the
    continuation is bit-identical."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [51, 52, 53])
    ls = dict(init_scale=2.0 ** 24, growth_interval=3)
    m = _module(st, 1, "fp16")
    a = TrainStep(m, (4, 3, 64, 64), lr=1e-2, optimizer="Adam", loss_scale=ls, **GRAPH)
    a.capture(*data[0])
    print("executor_choice", a.executor_choice)
    for k in range(4):
        a.step(*data[k % 3])
    sd_s, sd_o = a.scaler_state_dict(), a.optimizer_state_dict()
    sd_m = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    print("saved", sd_s)
    for k in range(4):
        a.step(*data[k % 3])
    torch.cuda.synchronize()
    want = (m.state_dict(), a.scaler_state_dict())
    m2 = _module(sd_m, 1, "fp16")
    b = TrainStep(m2, (4, 3, 64, 64), lr=1e-2, optimizer="Adam", loss_scale="dynamic", **GRAPH)
    b.load_optimizer_state_dict(sd_o)
    b.load_scaler_state_dict(sd_s)
    assert b.scaler_state_dict() == sd_s
    b.capture(*data[0])
    for k in range(4):
        b.step(*data[k % 3])
    torch.cuda.synchronize()
    got = (m2.state_dict(), b.scaler_state_dict())
    assert got[1] == want[1]
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k


def test_train_py_loss_scale(tmp_path):
    """train.py --dtype fp16 --loss_scale dynamic for 2 epochs: the fused step, the usual artefacts, the scale on the epoch line."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--dtype", "fp16", "--loss_scale", "dynamic", "--epochs", "2",
           "--train_size", "64", "--val_size", "32", "--input_h", "32", "--input_w", "32", "-b", "8", "--name", "amp_e2e"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dynamic loss scaling" in r.stdout and r.stdout.count("loss scale ") == 2, r.stdout[-2000:]
    rows = open(tmp_path / "models" / "amp_e2e" / "log.csv").read().strip().splitlines()
    assert rows[0].split(",") == ["epoch", "lr", "loss", "iou", "val_loss", "val_iou", "images_per_sec"]
    assert len(rows) == 3
    last = dict(zip(rows[0].split(","), rows[-1].split(",")))
    assert np.isfinite(float(last["val_iou"])) and np.isfinite(float(last["loss"]))
    assert os.path.exists(tmp_path / "models" / "amp_e2e" / "config.yml")
