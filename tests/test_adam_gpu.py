"""The fused Adam step on the MI355X (TrainStep(optimizer='Adam'), reference trains.py:73-76,225-227): the flat kernel against
torch.optim.Adam, the fused layouts against each other, graph against eager, the whole step against the CPU oracle and the
reference's Adam trajectory, the torch.optim state-dict round trip, and train.py --optimizer Adam end to end."""
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
from oracle import nunet_oracle as O  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


def _module(st, ds=False, dtype="fp32"):
    m = nunet_amd.archs.NestedUNet(1, 3, ds, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.clone() for k, v in st.items()})
    return m.to(DEV).train()


def _batch(synth, n, hw, seed):
    img, msk = synth.synth_batch(n, hw, hw, 3, 1, seed=seed)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_flat_adam_step_matches_torch_adam(wd, guard_bands):
    """nunet_adam_step (+ nunet_adam_prepare) against torch.optim.Adam(foreach=False) on the device over 10 steps fed identical
    gradients: n % 4 = 3 (vector body + scalar tail), grad_scale 0.5, a block of exactly-zero gradients. Bound: 8 ulp relative
    per element (plus a floor of 1e-6 of the tensor's largest magnitude for values that cancel towards zero). Each of the ten
    steps may round its last operations differently from torch's kernels - fused multiply-adds, torch's reciprocal-multiply
    for the bias correction, the scalars' single rounding - so a difference of one ulp per step in the moments is possible;
    a real error in the arithmetic (a missing bias correction, AdamW decay, wrong beta) is orders of magnitude larger."""
    lib = L.lib()
    n = 4 * 1031 + 3
    gen = torch.Generator(device=DEV).manual_seed(3)
    p = (torch.randn(n, device=DEV, generator=gen) * 0.1).contiguous()
    p_init = p.clone()
    ref = torch.nn.Parameter(p.clone())
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lr_val = float(np.float32(1e-3))
    lr, step, scal = torch.full((1,), lr_val, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    opt = L.Optim(kind=L.OPT_ADAM, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, nesterov=0,
                  lr=L.ptr(lr).value, adam_scal=L.ptr(scal).value, state0=L.ptr(m).value, state1=L.ptr(v).value)
    topt = torch.optim.Adam([ref], lr=lr_val, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    g = torch.zeros(n, device=DEV)
    import ctypes as C
    for k in range(10):
        g.copy_(torch.randn(n, device=DEV, generator=gen) * (10.0 ** (k % 3 - 3)))
        g[100:300] = 0.0                                   # exactly-zero gradients
        L.check(lib.nunet_adam_prepare(L.ptr(lr), 0.9, 0.999, L.ptr(step), L.ptr(scal), L.stream()), "adam_prepare")
        L.check(lib.nunet_adam_step(L.ptr(p), L.ptr(g), C.byref(opt), n, 0.5, L.stream()), "adam_step")
        ref.grad = g * 0.5
        topt.step()
    torch.cuda.synchronize()
    st = topt.state[ref]
    assert float(step) == 10.0 and float(st["step"]) == 10.0
    for mine, theirs, nm in ((p, ref.detach(), "param"), (m, st["exp_avg"], "exp_avg"), (v, st["exp_avg_sq"], "exp_avg_sq")):
        err = (mine - theirs).abs()
        bound = 8 * ULP * theirs.abs() + 1e-6 * float(theirs.abs().max())
        assert bool((err <= bound).all()), (nm, float((err / (theirs.abs() + 1e-30)).max()))
    if wd == 0.0:       # no gradient ever, no decay: the state stays zero and the parameters do not move
        assert float(m[100:300].abs().max()) == 0.0 and float(v[100:300].abs().max()) == 0.0
        assert torch.equal(p[100:300], p_init[100:300])


def _adam_state(ts, seed=7):
    """a non-trivial Adam state: moments of the magnitude a few steps leave, t = 5"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ts.exp_avg.copy_(torch.randn(ts.exp_avg.shape, device=DEV, generator=gen) * 1e-3)
    ts.exp_avg_sq.copy_((torch.randn(ts.exp_avg_sq.shape, device=DEV, generator=gen) * 1e-3) ** 2 + 1e-8)
    ts.adam_step.fill_(5.0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", [2])
def test_fused_adam_layouts_equal_unpack_plus_flat_adam(dtype, mode, synth):
    """nunet_plan_opt_step with Adam (layout 2, unpack_sgd_tiled_kernel)
    against unpack + the flat Adam step (layout 0) on the SAME gradient scratch from the SAME non-trivial state. The conv tiles'
    gradients are exact copies either way; the 1x1 heads' slabs are summed in another order (the bound of
    test_fused_update_equals_unpack_sgd_pack, 1e-5 of the largest gradient). Adam divides by sqrt(v) ~ 1e-3 here, so the
    parameters are bounded relative to the update (1e-4 of its largest move), the moments as in the SGD test."""
    st = synth.closed_form_state(1, 3, False, True)
    m = _module(st, dtype=dtype)
    x, t = _batch(synth, 2, 32, 1234)
    ts = TrainStep(m, tuple(x.shape), lr=1e-3, weight_decay=1e-3, use_graph=False, fused_update=0, keep_grads=True, optimizer="Adam")
    ts.x.copy_(x); ts.t.copy_(t)
    _adam_state(ts)
    ts._fwd_loss(); ts._bwd(3)                     # t = 6 prepared, gradient scratch complete, not yet unpacked
    eng = ts.eng
    p0, m0, v0 = eng.flat_params.clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone()
    ts._bwd(4); ts._opt()                          # reference: unpack + nunet_opt_step
    torch.cuda.synchronize()
    pa, ma, va, ga = eng.flat_params.clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone(), eng.flat_grads.clone()
    eng.flat_params.copy_(p0); ts.exp_avg.copy_(m0); ts.exp_avg_sq.copy_(v0); eng.flat_grads.zero_()
    ts.fused_update = mode
    ts._opt()
    torch.cuda.synchronize()
    pb, mb, vb, gb = eng.flat_params.clone(), ts.exp_avg.clone(), ts.exp_avg_sq.clone(), eng.flat_grads.clone()
    assert float(ts.adam_step) == 6.0
    assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())
    assert float((pa - pb).abs().max()) <= 1e-4 * float((pa - p0).abs().max())
    assert float((ma - mb).abs().max()) <= 1e-5 * float(ma.abs().max()) + 1e-9
    assert float((va - vb).abs().max()) <= 1e-5 * float(va.abs().max()) + 1e-12
    assert float((pa - p0).abs().max()) > 0.0


@pytest.mark.parametrize("mode", [0, 2])
def test_adam_graph_replay_equals_eager(mode, synth):
    """The captured Adam step replays bit for bit what the eager step computes (3 steps), the device step counter counts the
    steps taken (warm-up and capture leave no trace), and an lr set between replays reaches the step's scalars."""
    st = synth.closed_form_state(1, 3, False, True)
    batches = [_batch(synth, 4, 32, 1234 + k) for k in range(4)]
    outs = []
    for graph in (False, True):
        m = _module(st)
        ts = TrainStep(m, (4, 3, 32, 32), lr=1e-3, weight_decay=1e-4, use_graph=graph, fused_update=mode, optimizer="Adam")
        if graph:
            ts.capture(*batches[0])
        for x, t in batches[:3]:
            ts.step(x, t)
        torch.cuda.synchronize()
        assert float(ts.adam_step) == 3.0
        ts.set_lr(5e-3)
        ts.step(*batches[3])
        torch.cuda.synchronize()
        assert float(ts.adam_step) == 4.0
        ss = ts.adam_scal.tolist()
        assert abs(ss[0] - 5e-3 / (1 - 0.9 ** 4)) <= 1e-6 * ss[0]
        assert abs(ss[1] - 1 / (1 - 0.999 ** 4) ** 0.5) <= 1e-6 * ss[1]
        outs.append([a.clone() for a in (ts.eng.flat_params, ts.exp_avg, ts.exp_avg_sq, ts.eng.bnbuf, ts.loss_out)])
    for a, b, nm in zip(outs[0], outs[1], ("params", "exp_avg", "exp_avg_sq", "bn buffers", "loss")):
        assert torch.equal(a, b), nm


def test_fused_adam_step_against_oracle(synth):
    """TrainStep(optimizer='Adam'), eager and captured, against OracleNet + torch.optim.Adam over 3 steps in fp32 (loss / IoU bands
    of test_fused_train_step_graph_matches_eager_and_oracle). Parameter bound: Adam's first steps move every element by about
    lr * sign(g) whatever |g| is, so an element whose gradient lies within the fp32 gradient error of zero may move the other
    way: a max-abs bound says nothing. What is bounded is the update as a whole, in norm: |dw_hip - dw_oracle| <= 15 % of
    |dw_oracle| for deep layers (measured after 3 steps: 5.2 % on conv0_4.conv2.weight, 0.3 % on conv0_4.bn2.weight, 10 % on
    conv3_1.conv1.weight; the few sign-flipping elements dominate the difference and their number varies from layer to layer). A wrong step - no bias
    correction, decoupled decay, a stale t - is off by far more. The pre-BN conv biases are left out: BatchNorm cancels their gradients, which are noise that Adam
    turns into lr-sized moves."""
    n, hw = 4, 32
    st = synth.closed_form_state(1, 3, False, True)
    batches = [synth.synth_batch(n, hw, hw, 3, 1, seed=1234 + k) for k in range(3)]
    net = O.OracleNet(st, 1, 3, False)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    ref = [O.train_step(net, opt, torch.from_numpy(b[0]), torch.from_numpy(b[1])) for b in batches]
    for graph in (False, True):
        m = _module(st)
        ts = TrainStep(m, (n, 3, hw, hw), lr=1e-3, weight_decay=1e-4, use_graph=graph, optimizer="Adam")
        if graph:
            ts.capture(torch.from_numpy(batches[0][0]).to(DEV), torch.from_numpy(batches[0][1]).to(DEV))
        for k, b in enumerate(batches):
            ts.reset_meters()
            ts.step(torch.from_numpy(b[0]).to(DEV), torch.from_numpy(b[1]).to(DEV))
            loss, iou = ts.epoch_stats()
            assert abs(loss - ref[k][0]) < (1e-4 if k == 0 else 3e-3), (graph, k, loss, ref[k][0])
            assert abs(iou - ref[k][1]) < 2e-2, (graph, k, iou, ref[k][1])
        assert bool(torch.isfinite(ts.eng.flat_params).all())
        for name in ("conv0_4.conv2.weight", "conv0_4.bn2.weight", "conv3_1.conv1.weight"):
            w0 = torch.from_numpy(np.asarray(st[name])).double()
            w = dict(m.named_parameters())[name].detach().cpu().double()
            rw = net.params[name].detach().double()
            dref = rw - w0
            assert float(dref.norm()) > 0
            rel = float((w - rw).norm() / dref.norm())
            print("update difference vs oracle", graph, name, rel)
            assert rel <= 0.15, (graph, name, rel)


def test_adam_trajectory_against_reference(synth):
    """8 captured Adam steps + cosine schedule against the reference's (tests/golden/make_golden_adam.py), bands of
    test_trajectory_against_reference; the second step - the first after an update - is held to 2e-3 (Adam's sign-like first
    step amplifies the fp32 gradient noise of near-zero elements more than SGD's)."""
    g = load_golden("trajectory_adam_n4_32x32")
    m = _module(synth.closed_form_state(1, 3, False, True))
    batches = [_batch(synth, 4, 32, 1234 + k) for k in range(8)]
    ts = TrainStep(m, (4, 3, 32, 32), lr=1e-3, weight_decay=1e-4, optimizer="Adam")
    ts.capture(*batches[0])
    step = 0
    for ep in range(4):
        lr = cosine_lr(1e-3, 1e-5, ep, 4)
        ts.set_lr(lr)
        for _ in range(2):
            ts.reset_meters()
            ts.step(*batches[step])
            loss, iou = ts.epoch_stats()
            assert abs(lr - g["lr"][step]) < 1e-12
            assert abs(loss - g["loss"][step]) < (1e-4 if step == 0 else 2e-3 if step == 1 else 2e-2), (step, loss, g["loss"][step])
            assert abs(iou - g["iou"][step]) < (5e-3 if step < 2 else 5e-2), (step, iou, g["iou"][step])
            step += 1
    m.eval()
    img, msk = synth.synth_batch(4, 32, 32, 3, 1, seed=99)
    with torch.no_grad():
        o = m(torch.from_numpy(img).to(DEV))
    vloss = float(nunet_amd.losses.BCEDiceLoss()(o, torch.from_numpy(msk).to(DEV)))
    assert abs(vloss - float(g["val_loss"])) < 3e-2


def test_adam_state_round_trip(synth):
    """optimizer_state_dict() after 3 fused steps, loaded with the module state into a fresh TrainStep: its next step is
    bit-identical to the uninterrupted run's. The same dict loads into a stock torch.optim.Adam over the module's parameters."""
    st = synth.closed_form_state(1, 3, False, True)
    batches = [_batch(synth, 4, 32, 1234 + k) for k in range(4)]
    m = _module(st)
    ts = TrainStep(m, (4, 3, 32, 32), lr=1e-3, weight_decay=1e-4, optimizer="Adam")
    ts.capture(*batches[0])
    for x, t in batches[:3]:
        ts.step(x, t)
    torch.cuda.synchronize()
    msd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    osd = ts.optimizer_state_dict()
    assert float(osd["state"][0]["step"]) == 3.0
    assert osd["param_groups"][0]["betas"] == (0.9, 0.999) and osd["param_groups"][0]["amsgrad"] is False
    ts.step(*batches[3])
    torch.cuda.synchronize()
    p_cont = ts.eng.flat_params.clone()
    m2 = _module(msd)
    ts2 = TrainStep(m2, (4, 3, 32, 32), lr=0.5, weight_decay=1e-4, optimizer="Adam")
    ts2.load_optimizer_state_dict(osd)
    assert float(ts2.lr) == float(ts.lr) and float(ts2.adam_step) == 3.0
    ts2.capture(*batches[0])
    ts2.step(*batches[3])
    torch.cuda.synchronize()
    assert torch.equal(ts2.eng.flat_params, p_cont)
    assert float(ts2.adam_step) == 4.0
    params = [p for p in m2.parameters() if p.requires_grad]
    stock = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-4)
    stock.load_state_dict(osd)
    for i, p in enumerate(params):
        s = stock.state[p]
        assert torch.equal(s["exp_avg"].cpu(), osd["state"][i]["exp_avg"]) and s["exp_avg"].shape == p.shape
        assert float(s["step"]) == 3.0


def test_unknown_optimizer_is_refused(synth):
    m = _module(synth.closed_form_state(1, 3, False, True))
    with pytest.raises(L.NunetError):
        TrainStep(m, (2, 3, 32, 32), optimizer="AdamW")


def test_train_py_adam_runs_the_fused_step(tmp_path):
    """train.py --optimizer Adam (reference trains.py:73-76,225-227) for 2 epochs on a small synthetic set, as a child
    process under a time limit: it takes the fused step and logs a finite val_iou."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--optimizer", "Adam", "--epochs", "2", "--train_size", "64",
           "--val_size", "32", "--input_h", "32", "--input_w", "32", "-b", "8", "--name", "adam_e2e"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "=> fused training step (TrainStep): Adam" in r.stdout, r.stdout[-2000:]
    rows = open(tmp_path / "models" / "adam_e2e" / "log.csv").read().strip().splitlines()
    head = rows[0].split(",")
    assert len(rows) == 3
    last = dict(zip(head, rows[-1].split(",")))
    assert np.isfinite(float(last["val_iou"])) and np.isfinite(float(last["loss"]))
