"""CPU side of the fused Adam step (trainer.TrainStep(optimizer='Adam')): the oracle with a stock torch.optim.Adam follows
the reference's Adam trajectory (tests/golden/make_golden_adam.py), the flat <-> torch.optim state-dict packing round-trips
against a real torch.optim.Adam, and the new ABI entries refuse bad arguments before touching a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import nunet_oracle as O

import nunet_amd
from nunet_amd import _lib as L
from nunet_amd.optim_state import flat_to_torch_state, torch_state_to_flat


def test_oracle_adam_trajectory(synth):
    """OracleNet + torch.optim.Adam(lr 1e-3, wd 1e-4) + the closed-form cosine lr reproduce the reference's 8 steps
    (bands of test_oracle_trajectory)."""
    g = load_golden("trajectory_adam_n4_32x32")
    net = O.OracleNet(synth.closed_form_state(1, 3, False, True), 1, 3, False)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    step = 0
    for ep in range(4):
        lr = O.cosine_lr(1e-3, 1e-5, ep, 4)
        for grp in opt.param_groups:
            grp["lr"] = lr
        for _ in range(2):
            img, msk = synth.synth_batch(4, 32, 32, 3, 1, seed=1234 + step)
            loss, iou = O.train_step(net, opt, torch.from_numpy(img), torch.from_numpy(msk))
            assert abs(lr - g["lr"][step]) < 1e-12
            assert abs(loss - g["loss"][step]) < 2e-4, (step, loss, g["loss"][step])
            assert abs(iou - g["iou"][step]) < 2e-3, (step, iou, g["iou"][step])
            step += 1
    net.eval()
    img, msk = synth.synth_batch(4, 32, 32, 3, 1, seed=99)
    with torch.no_grad():
        o = net(torch.from_numpy(img))
    assert abs(float(O.bce_dice_loss(o, torch.from_numpy(msk))) - float(g["val_loss"])) < 1e-3


def _layout(params):
    out, off = [], 0
    for p in params:
        out.append((off, p.shape))
        off += p.numel()
    return out, off


@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_state_dict_packing_matches_torch_optim(kind):
    """flat_to_torch_state writes what a real torch optimiser over NestedUNet(1,3,False).parameters() writes after one step
    (keys, shapes, step, param_groups), the stock optimiser loads it, and torch_state_to_flat inverts it exactly."""
    torch.manual_seed(0)
    m = nunet_amd.archs.NestedUNet(1, 3, False)
    params = [p for p in m.parameters() if p.requires_grad]
    if kind == "Adam":
        hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, amsgrad=False)
        opt = torch.optim.Adam(params, **hyper)
        names = ("exp_avg", "exp_avg_sq")
    else:
        hyper = dict(lr=1e-2, momentum=0.9, dampening=0, weight_decay=1e-4, nesterov=False)
        opt = torch.optim.SGD(params, **hyper)
        names = ("momentum_buffer",)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    ref = opt.state_dict()
    layout, n = _layout(params)
    flat = {k: torch.cat([ref["state"][i][k].reshape(-1) for i in range(len(params))]) for k in names}
    sd = flat_to_torch_state(layout, flat, 1.0 if kind == "Adam" else None, hyper)
    assert sd["param_groups"] == ref["param_groups"]
    assert sorted(sd["state"]) == sorted(ref["state"])
    for i in ref["state"]:
        assert sorted(sd["state"][i]) == sorted(ref["state"][i]), i
        for k, v in ref["state"][i].items():
            assert sd["state"][i][k].shape == v.shape and sd["state"][i][k].dtype == v.dtype, (i, k)
            assert torch.equal(sd["state"][i][k], v), (i, k)
    # a stock optimiser loads it and continues identically
    opt2 = type(opt)(params, **hyper)
    opt2.load_state_dict(sd)
    assert torch.equal(torch.cat([opt2.state[p][names[0]].reshape(-1) for p in params]), flat[names[0]])
    # and back to flat buffers, bit for bit
    back = {k: torch.full((n,), float("nan")) for k in names}
    step, lr = torch_state_to_flat(ref, layout, back)
    for k in names:
        assert torch.equal(back[k], flat[k]), k
    assert lr == hyper["lr"]
    assert step == (1.0 if kind == "Adam" else None)


def test_state_dict_packing_rejects_mismatched_model():
    layout = [(0, torch.Size([2, 3])), (6, torch.Size([4]))]
    sd = {"state": {0: {"step": torch.tensor(1.0), "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(6)}},
          "param_groups": [{"lr": 1e-3, "params": [0, 1]}]}
    with pytest.raises(ValueError):
        torch_state_to_flat(sd, layout, {"exp_avg": torch.zeros(10)})
    sd["param_groups"][0]["params"] = [0]
    with pytest.raises(ValueError):
        torch_state_to_flat(sd, layout, {"exp_avg": torch.zeros(10)})


def _optim(**kw):
    fake = 0x1000          # never dereferenced: every call below is refused before it reaches the device
    d = dict(kind=L.OPT_ADAM, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, nesterov=0,
             lr=fake, adam_scal=fake, state0=fake, state1=fake)
    d.update(kw)
    return L.Optim(**d)


def test_adam_abi_rejects_bad_arguments():
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    s = None
    bad = [_optim(beta1=1.0), _optim(beta1=-0.1), _optim(beta2=1.0), _optim(eps=0.0), _optim(eps=-1e-8),
           _optim(state0=None), _optim(state1=None), _optim(adam_scal=None), _optim(kind=7), _optim(kind=L.OPT_SGD, lr=None)]
    for o in bad:
        assert lib.nunet_plan_opt_step(fake, fake, C.byref(o), fake, 1 << 40, 1.0, None, s) == -1
    for o in bad[:-2]:
        assert lib.nunet_adam_step(fake, fake, C.byref(o), 16, 1.0, s) == -1
    assert lib.nunet_adam_step(fake, fake, C.byref(_optim(kind=L.OPT_SGD)), 16, 1.0, s) == -1      # not an Adam optimiser
    assert lib.nunet_adam_step(fake, fake, C.byref(_optim()), 0, 1.0, s) == -1                      # n <= 0
    assert lib.nunet_adam_step(fake, fake, None, 16, 1.0, s) == -1
    assert lib.nunet_adam_step(None, fake, C.byref(_optim()), 16, 1.0, s) == -1
    assert lib.nunet_adam_prepare(fake, 1.0, 0.999, fake, fake, s) == -1
    assert lib.nunet_adam_prepare(fake, 0.9, -0.5, fake, fake, s) == -1
    assert lib.nunet_adam_prepare(None, 0.9, 0.999, fake, fake, s) == -1
    assert lib.nunet_adam_prepare(fake, 0.9, 0.999, None, fake, s) == -1
    assert lib.nunet_plan_opt_step(None, fake, C.byref(_optim()), fake, 1 << 40, 1.0, None, s) == -1
    assert lib.nunet_plan_opt_step(fake, fake, None, fake, 1 << 40, 1.0, None, s) == -1
    assert b"null optimiser" in lib.nunet_last_error()


def test_plan_optimiser_entries_disarm_and_sgd_state():
    """The plan's optimiser entry on a real plan. The plan kernel loads SGD's momentum buffer whatever the momentum, so it
    refuses state0 = NULL; the flat kernel reads it only when momentum != 0, so nunet_opt_step lets that descriptor through - seen without a device as the
    next refusal in line (n <= 0), while with momentum != 0 the missing buffer is what it reports."""
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    cfg = L.PlanCfg(2, 32, 32, 3, 1, 0, L.F32, 0)
    plan = lib.nunet_plan_create(C.byref(cfg))
    assert plan
    try:
        sgd = _optim(kind=L.OPT_SGD, momentum=0.0, adam_scal=None, state0=None, state1=None)
        assert lib.nunet_plan_opt_step(plan, fake, C.byref(sgd), fake, 1 << 40, 1.0, None, None) == -1
        assert b"state0" in lib.nunet_last_error()
    finally:
        lib.nunet_plan_destroy(plan)
    assert lib.nunet_opt_step(fake, fake, C.byref(sgd), 0, 1.0, None) == -1
    assert b"state0" not in lib.nunet_last_error() and b"bad args" in lib.nunet_last_error()
    sgd.momentum = 0.9
    assert lib.nunet_opt_step(fake, fake, C.byref(sgd), 0, 1.0, None) == -1
    assert b"state0" in lib.nunet_last_error()
