"""CPU side of dynamic loss scaling (TrainStep(loss_scale=...)): the pure-torch restatement of the scale update follows a real
torch.amp.GradScaler("cpu") step by step, the state-dict format round-trips through one, and the new ABI entries refuse bad
arguments before touching a device."""
import ctypes as C

import pytest
import torch

from nunet_amd import _lib as L
from nunet_amd import loss_scale as LS


def _drive(scaler, p, opt, found_inf):
    """One GradScaler step with a gradient that is (found_inf) or is not non-finite; returns whether the step was skipped."""
    scaler.scale(torch.ones(()))           # (GradScaler creates its state lazily, at the first scale())
    p.grad = torch.tensor([float("inf") if found_inf else 1.0])
    before = p.detach().clone()
    scaler.step(opt)
    scaler.update()
    return bool(torch.equal(before, p.detach()))


@pytest.mark.parametrize("settings", [dict(), dict(init_scale=2.0 ** 20, growth_interval=3),
                                      dict(init_scale=1000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=2)])
def test_update_rule_matches_grad_scaler(settings):
    cfg = LS.scaler_settings(settings if settings else "dynamic")
    scaler = torch.amp.GradScaler("cpu", **settings)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.5)
    script = [1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    scale, tracker = cfg["init_scale"], 0
    for found in script:
        skipped = _drive(scaler, p, opt, found)
        assert skipped == bool(found)
        scale, tracker = LS.update_scale(scale, tracker, found, cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"])
        assert scale == scaler.get_scale(), (found, scale, scaler.get_scale())
        assert tracker == scaler._get_growth_tracker()
        assert LS.inv_scale(scale) == scaler._scale.double().reciprocal().float().item()


def test_growth_is_capped_at_fp32_max():
    """A grown scale that overflows fp32 is not taken; the tracker still resets (torch's _amp_update_scale_)."""
    big = 2.0 ** 127
    scaler = torch.amp.GradScaler("cpu", init_scale=big, growth_interval=1)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.5)
    scale, tracker = big, 0
    for _ in range(3):
        _drive(scaler, p, opt, False)
        scale, tracker = LS.update_scale(scale, tracker, False, 2.0, 0.5, 1)
        assert scale == scaler.get_scale() == big and tracker == scaler._get_growth_tracker() == 0
    near = float(torch.finfo(torch.float32).max) / 1.5       # * 2 overflows fp32, but not double
    scale, tracker = LS.update_scale(near, 0, False, 2.0, 0.5, 1)
    assert scale == torch.tensor(near, dtype=torch.float32).item() and tracker == 0


def test_state_dict_round_trips_through_grad_scaler():
    scaler = torch.amp.GradScaler("cpu", init_scale=4096.0, growth_factor=4.0, backoff_factor=0.125, growth_interval=7)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.5)
    for found in (0, 0, 1, 0):
        _drive(scaler, p, opt, found)
    sd = scaler.state_dict()
    scale, tracker, cfg = LS.from_state_dict(sd)
    mine = LS.to_state_dict(scale, tracker, cfg)
    assert mine == sd and all(type(mine[k]) is type(sd[k]) for k in sd)
    fresh = torch.amp.GradScaler("cpu")
    fresh.load_state_dict(mine)
    assert fresh.state_dict() == sd


def test_settings():
    assert LS.scaler_settings(None) is None
    assert LS.scaler_settings("dynamic") == dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    assert LS.scaler_settings(dict(init_scale=8)) == dict(init_scale=8.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    for bad in (dict(init_scale=0.0), dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(backoff_factor=0.0),
                dict(growth_interval=0), dict(scale=2.0), "static"):
        with pytest.raises(ValueError):
            LS.scaler_settings(bad)


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def test_abi_refuses_bad_arguments(lib):
    """Every new entry validates before it launches: a null pointer or a bad factor returns NUNET_EINVAL with a message, and
    no stream is touched (the pointers below are never dereferenced)."""
    fake = C.c_void_p(0x1000)        # never dereferenced: validation fails first
    EINVAL = -1

    def einval(rc, word):
        msg = lib.nunet_last_error().decode()
        return rc == EINVAL and word in msg, (rc, msg)

    assert lib.nunet_scaler_check(None, 16, fake, None) == EINVAL
    assert lib.nunet_scaler_check(fake, 16, None, None) == EINVAL
    assert lib.nunet_scaler_check(fake, 0, fake, None) == EINVAL
    ok, info = einval(lib.nunet_scaler_update(None, 2.0, 0.5, 10, None), "null")
    assert ok, info
    for gf, bf, gi, word in ((1.0, 0.5, 10, "growth_factor"), (-2.0, 0.5, 10, "growth_factor"), (float("inf"), 0.5, 10, "growth_factor"),
                             (2.0, 0.0, 10, "backoff_factor"), (2.0, -0.5, 10, "backoff_factor"), (2.0, 1.0, 10, "backoff_factor"),
                             (2.0, 0.5, 0, "growth_interval")):
        ok, info = einval(lib.nunet_scaler_update(fake, gf, bf, gi, None), word)
        assert ok, (gf, bf, gi, info)
    assert lib.nunet_adam_prepare_scaled(fake, 0.9, 0.999, fake, fake, None, None) == EINVAL
    assert lib.nunet_adam_prepare_scaled(fake, 1.0, 0.999, fake, fake, fake, None) == EINVAL
    ws = 1 << 20
    assert lib.nunet_loss_step_scaled(fake, fake, 2, 64, 1, L.LOSS_BCE_DICE, fake, ws, fake, fake, None, 0.0, None, None) == EINVAL
    assert lib.nunet_loss_step_scaled(fake, fake, 0, 64, 1, L.LOSS_BCE_DICE, fake, ws, fake, fake, None, 0.0, fake, None) == EINVAL
    opt = L.Optim(kind=L.OPT_SGD, momentum=0.9, lr=None, state0=fake.value, scaler=fake.value)
    assert lib.nunet_opt_step(fake, fake, C.byref(opt), 16, 1.0, None) == EINVAL
    opt = L.Optim(kind=7, lr=fake.value, state0=fake.value)
    assert lib.nunet_opt_step(fake, fake, C.byref(opt), 16, 1.0, None) == EINVAL
    opt = L.Optim(kind=L.OPT_ADAM, beta1=0.9, beta2=0.999, eps=1e-8, adam_scal=fake.value, state0=fake.value, state1=None)
    assert lib.nunet_opt_step(fake, fake, C.byref(opt), 16, 1.0, None) == EINVAL
    # the flat Adam entry refuses a scaler: it cannot honour a skipped step the way the scaled entries do
    opt = L.Optim(kind=L.OPT_ADAM, beta1=0.9, beta2=0.999, eps=1e-8, adam_scal=fake.value, state0=fake.value, state1=fake.value,
                  scaler=fake.value)
    ok, info = einval(lib.nunet_adam_step(fake, fake, C.byref(opt), 16, 1.0, None), "nunet_opt_step")
    assert ok, info
