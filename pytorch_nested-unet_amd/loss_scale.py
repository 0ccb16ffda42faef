"""Dynamic loss scaling rule and state format (pure torch, no device code).

TrainStep(loss_scale=...) keeps torch.amp.GradScaler's state on the device and updates it with a one-thread kernel
(nunet_scaler_update, include/nunet.h). This module restates that update in torch so that tests and tools can replay it on
the host, and translates between the settings TrainStep takes and torch.amp.GradScaler.state_dict()'s format.
"""
import math

import torch

DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)


def scaler_settings(loss_scale):
    """TrainStep's loss_scale argument -> None (no scaling) or a full settings dict: "dynamic" gives torch's defaults, a dict
    with GradScaler's constructor names overrides them."""
    if loss_scale is None or loss_scale is False:
        return None
    if loss_scale == "dynamic" or loss_scale is True:
        return dict(DEFAULTS)
    if not isinstance(loss_scale, dict):
        raise ValueError("loss_scale must be None, 'dynamic' or a dict of %s, got %r" % (sorted(DEFAULTS), loss_scale))
    unknown = set(loss_scale) - set(DEFAULTS)
    if unknown:
        raise ValueError("loss_scale: unknown settings %s (GradScaler's are %s)" % (sorted(unknown), sorted(DEFAULTS)))
    s = dict(DEFAULTS)
    s.update(loss_scale)
    s["init_scale"] = float(s["init_scale"])
    s["growth_factor"] = float(s["growth_factor"])
    s["backoff_factor"] = float(s["backoff_factor"])
    s["growth_interval"] = int(s["growth_interval"])
    check_settings(s)
    return s


def check_settings(s):
    if not (s["init_scale"] > 0.0 and math.isfinite(s["init_scale"])):
        raise ValueError("loss_scale: init_scale must be a finite number > 0, got %r" % s["init_scale"])
    if not (s["growth_factor"] > 1.0 and math.isfinite(s["growth_factor"])):
        raise ValueError("loss_scale: growth_factor must be > 1, got %r" % s["growth_factor"])
    if not (0.0 < s["backoff_factor"] < 1.0):
        raise ValueError("loss_scale: backoff_factor must lie in (0, 1), got %r" % s["backoff_factor"])
    if not (0 < s["growth_interval"] < 2 ** 31):
        raise ValueError("loss_scale: growth_interval must be a positive int32, got %r" % s["growth_interval"])


def inv_scale(scale):
    """1 / scale as torch's unscale_ forms it: the reciprocal in double, rounded to fp32."""
    return torch.tensor([scale], dtype=torch.float32).double().reciprocal().float().item()


def update_scale(scale, tracker, found_inf, growth_factor, backoff_factor, growth_interval):
    """One step of torch's _amp_update_scale_: (scale, growth_tracker) after a step that did (found_inf) or did not find a
    non-finite gradient. scale is an fp32 value; the factors are Python floats (doubles): products are formed in double and
    rounded to fp32 once, and a grown scale that is not finite in fp32 is not taken."""
    s32 = torch.tensor([scale], dtype=torch.float32)
    if found_inf:
        return (s32.double() * backoff_factor).float().item(), 0
    t = tracker + 1
    if t == growth_interval:
        grown = (s32.double() * growth_factor).float()
        return (grown.item() if bool(torch.isfinite(grown)) else s32.item()), 0
    return s32.item(), t


def to_state_dict(scale, tracker, settings):
    """torch.amp.GradScaler.state_dict()'s format."""
    return {"scale": float(scale), "growth_factor": float(settings["growth_factor"]),
            "backoff_factor": float(settings["backoff_factor"]), "growth_interval": int(settings["growth_interval"]),
            "_growth_tracker": int(tracker)}


def from_state_dict(sd):
    """Inverse of to_state_dict (and what torch.amp.GradScaler.state_dict() writes): (scale, tracker, settings)."""
    missing = {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"} - set(sd)
    if missing:
        raise ValueError("not a GradScaler state dict: %s missing" % sorted(missing))
    settings = dict(init_scale=float(sd["scale"]), growth_factor=float(sd["growth_factor"]),
                    backoff_factor=float(sd["backoff_factor"]), growth_interval=int(sd["growth_interval"]))
    check_settings(settings)
    return float(sd["scale"]), int(sd["_growth_tracker"]), settings
