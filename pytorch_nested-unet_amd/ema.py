"""Weight EMA rule and state format (pure torch, no device code).

TrainStep(ema_decay=...) keeps an exponential moving average of the parameters and of the BatchNorm running statistics on
the device and updates it inside the captured step (nunet_ema, include/nunet.h): what
torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True) does with one
update_parameters(model) per applied step. This module restates that recurrence on the host, in any dtype, so that tests and
tools can replay it, and translates between the flat averaged arenas and model.state_dict()'s format.
"""
from collections import OrderedDict

import torch


def check_decay(decay):
    """The decay as a float; raises NunetError unless it lies in [0, 1)."""
    from ._lib import NunetError
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise NunetError("ema_decay must be None or a number in [0, 1) (got %r)" % (decay,))
    if not (0.0 <= d < 1.0):
        raise NunetError("ema_decay must lie in [0, 1) (got %r)" % (decay,))
    return d


def decay_at(decay, warmup, n_averaged):
    """d_t of the update that finds `n_averaged` earlier ones (>= 1): decay, or with warmup min(decay, (1 + n) / (10 + n))."""
    n = int(n_averaged)
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def weight(decay, warmup, n_averaged):
    """The lerp weight of the update that finds `n_averaged` earlier ones, as the device forms it: 1.0 for the first (a copy),
    else 1 - d_t in double, rounded to fp32 once (how torch's lerp_ receives its Python-float weight). Returned as a Python
    float holding the fp32 value."""
    if int(n_averaged) == 0:
        return 1.0
    return torch.tensor([1.0 - decay_at(decay, warmup, n_averaged)], dtype=torch.float64).float().item()


class Recurrence:
    """The averaging rule over a list of tensors, in `dtype` (default fp64): update(tensors) after every applied step; a
    skipped step calls nothing. values[k] is the average of tensors[k]; n_averaged counts the updates."""

    def __init__(self, decay, warmup=False, dtype=torch.float64):
        self.decay, self.warmup, self.dtype = check_decay(decay), bool(warmup), dtype
        self.values = None
        self.n_averaged = 0
        self.w = 0.0

    def update(self, tensors):
        cur = [t.detach().to("cpu", self.dtype).clone() for t in tensors]
        self.w = weight(self.decay, self.warmup, self.n_averaged)
        if self.n_averaged == 0:
            self.values = cur
        else:
            self.values = [e + self.w * (p - e) for e, p in zip(self.values, cur)]
        self.n_averaged += 1
        return self.values


def _layout(model, eng):
    """state_dict key -> ("p" | "b", offset, shape) into the flat parameter / BatchNorm arenas; keys that are neither (the
    num_batches_tracked counters) are absent."""
    out = {}
    for name, p, off in zip(eng.param_names, eng.module_params, eng.param_off):
        out[name] = ("p", off, tuple(p.shape))
    off = 0
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            pre = name + "." if name else ""
            out[pre + "running_mean"] = ("b", off, (c,))
            out[pre + "running_var"] = ("b", off + c, (c,))
            off += 2 * c
    return out


def state_dict_from_flat(model, eng, flat_params, bnbuf):
    """OrderedDict with model.state_dict()'s keys, shapes and dtypes: parameters from `flat_params`, running statistics from
    `bnbuf` (copies), everything else - num_batches_tracked - the live model's value."""
    lay = _layout(model, eng)
    arenas = {"p": flat_params, "b": bnbuf}
    out = OrderedDict()
    for k, v in model.state_dict().items():
        if k in lay:
            kind, off, shape = lay[k]
            n = 1
            for d in shape:
                n *= d
            out[k] = arenas[kind][off:off + n].view(shape).clone().to(v.dtype)
        else:
            out[k] = v.detach().clone()
    return out


def flat_from_state_dict(model, eng, sd, flat_params, bnbuf):
    """Inverse of state_dict_from_flat: the parameters and running statistics of `sd` are copied into the flat arenas; a
    missing key or a wrong shape raises."""
    from ._lib import NunetError
    arenas = {"p": flat_params, "b": bnbuf}
    for k, (kind, off, shape) in _layout(model, eng).items():
        if k not in sd:
            raise NunetError("load_ema_state_dict: key %r is missing" % k)
        if tuple(sd[k].shape) != shape:
            raise NunetError("load_ema_state_dict: %r has shape %s, the model's is %s" % (k, tuple(sd[k].shape), shape))
        with torch.no_grad():
            arenas[kind][off:off + sd[k].numel()].view(shape).copy_(sd[k])
