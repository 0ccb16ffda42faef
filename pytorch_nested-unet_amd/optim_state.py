"""Flat optimiser state <-> torch.optim state dicts (pure torch, no device code).

TrainStep keeps every optimiser buffer as ONE flat fp32 tensor in parameter order (what its kernels stream). torch.optim keeps
per-parameter tensors keyed by the parameter's index in the optimiser's parameter list - for train.py's optimisers,
filter(requires_grad, model.parameters()) (reference trains.py:221-231). These two functions translate between the forms, so
that a checkpoint taken from the fused step resumes under a stock torch optimiser and the reverse.
"""
import torch


def _param_group(hyper, n):
    """param_groups[0] as the installed torch writes it for these hyper-parameters (Adam when `betas` is given, else SGD)."""
    h = dict(hyper)
    opt = torch.optim.Adam if "betas" in h else torch.optim.SGD
    g = opt([torch.zeros(1, requires_grad=True)], **h).state_dict()["param_groups"][0]
    g["params"] = list(range(n))
    return g


def flat_to_torch_state(layout, flat, step, hyper):
    """layout: [(offset, shape)] of the trainable parameters in optimiser order; flat: {state name: flat fp32 tensor}
    ('exp_avg', 'exp_avg_sq' for Adam, 'momentum_buffer' for SGD); step: Adam's step count (None for SGD); hyper: the
    constructor arguments of the torch optimiser (lr, betas, eps, weight_decay, amsgrad / momentum, dampening, weight_decay,
    nesterov). Returns {'state': {i: {...}}, 'param_groups': [...]} with CPU tensors."""
    state = {}
    host = {k: v.detach().to("cpu", torch.float32) for k, v in flat.items()}
    for i, (off, shape) in enumerate(layout):
        n = 1
        for s in shape:
            n *= int(s)
        st = {}
        if step is not None:
            st["step"] = torch.tensor(float(step), dtype=torch.float32)
        for k, v in host.items():
            st[k] = v[off:off + n].reshape(shape).clone()
        state[i] = st
    return {"state": state, "param_groups": [_param_group(hyper, len(layout))]}


def torch_state_to_flat(sd, layout, flat):
    """Inverse of flat_to_torch_state: the per-parameter tensors of `sd` are written into the flat buffers of `flat` (in place,
    any device); a parameter without state gets zeros. Returns (step, lr): the step count of the state (None when it has
    none) and param_groups[0]['lr'] (None when absent)."""
    state = sd.get("state", {})
    groups = sd.get("param_groups", [])
    ids = groups[0]["params"] if groups else list(range(len(layout)))
    if len(ids) != len(layout):
        raise ValueError("optimizer state covers %d parameters, the model has %d trainable ones" % (len(ids), len(layout)))
    step = None
    for name, buf in flat.items():
        host = torch.zeros(buf.numel(), dtype=torch.float32)
        for pid, (off, shape) in zip(ids, layout):
            st = state.get(pid, state.get(str(pid)))
            if st is None or st.get(name) is None:
                continue
            t = st[name].detach().to("cpu", torch.float32).reshape(-1)
            n = 1
            for s in shape:
                n *= int(s)
            if t.numel() != n:
                raise ValueError("state %r of parameter %s has %d elements, expected %d" % (name, pid, t.numel(), n))
            host[off:off + n] = t
        buf.copy_(host.to(buf.device))
    for pid in ids:
        st = state.get(pid, state.get(str(pid)))
        if st is not None and "step" in st:
            step = float(st["step"])
            break
    lr = float(groups[0]["lr"]) if groups and "lr" in groups[0] else None
    return step, lr
