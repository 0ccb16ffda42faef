"""Host side of the weight EMA (TrainStep(ema_decay=...)): the restated recurrence of pytorch_nested-unet_amd/ema.py against
torch.optim.swa_utils.AveragedModel, the warm-up closed form, the state-dict format, and the argument checks of the new C
entries that need no device (they refuse before the first launch)."""
import ctypes as C
import importlib
import os

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import nunet_amd
from nunet_amd import _lib as L

EMA = importlib.import_module("pytorch_nested-unet_amd.ema")
EINVAL = -1


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(2, 3, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(3)

    def forward(self, x):
        return self.bn(self.conv(x))


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.999])
def test_recurrence_equals_averaged_model(decay):
    """Five SGD steps of a tiny fp64 conv + BatchNorm module, AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay),
    use_buffers=True).update_parameters after each: the restated recurrence over parameters and running statistics equals
    it - the first update a bit-exact copy, n_averaged alike. Both sides run in fp64, where torch's lerp (two formulas, split at
    weight 0.5) and e + w (p - e) differ by a few 2^-53 relative per update; w itself is the fp32-rounded weight in the
    restatement and the double 1 - decay in torch: |w32 - w| <= 2^-25 per update times a difference of at most 2 M. Bound:
    T (2^-24 + 8 * 2^-53) M with M = max |value|."""
    torch.manual_seed(3)
    m = _Tiny().double().train()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
    rec = EMA.Recurrence(decay)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    tracked = lambda mod: [mod.conv.weight, mod.conv.bias, mod.bn.weight, mod.bn.bias, mod.bn.running_mean, mod.bn.running_var]
    T = 5
    for k in range(T):
        opt.zero_grad()
        m(torch.randn(4, 2, 5, 5, dtype=torch.float64)).square().mean().backward()
        opt.step()
        avg.update_parameters(m)
        rec.update(tracked(m))
        assert int(avg.n_averaged) == rec.n_averaged == k + 1
        big = max(float(v.abs().max()) for v in rec.values)
        for a, b in zip(tracked(avg.module), rec.values):
            if k == 0:
                assert torch.equal(a.detach(), b)
            assert float((a.detach() - b).abs().max()) <= (k + 1) * (2.0 ** -24 + 8 * 2.0 ** -53) * big
    assert rec.w == torch.tensor(1.0 - decay, dtype=torch.float64).float().item()
    # torch's integer branch: the counter is NOT an average worth keeping (the live model's value is what ema_state_dict carries)
    assert int(m.bn.num_batches_tracked) == T


def test_warmup_closed_form():
    """weight(decay, warmup, n): 1 for the first update; then float(1 - min(decay, (1 + n) / (10 + n))), the difference formed
    in double. The warm-up decay rises monotonically and hands over to `decay` at n = (10 decay - 1) / (1 - decay)."""
    d = 0.999
    assert EMA.weight(d, True, 0) == EMA.weight(d, False, 0) == 1.0
    prev = 0.0
    for n in range(1, 20000, 7):
        dt = EMA.decay_at(d, True, n)
        assert dt == min(d, (1.0 + n) / (10.0 + n)) and dt >= prev
        prev = dt
        w = EMA.weight(d, True, n)
        assert w == torch.tensor(1.0 - dt, dtype=torch.float64).to(torch.float32).item()
        assert (dt == d) == (n >= (10 * d - 1) / (1 - d))
        assert EMA.weight(d, False, n) == torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32).item()
    assert EMA.weight(0.9, True, 1) == torch.tensor(1.0 - 2.0 / 11.0, dtype=torch.float64).float().item()
    assert EMA.weight(0.9, True, 200) == torch.tensor(1.0 - 0.9, dtype=torch.float64).float().item()


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), "x"])
def test_decay_outside_the_unit_interval_is_refused(bad):
    with pytest.raises(L.NunetError):
        EMA.check_decay(bad)
    with pytest.raises(L.NunetError):
        EMA.Recurrence(bad)


def test_decay_in_range_is_taken():
    for ok in (0, 0.0, 0.5, 0.9999, 1.0 - 2.0 ** -40):
        assert EMA.check_decay(ok) == float(ok)


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """No device needed: every refusal comes before the first launch. A decay outside [0, 1), a null or misaligned state, an
    ema without ema_params (and the reverse), and the flat Adam entry with an ema."""
    lib = L.lib()
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    for bad in (-0.5, 1.0, 2.0, float("nan")):
        assert lib.nunet_ema_init(C.c_void_p(a), bad, 0, 0, None) == EINVAL
        assert b"decay" in lib.nunet_last_error()
    assert lib.nunet_ema_init(None, 0.9, 0, 0, None) == EINVAL
    assert lib.nunet_ema_init(C.c_void_p(a + 4), 0.9, 0, 0, None) == EINVAL
    assert lib.nunet_ema_init(C.c_void_p(a), 0.9, 0, -1, None) == EINVAL and b"n_averaged" in lib.nunet_last_error()
    assert lib.nunet_ema_prepare(None, None, None) == EINVAL
    assert lib.nunet_ema_prepare(C.c_void_p(a + 4), None, None) == EINVAL
    assert lib.nunet_ema_lerp(None, C.c_void_p(a), 4, C.c_void_p(a + 64), None) == EINVAL
    assert lib.nunet_ema_lerp(C.c_void_p(a), C.c_void_p(a + 32), 0, C.c_void_p(a + 64), None) == EINVAL
    assert lib.nunet_ema_lerp(C.c_void_p(a), C.c_void_p(a + 32), 4, None, None) == EINVAL
    assert lib.nunet_ema_lerp(C.c_void_p(a + 2), C.c_void_p(a + 32), 4, C.c_void_p(a + 64), None) == EINVAL
    for kind in (L.OPT_SGD, L.OPT_ADAM):
        o = L.Optim(kind=kind, momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, nesterov=0, lr=a, adam_scal=a + 8,
                    state0=a + 16, state1=a + 32)
        o.ema = a + 64                                   # an ema, no ema_params
        assert lib.nunet_opt_step(C.c_void_p(a + 96), C.c_void_p(a + 112), C.byref(o), 2, 1.0, None) == EINVAL
        assert b"ema_params" in lib.nunet_last_error()
        assert lib.nunet_plan_opt_step(None, None, C.byref(o), None, 0, 1.0, None, None) == EINVAL
        o.ema, o.ema_params = None, a + 48               # ema_params, no ema
        assert lib.nunet_opt_step(C.c_void_p(a + 96), C.c_void_p(a + 112), C.byref(o), 2, 1.0, None) == EINVAL
        assert b"ema_params" in lib.nunet_last_error()
    o = L.Optim(kind=L.OPT_ADAM, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, nesterov=0, lr=a, adam_scal=a + 8,
                state0=a + 16, state1=a + 32, ema=a + 64, ema_params=a + 48)
    assert lib.nunet_adam_step(C.c_void_p(a + 96), C.c_void_p(a + 112), C.byref(o), 2, 1.0, None) == EINVAL
    assert b"EMA" in lib.nunet_last_error()


def test_struct_sizes_match_the_header():
    """nunet_ema is 32 bytes (EMA_WORDS int32 words); nunet_optim grew by two pointers, behind the state pointers (scaler and
    clip stay its trailing pair, which tests/test_clip_cpu.py pins), at the offsets the header's field order gives."""
    assert L.EMA_WORDS * 4 == 32
    names = [f[0] for f in L.Optim._fields_]
    assert names[-6:] == ["state0", "state1", "ema", "ema_params", "scaler", "clip"]
    assert L.Optim.ema.offset == L.Optim.state1.offset + 8 and L.Optim.ema_params.offset == L.Optim.ema.offset + 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nunet.h")).read()
    body = hdr[hdr.index("typedef struct {\n  int32_t kind;"):hdr.index("} nunet_optim;")]
    order = [body.index(k) for k in ("state1;", "nunet_ema* ema;", "float* ema_params;", "nunet_scaler* scaler;", "nunet_clip* clip;")]
    assert order == sorted(order)
    assert C.sizeof(L.Optim) == 40 + 8 * 8               # 40 bytes of hyper-parameters, then eight pointers
    assert (L.EMA_SKIP, L.EMA_LERP, L.EMA_COPY) == (0, 1, 2)


@pytest.mark.parametrize("arch,ds", [("NestedUNet", False), ("NestedUNet", True), ("UNet", False)])
def test_state_dict_key_parity(arch, ds):
    """ema.state_dict_from_flat over CPU stand-ins of the engine's arenas: model.state_dict()'s keys in order, shapes and
    dtypes; parameters and running statistics from the flat arenas, num_batches_tracked the live model's; and back."""
    torch.manual_seed(5)
    m = getattr(nunet_amd.archs, arch)(2, 3, ds)

    class Eng:
        pass
    eng = Eng()
    eng.module_params = list(m.parameters())
    eng.param_names = [k for k, _ in m.named_parameters()]
    eng.param_off, off = [], 0
    for p in eng.module_params:
        eng.param_off.append(off)
        off += p.numel()
    nb = sum(2 * b.num_features for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    flat, bnbuf = torch.randn(off), torch.rand(nb) + 0.5
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.num_batches_tracked.fill_(7)
    ref = m.state_dict()
    sd = EMA.state_dict_from_flat(m, eng, flat, bnbuf)
    assert list(sd.keys()) == list(ref.keys())
    np_, nb_ = 0, 0
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 7
        elif k.endswith("running_mean") or k.endswith("running_var"):
            nb_ += v.numel()
        else:
            np_ += v.numel()
    assert (np_, nb_) == (off, nb)
    # parameters in parameters() order, running statistics in module order: mean then var
    assert torch.equal(torch.cat([sd[k].reshape(-1) for k in eng.param_names]), flat)
    assert torch.equal(torch.cat([sd[k] for k in ref if k.endswith("running_mean") or k.endswith("running_var")]), bnbuf)
    flat2, bn2 = torch.zeros(off), torch.zeros(nb)
    EMA.flat_from_state_dict(m, eng, sd, flat2, bn2)
    assert torch.equal(flat2, flat) and torch.equal(bn2, bnbuf)
    m2 = getattr(nunet_amd.archs, arch)(2, 3, ds)
    m2.load_state_dict(sd)                               # a stock module takes it
    bad = dict(sd)
    del bad[eng.param_names[0]]
    with pytest.raises(L.NunetError):
        EMA.flat_from_state_dict(m, eng, bad, flat2, bn2)
