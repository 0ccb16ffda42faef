"""Weight EMA inside the fused step on the MI355X (TrainStep(ema_decay=...), EvalStep(weights=...)): the flat entries against
the fp64 recurrence, the fused update in both layouts against a twin step without an EMA (bit for bit) and the recurrence on
the device's own parameter trajectory, captured against eager, fp16 steps skipped by loss scaling, validation of the averaged
weights, the state-dict round trip, and train.py --ema_decay / val.py --ema end to end.

Tolerance: an update is three fp32 roundings (p' - ema, * w, + ema) with w <= 1, so its absolute error is at most
5 * 2^-24 * M, with M a bound of |p| and |ema| over the run; earlier error is carried with a factor 1 - w <= 1. After T updates
the device's average lies within 5 * T * 2^-24 * M of the fp64 recurrence run on the parameters read back after each step
with the same fp32-rounded w. The first update is a bit-exact copy."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.trainer import EvalStep, TrainStep  # noqa: E402

EMA = importlib.import_module("pytorch_nested-unet_amd.ema")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor, chosen without timing
EPS = 2.0 ** -24


def _bound(T, big):
    return 5.0 * T * EPS * big


def _module(st, ncls=1, dtype="fp32", cin=3, ds=False, arch="NestedUNet"):
    m = getattr(nunet_amd.archs, arch)(ncls, cin, ds, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v.clone() for k, v in st.items()})
    return m.to(DEV).train()


def _batches(synth, n, hw, ncls, seeds, cin=3):
    out = []
    for s in seeds:
        img, msk = synth.synth_batch(n, hw, hw, cin, ncls, seed=s)
        out.append((torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)))
    return out


def _state(ts):
    eng = ts.eng
    return [t.detach().clone() for t in [eng.flat_params, eng.bnbuf, eng.nbt, ts.meters, eng.flat_grads] + ts.opt_state]


def _ema_state(ts):
    return [ts.ema_params.detach().clone(), ts.ema_bnbuf.detach().clone(), ts._ema.detach().clone()]


def _words(t):
    """(decay, warmup, n_averaged, w, live) of a nunet_ema tensor"""
    torch.cuda.synchronize()
    w = t.cpu()
    return float(w[0:2].view(torch.float64)), int(w[2]), int(w[3]), float(w[4:5].view(torch.float32)), int(w[5])


def _new_ema(decay, warmup, n_averaged=0):
    e = torch.zeros(L.EMA_WORDS, dtype=torch.int32, device=DEV)
    L.check(L.lib().nunet_ema_init(L.ptr(e), decay, int(warmup), n_averaged, L.stream()), "ema_init")
    return e


def _check_against_recurrence(what, T, dev_vals, rec_vals, hist_max):
    """|device average - fp64 recurrence| <= 5 T 2^-24 M elementwise; M over the trajectory and both averages"""
    big = max(hist_max, float(dev_vals.abs().max()), float(rec_vals.abs().max()))
    err = float((dev_vals.double().cpu() - rec_vals).abs().max())
    print("%s: T %d, max |ema - fp64 recurrence| %.3e, bound %.3e (M %.4g)" % (what, T, err, _bound(T, big), big))
    assert err <= _bound(T, big), (what, err, _bound(T, big))


# -- 1. flat entries -------------------------------------------------------------------------------------------------------------
def test_prepare_forms_the_warmup_weights_and_honours_found_inf():
    """nunet_ema_prepare from n_averaged = 0 .. 12 with warm-up (decay 0.999): mode COPY and w = 1 first, then mode LERP and
    w = float(1 - min(decay, (1 + n) / (10 + n))) - the closed form of ema.weight, bit for bit - and n_averaged + 1 each time.
    With the scaler's found_inf set: mode SKIP, n_averaged and w untouched. Without warm-up: float(1 - decay) for every n >= 1."""
    lib, st = L.lib(), L.stream()
    e = _new_ema(0.999, True)
    assert _words(e) == (0.999, 1, 0, 0.0, L.EMA_SKIP)
    for n in range(13):
        L.check(lib.nunet_ema_prepare(L.ptr(e), None, st), "ema_prepare")
        d, wu, na, w, live = _words(e)
        assert (d, wu, na) == (0.999, 1, n + 1)
        assert w == EMA.weight(0.999, True, n), (n, w, EMA.weight(0.999, True, n))
        assert live == (L.EMA_COPY if n == 0 else L.EMA_LERP)
    scaler = torch.zeros(L.SCALER_WORDS, dtype=torch.int32, device=DEV)
    scaler[3] = 1                                    # found_inf
    before = _words(e)
    L.check(lib.nunet_ema_prepare(L.ptr(e), L.ptr(scaler), st), "ema_prepare")
    assert _words(e) == before[:4] + (L.EMA_SKIP,)
    scaler[3] = 0
    L.check(lib.nunet_ema_prepare(L.ptr(e), L.ptr(scaler), st), "ema_prepare")
    assert _words(e) == (0.999, 1, 14, EMA.weight(0.999, True, 13), L.EMA_LERP)
    e = _new_ema(0.9, False, n_averaged=5)
    L.check(lib.nunet_ema_prepare(L.ptr(e), None, st), "ema_prepare")
    assert _words(e) == (0.9, 0, 6, EMA.weight(0.9, False, 5), L.EMA_LERP)
    assert EMA.weight(0.9, False, 5) == float(torch.tensor(1.0 - 0.9, dtype=torch.float64).float())


@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1025, 4099])
def test_flat_step_with_ema(n, offset, optimizer, guard_bands):
    """nunet_opt_step with an ema over n values, every pointer 16-byte aligned (offset 0) or one float past it (scalar path),
    three steps with warm-up (decay 0.9): p and the optimiser state are bit-identical to the same calls without an ema; the
    first update leaves ema == p bit for bit (from a different start); after each later one ema is within the bound of the fp64
    recurrence on the p read back; a step with found_inf set writes nothing."""
    lib, st = L.lib(), L.stream()
    gen = torch.Generator(device=DEV).manual_seed(77 + n)
    ns = 1 if optimizer == "SGD" else 2

    def bufs(k):
        out = []
        for _ in range(k):
            b = torch.zeros(n + offset, dtype=torch.float32, device=DEV)
            out.append(b[offset:])
            assert out[-1].data_ptr() % 16 == 4 * offset
        return out

    p0 = torch.randn(n, device=DEV, generator=gen)
    s0 = [torch.randn(n, device=DEV, generator=gen).abs() * 0.01 for _ in range(ns)]
    grads = [torch.randn(n, device=DEV, generator=gen) for _ in range(3)]
    lr = torch.full((1,), 0.05, dtype=torch.float32, device=DEV)
    scal = torch.tensor([0.05, 1.0], dtype=torch.float32, device=DEV)
    runs = {}
    for with_ema in (False, True):
        p, g, a, b, ema = bufs(5)
        p.copy_(p0)
        a.copy_(s0[0])
        if ns == 2:
            b.copy_(s0[1])
        ema.fill_(123.0)
        if optimizer == "SGD":
            o = L.Optim(kind=L.OPT_SGD, momentum=0.9, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=1e-2, nesterov=1, lr=L.ptr(lr).value,
                        state0=L.ptr(a).value)
        else:
            o = L.Optim(kind=L.OPT_ADAM, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, nesterov=0, lr=L.ptr(lr).value,
                        adam_scal=L.ptr(scal).value, state0=L.ptr(a).value, state1=L.ptr(b).value)
        words = _new_ema(0.9, True)
        if with_ema:
            o.ema, o.ema_params = L.ptr(words).value, L.ptr(ema).value
        rec = EMA.Recurrence(0.9, True)
        hist = 0.0
        traj = []
        for k, gk in enumerate(grads):
            g.copy_(gk)
            if with_ema:
                L.check(lib.nunet_ema_prepare(L.ptr(words), None, st), "ema_prepare")
            L.check(lib.nunet_opt_step(L.ptr(p), L.ptr(g), C_byref(o), n, 0.5, st), "opt_step")
            torch.cuda.synchronize()
            traj.append([p.clone(), a.clone(), b.clone()])
            if with_ema:
                rec.update([p])
                hist = max(hist, float(p.abs().max()))
                assert _words(words)[2:] == (k + 1, rec.w, L.EMA_COPY if k == 0 else L.EMA_LERP)
                if k == 0:
                    assert torch.equal(ema, p)
                _check_against_recurrence("flat %s n %d offset %d step %d" % (optimizer, n, offset, k), k + 1, ema, rec.values[0], hist)
        if with_ema:
            # a step skipped by loss scaling: nothing is written, the average and n_averaged included
            scaler = torch.zeros(L.SCALER_WORDS, dtype=torch.int32, device=DEV)
            scaler[0:2] = torch.tensor([1.0, 1.0], dtype=torch.float32).view(torch.int32).to(DEV)
            scaler[3] = 1
            o.scaler = L.ptr(scaler).value
            before = [p.clone(), a.clone(), b.clone(), ema.clone()]
            L.check(lib.nunet_ema_prepare(L.ptr(words), L.ptr(scaler), st), "ema_prepare")
            L.check(lib.nunet_opt_step(L.ptr(p), L.ptr(g), C_byref(o), n, 0.5, st), "opt_step")
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(before, [p, a, b, ema]))
            assert _words(words)[2:] == (3, rec.w, L.EMA_SKIP)
        else:
            assert bool((ema == 123.0).all())
        runs[with_ema] = traj
    for k in range(3):
        for u, v in zip(runs[False][k], runs[True][k]):
            assert torch.equal(u, v), (k, "p / optimiser state differ from the step without an ema")
    assert not torch.equal(runs[True][0][0], p0)


def C_byref(o):
    import ctypes
    return ctypes.byref(o)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (0, 1), (3, 2)])
@pytest.mark.parametrize("n", [1, 3, 255, 1025, 4099])
def test_ema_lerp(n, offsets, guard_bands):
    """nunet_ema_lerp over n values, the two pointers congruent modulo 16 bytes (16-byte middle, scalar head / tail) or not (all
    scalars): the copy is exact, a lerp is within one update's bound of fp64, mode SKIP writes nothing, src is never written."""
    lib, st = L.lib(), L.stream()
    gen = torch.Generator(device=DEV).manual_seed(5 + n)
    eo, so = offsets
    ema = torch.zeros(n + eo, dtype=torch.float32, device=DEV)[eo:]
    src = torch.zeros(n + so, dtype=torch.float32, device=DEV)[so:]
    assert ema.data_ptr() % 16 == 4 * eo and src.data_ptr() % 16 == 4 * so
    vals = torch.randn(n, device=DEV, generator=gen)
    src.copy_(vals)
    ema.fill_(-7.0)
    words = _new_ema(0.75, False)
    L.check(lib.nunet_ema_lerp(L.ptr(ema), L.ptr(src), n, L.ptr(words), st), "ema_lerp")       # mode SKIP (no prepare yet)
    torch.cuda.synchronize()
    assert bool((ema == -7.0).all())
    L.check(lib.nunet_ema_prepare(L.ptr(words), None, st), "ema_prepare")
    L.check(lib.nunet_ema_lerp(L.ptr(ema), L.ptr(src), n, L.ptr(words), st), "ema_lerp")       # the copy
    torch.cuda.synchronize()
    assert torch.equal(ema, vals)
    nxt = torch.randn(n, device=DEV, generator=gen) * 3.0
    src.copy_(nxt)
    L.check(lib.nunet_ema_prepare(L.ptr(words), None, st), "ema_prepare")
    L.check(lib.nunet_ema_lerp(L.ptr(ema), L.ptr(src), n, L.ptr(words), st), "ema_lerp")
    w = _words(words)[3]
    assert w == 0.25
    want = vals.double().cpu() + w * (nxt.double().cpu() - vals.double().cpu())
    _check_against_recurrence("lerp n %d offsets %s" % (n, offsets), 1, ema, want, float(max(vals.abs().max(), nxt.abs().max())))
    assert torch.equal(src, nxt)


# -- 2. the fused step -------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "nested_k1_c3": dict(ncls=1, cin=3, ds=False, arch="NestedUNet"),       # first layer cin = 3: the scalar tile path
    "nested_k3_c4": dict(ncls=3, cin=4, ds=False, arch="NestedUNet"),       # cin = 4: the first layer takes the aligned path
    "nested_ds_k1_c4": dict(ncls=1, cin=4, ds=True, arch="NestedUNet"),     # four heads
    "nested_ds_k3_c3": dict(ncls=3, cin=3, ds=True, arch="NestedUNet"),
    "unet_k1_c4": dict(ncls=1, cin=4, ds=False, arch="UNet"),
    "unet_k3_c3": dict(ncls=3, cin=3, ds=False, arch="UNet"),
}


def _closed_form(synth, c):
    if c["arch"] == "UNet":
        return synth.closed_form_state_unet(c["ncls"], c["cin"])
    return synth.closed_form_state(c["ncls"], c["cin"], c["ds"], True)


def _run_with_twin(synth, c, hw, kw, ema_kw, T=4, seeds=(301, 302, 303, 304)):
    """T eager steps of a TrainStep with an EMA beside a twin without: everything the twin owns is bit-identical after every
    step; the averages are within the bound of the recurrence on the parameters / BatchNorm buffers read back."""
    st = _closed_form(synth, c)
    data = _batches(synth, 2, hw, c["ncls"], seeds[:T], cin=c["cin"])
    shape = (2, c["cin"], hw, hw)
    m, mt = (_module(st, c["ncls"], "fp32", c["cin"], c["ds"], c["arch"]) for _ in range(2))
    ts = TrainStep(m, shape, use_graph=False, **kw, **ema_kw)
    twin = TrainStep(mt, shape, use_graph=False, **kw)
    assert twin.ema_stats() is None and ts.ema_stats() == dict(n_averaged=0, w=0.0)
    assert torch.equal(ts.ema_params, ts.eng.flat_params) and torch.equal(ts.ema_bnbuf, ts.eng.bnbuf)
    assert ts.ema_params.data_ptr() != ts.eng.flat_params.data_ptr()
    rec = EMA.Recurrence(ema_kw["ema_decay"], ema_kw.get("ema_warmup", False))
    hist = [0.0, 0.0]
    for k, (x, t) in enumerate(data):
        ts.step(x, t)
        twin.step(x, t)
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(_state(ts), _state(twin))):
            assert torch.equal(a, b), (k, j, "differs from the twin without an EMA")
        for p, pt in zip(m.parameters(), mt.parameters()):
            assert torch.equal(p.grad, pt.grad)
        rec.update([ts.eng.flat_params, ts.eng.bnbuf])
        hist = [max(hist[0], float(ts.eng.flat_params.abs().max())), max(hist[1], float(ts.eng.bnbuf.abs().max()))]
        assert ts.ema_stats() == dict(n_averaged=k + 1, w=rec.w)
        if k == 0:
            assert torch.equal(ts.ema_params, ts.eng.flat_params) and torch.equal(ts.ema_bnbuf, ts.eng.bnbuf)
    assert float((ts.eng.flat_params - ts.ema_params).abs().max()) > 0          # the parameters moved away from their average
    _check_against_recurrence("ema_params", T, ts.ema_params, rec.values[0], hist[0])
    _check_against_recurrence("ema_bnbuf", T, ts.ema_bnbuf, rec.values[1], hist[1])
    return ts, twin


@pytest.mark.parametrize("fused_update", [0, 2])
@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fused_step_with_ema(synth, config, optimizer, fused_update):
    """2x16x16 fp32, T = 4 eager steps, decay 0.9 (warm-up for the deep-supervision models): parameters, optimiser state, BN
    buffers, meters and p.grad bit-identical to the twin; EMA and EMA-BN within the bound; n_averaged == 4."""
    c = CONFIGS[config]
    kw = dict(lr=1e-2, optimizer=optimizer, weight_decay=1e-4, fused_update=fused_update)
    ts, twin = _run_with_twin(synth, c, 16, kw, dict(ema_decay=0.9, ema_warmup=c["ds"]))
    assert ts.ema_stats()["n_averaged"] == 4
    sd, ref = ts.ema_state_dict(), ts.model.state_dict()
    assert list(sd) == list(ref) and all(sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype for k in ref)


@pytest.mark.parametrize("fused_update", [0, 2])
def test_fused_step_with_ema_and_a_binding_clip(synth, fused_update):
    """clip_grad_norm = 1e-3, far below the gradient norm: every step is clipped; the average follows the parameter the clipped
    update stores, and the twin (same clip, no EMA) is bit-identical."""
    kw = dict(lr=1e-2, optimizer="SGD", weight_decay=1e-4, fused_update=fused_update, clip_grad_norm=1e-3)
    ts, twin = _run_with_twin(synth, CONFIGS["nested_k1_c3"], 32, kw, dict(ema_decay=0.99))
    s = ts.grad_norm_stats()
    assert (s["clipped"], s["steps"]) == (4, 4) and s == twin.grad_norm_stats()


def test_bad_arguments_raise(synth):
    st = _closed_form(synth, CONFIGS["nested_k1_c3"])
    m = _module(st)
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(L.NunetError):
            TrainStep(m, (2, 3, 16, 16), use_graph=False, ema_decay=bad)
    ts = TrainStep(m, (2, 3, 16, 16), use_graph=False)
    for call in (ts.ema_state_dict, lambda: ts.load_ema_state_dict({})):
        with pytest.raises(L.NunetError):
            call()
    n = ts.eng.flat_params.numel()
    with pytest.raises(L.NunetError):
        EvalStep(m, (2, 3, 16, 16), weights=(torch.zeros(n - 1, device=DEV), ts.eng.bnbuf.clone()))
    with pytest.raises(L.NunetError):
        EvalStep(m, (2, 3, 16, 16), weights=(ts.eng.flat_params.clone(), torch.zeros(3, device=DEV)))
    with pytest.raises(L.NunetError):
        EvalStep(m, (2, 3, 16, 16), weights=(torch.zeros(n), ts.eng.bnbuf.clone()))
    with pytest.raises(L.NunetError):
        EvalStep(m, (2, 3, 16, 16), weights=ts.eng.flat_params)


# -- 3. captured vs eager ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer,fused_update", [("SGD", 2), ("Adam", 0)])
def test_captured_equals_eager(synth, optimizer, fused_update):
    """The one-hipGraph step with an EMA: capture() leaves the averages and n_averaged untouched, three replays equal three
    eager steps bit for bit (average included), and the graph holds exactly two kernel nodes more than without an EMA (the
    one-thread bookkeeping and the BatchNorm lerp)."""
    c = CONFIGS["nested_k1_c3"]
    st = _closed_form(synth, c)
    data = _batches(synth, 2, 32, 1, [41, 42, 43])
    kw = dict(lr=1e-2, optimizer=optimizer, fused_update=fused_update)
    m = _module(st)
    ts = TrainStep(m, (2, 3, 32, 32), ema_decay=0.9, ema_warmup=True, **kw, **GRAPH)
    before = _ema_state(ts) + _state(ts)[:4]
    ts.capture(*data[0])
    torch.cuda.synchronize()
    print("executor_choice", ts.executor_choice)
    assert ts.g_fb is not None
    for a, b in zip(before, _ema_state(ts) + _state(ts)[:4]):
        assert torch.equal(a, b), "capture() left a trace"
    assert ts.ema_stats() == dict(n_averaged=0, w=0.0)
    me = _module(st)
    eager = TrainStep(me, (2, 3, 32, 32), use_graph=False, ema_decay=0.9, ema_warmup=True, **kw)
    for x, t in data:
        ts.step(x, t)
        eager.step(x, t)
        torch.cuda.synchronize()
        for a, b in zip(_state(ts) + _ema_state(ts)[:2], _state(eager) + _ema_state(eager)[:2]):
            assert torch.equal(a, b)
        assert ts.ema_stats() == eager.ema_stats()
    assert ts.ema_stats()["n_averaged"] == 3
    mo = _module(st)
    off = TrainStep(mo, (2, 3, 32, 32), **kw, **GRAPH)
    off.capture(*data[0])
    n_on, n_off = ts.g_fb.info()["nodes"], off.g_fb.info()["nodes"]
    print("graph nodes with / without EMA: %d / %d" % (n_on, n_off))
    assert n_on == n_off + 2


# -- 4. fp16 with loss scaling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer,fused_update", [("SGD", 2), ("Adam", 0)])
def test_skipped_steps_leave_the_average(synth, optimizer, fused_update):
    """fp16, init_scale 2^40: the first steps overflow and are skipped - the averages, n_averaged and w stay bit-unchanged
    (mode SKIP) while the scale backs off; the first clean step performs the copy (n_averaged 1), the next one a lerp."""
    st = _closed_form(synth, CONFIGS["nested_k1_c3"])
    (x, t), = _batches(synth, 2, 32, 1, [51])
    m = _module(st, 1, "fp16")
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-3, optimizer=optimizer, fused_update=fused_update, use_graph=False,
                   loss_scale=dict(init_scale=2.0 ** 40), ema_decay=0.9)
    ts.ema_params.add_(1.0)                          # (so that an unwanted copy would show)
    start = _ema_state(ts)
    skipped = 0
    for k in range(40):
        ts.step(x, t)
        sk = ts.scaler_stats()[1]
        if sk == skipped:
            break
        skipped = sk
        now = _ema_state(ts)
        assert torch.equal(now[0], start[0]) and torch.equal(now[1], start[1]), k
        assert _words(ts._ema) == (0.9, 0, 0, 0.0, L.EMA_SKIP)
    print("%d steps skipped before the first clean one" % skipped)
    assert skipped >= 1 and ts.scaler_stats()[1] == skipped
    assert _words(ts._ema) == (0.9, 0, 1, 1.0, L.EMA_COPY)
    assert torch.equal(ts.ema_params, ts.eng.flat_params) and torch.equal(ts.ema_bnbuf, ts.eng.bnbuf)
    copied = _ema_state(ts)
    ts._write_scaler(ts.scaler_stats()[0] / 4.0, 0, skipped)      # (headroom: the next step must not overflow again)
    ts.step(x, t)
    assert ts.scaler_stats()[1] == skipped
    assert ts.ema_stats() == dict(n_averaged=2, w=EMA.weight(0.9, False, 1))
    want = copied[0].double().cpu() + ts.ema_stats()["w"] * (ts.eng.flat_params.double().cpu() - copied[0].double().cpu())
    _check_against_recurrence("lerp behind the copy", 1, ts.ema_params, want,
                              float(max(copied[0].abs().max(), ts.eng.flat_params.abs().max())))
    # a later overflow: the mode word says SKIP, everything else stays
    ts._write_scaler(2.0 ** 40, 0, skipped)
    before = _ema_state(ts)
    ts.step(x, t)
    assert ts.scaler_stats()[1] == skipped + 1
    now = _ema_state(ts)
    assert torch.equal(now[0], before[0]) and torch.equal(now[1], before[1])
    assert _words(ts._ema) == (0.9, 0, 2, EMA.weight(0.9, False, 1), L.EMA_SKIP)


# -- 5. EvalStep on the averaged weights ---------------------------------------------------------------------------------------------
def _same(a, b):
    """== over the nested result of EvalStep.result(), with NaN equal to NaN (a class nobody predicted has no precision)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and a != a:
        return b != b
    return a == b


def test_eval_step_on_the_averaged_weights(synth):
    """A deep-supervision NestedUNet after three SGD steps at lr 0.05: EvalStep(weights=(ts.ema_params, ts.ema_bnbuf)) returns
    loss and iou bit-equal to an EvalStep on a second model loaded from ts.ema_state_dict() - plain, pruned to depth 2 and per
    head - and not the live model's."""
    c = CONFIGS["nested_ds_k1_c4"]
    st = _closed_form(synth, c)
    data = _batches(synth, 2, 32, 1, [61, 62, 63], cin=4)
    m = _module(st, 1, "fp32", 4, True)
    shape = (2, 4, 32, 32)
    with torch.no_grad():                            # centre every head's logits, so that the IoU compared below is not that of an empty prediction
        outs = m.eval()(data[0][0])
        for head, o in zip((m.final1, m.final2, m.final3, m.final4), outs):
            head.bias.sub_(o.median())
    m.train()
    ts = TrainStep(m, shape, lr=0.05, use_graph=False, ema_decay=0.9)
    for x, t in data:
        ts.step(x, t)
    img, msk = synth.synth_batch(5, 32, 32, 4, 1, seed=64)              # two full batches and a tail of one
    vx, vt = torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV)
    sd = ts.ema_state_dict()
    m2 = _module(sd, 1, "fp32", 4, True)
    w = (ts.ema_params, ts.ema_bnbuf)
    live = EvalStep(m, shape).evaluate(vx, vt)
    for kw in (dict(), dict(depth=2), dict(per_head=True)):
        a = EvalStep(m, shape, weights=w, **kw).evaluate(vx, vt)
        b = EvalStep(m2, shape, **kw).evaluate(vx, vt)
        print(kw, "ema loss %.9g iou %.9g; live loss %.9g iou %.9g" % (a["loss"], a["iou"], live["loss"], live["iou"]))
        assert _same(a, b), (kw, a, b)
        assert a["loss"] == b["loss"] and a["iou"] == b["iou"] and a["samples"] == 5
    plain = EvalStep(m, shape, weights=w).evaluate(vx, vt)
    assert plain["loss"] != live["loss"] and (plain["loss"], plain["iou"]) != (live["loss"], live["iou"])
    for k, v in m.state_dict().items():              # the live module was not touched; its counters are the EMA dict's
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 3
    first = ts.eng.param_names[0]
    assert torch.equal(sd[first].reshape(-1), ts.ema_params[:sd[first].numel()])


# -- 6. state-dict round trip --------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip(synth):
    """Two steps, ema_state_dict + model / optimiser state into a fresh TrainStep (load_ema_state_dict with n_averaged), two
    more steps: parameters, averages and n_averaged equal the uninterrupted four steps bit for bit (warm-up on, so a wrong
    n_averaged would change w)."""
    c = CONFIGS["nested_k1_c3"]
    st = _closed_form(synth, c)
    data = _batches(synth, 2, 16, 1, [71, 72, 73, 74])
    kw = dict(lr=1e-2, use_graph=False, ema_decay=0.9, ema_warmup=True)
    ma = _module(st)
    a = TrainStep(ma, (2, 3, 16, 16), **kw)
    for x, t in data:
        a.step(x, t)
    mb = _module(st)
    b = TrainStep(mb, (2, 3, 16, 16), **kw)
    for x, t in data[:2]:
        b.step(x, t)
    saved = dict(model={k: v.detach().cpu().clone() for k, v in mb.state_dict().items()}, opt=b.optimizer_state_dict(),
                 ema={k: v.cpu() for k, v in b.ema_state_dict().items()}, n=b.ema_stats()["n_averaged"])
    assert saved["n"] == 2
    del b, mb
    mc = _module(saved["model"])
    cst = TrainStep(mc, (2, 3, 16, 16), **kw)
    cst.load_optimizer_state_dict(saved["opt"])
    cst.load_ema_state_dict(saved["ema"], n_averaged=saved["n"])
    assert cst.ema_stats()["n_averaged"] == 2
    for x, t in data[2:]:
        cst.step(x, t)
    torch.cuda.synchronize()
    assert torch.equal(cst.eng.flat_params, a.eng.flat_params) and torch.equal(cst.eng.bnbuf, a.eng.bnbuf)
    assert torch.equal(cst.ema_params, a.ema_params) and torch.equal(cst.ema_bnbuf, a.ema_bnbuf)
    assert cst.ema_stats() == a.ema_stats() == dict(n_averaged=4, w=EMA.weight(0.9, True, 3))


# -- 7. train.py / val.py ------------------------------------------------------------------------------------------------------------
def test_train_py_and_val_py_with_ema(tmp_path):
    """train.py --ema_decay 0.9 --ema_warmup true, 2 epochs of 4 steps at 2x32x32: ema_val_loss / ema_val_iou on the epoch line
    and as the last log.csv columns, model_ema.pth saved; val.py --ema true --no_images prints the IoU logged for the saved
    epoch (the best ema_val_iou); without the file it says what is missing."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--ema_decay", "0.9", "--ema_warmup", "true", "--epochs", "2", "--train_size", "8",
           "--val_size", "4", "--batch_size", "2", "--input_h", "32", "--input_w", "32", "--name", "ema_e2e"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "weight EMA 0.9 with warm-up" in r.stdout, r.stdout[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch [")]
    assert len(lines) == 2 and all(" - ema_val_loss " in ln and " - ema_val_iou " in ln for ln in lines), r.stdout[-2000:]
    run = tmp_path / "models" / "ema_e2e"
    rows = [ln.split(",") for ln in open(run / "log.csv").read().strip().splitlines()]
    assert rows[0] == ["epoch", "lr", "loss", "iou", "val_loss", "val_iou", "images_per_sec", "ema_val_loss", "ema_val_iou"]
    assert len(rows) == 3
    assert "ema_decay: 0.9" in open(run / "config.yml").read() and "ema_warmup: true" in open(run / "config.yml").read()
    assert (run / "model_ema.pth").exists() and "=> saved best EMA model" in r.stdout
    best = max(float(row[-1]) for row in rows[1:])
    val = [sys.executable, os.path.join(ROOT, "val.py"), "--name", "ema_e2e", "--ema", "true", "--no_images"]
    v = subprocess.run(val, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert v.returncode == 0, v.stdout[-2000:] + v.stderr[-2000:]
    assert "weights: EMA (model_ema.pth)" in v.stdout
    assert "IoU: %.4f" % best in v.stdout.splitlines(), (best, v.stdout[-500:])
    os.remove(run / "model_ema.pth")
    v = subprocess.run(val, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert v.returncode == 2 and "model_ema.pth" in v.stdout and "--ema_decay" in v.stdout, v.stdout[-500:]
