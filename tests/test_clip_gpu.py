"""Gradient-norm clipping inside the fused step on the MI355X (TrainStep(clip_grad_norm=...)): the flat square-norm kernel and
the finalize launch against torch in fp64, the plan-scratch norm against p.grad in every model shape and update layout, inf as
the identity, a binding clip against torch.nn.utils.clip_grad_norm_ + stock torch optimisers, a threshold that changes between
replays of one captured step, the interplay with loss scaling, and train.py --clip_grad_norm end to end.

Norm tolerance: 1e-6 relative against an fp64 torch norm. Every element carries at most one fp32 rounding (g * gscale,
<= 2^-24 relative) and the sum of squares is exact products summed in double, so the norm is within about 1e-7."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.trainer import TrainStep  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH = dict(segmented=False, schedule="lanes")      # the one-hipGraph executor, chosen without timing
INF = float("inf")
EINVAL = -1


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


def _grad_norm64(model):
    return float(torch.linalg.vector_norm(torch.cat([p.grad.detach().double().reshape(-1) for p in model.parameters()])))


def _state(ts):
    eng = ts.eng
    out = [eng.flat_params, eng.bnbuf, eng.nbt, ts.meters, eng.flat_grads] + ts.opt_state
    return [t.detach().clone() for t in out]


def _clip_words(clip):
    """(max_norm, coef, norm, peak, norm_sum, clipped, steps) of a nunet_clip tensor"""
    torch.cuda.synchronize()
    w = clip.cpu()
    f = w.view(torch.float32)
    return float(f[0]), float(f[1]), float(f[2]), float(f[3]), float(w[4:6].view(torch.float64)), int(w[6]), int(w[7])


def _torch_coef(max_norm, norm):
    """clip_grad_norm_'s factor as torch forms it: an fp32 tensor norm, a Python-float max_norm"""
    return float(torch.clamp(max_norm / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0))


# -- 1. flat kernel + finalize -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1025, 4099, 2 ** 20 + 5])
def test_flat_sqnorm_and_finalize_against_fp64(n, offset, guard_bands):
    """nunet_grad_sqnorm + nunet_clip_finalize over n values randn * 10^U(-6, 3), the pointer 16-byte aligned (offset 0) or one
    float past it (the scalar head / tail path): norm to 1e-6 of torch's fp64 norm; coef for max_norm in {inf, 2 norm, 0.3 norm}
    to 1e-6 of torch's formula (exactly 1 wherever torch's is: always for inf, for 2 norm unless the norm is of the order of the
    formula's 1e-6); the statistics after the three calls; bit-identical norms; a workspace one byte short is refused."""
    lib = L.lib()
    gen = torch.Generator(device=DEV).manual_seed(1000 + n)
    vals = torch.randn(n, device=DEV, generator=gen) * 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 9.0 - 6.0)
    buf = torch.zeros(n + offset, dtype=torch.float32, device=DEV)
    g = buf[offset:]
    g.copy_(vals)
    assert g.data_ptr() % 16 == 4 * offset
    nb = lib.nunet_grad_sqnorm_ws_bytes(n)
    assert nb >= 8 and nb % 8 == 0
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=DEV)
    clip = torch.zeros(L.CLIP_WORDS, dtype=torch.int32, device=DEV)
    st = L.stream()
    assert lib.nunet_grad_sqnorm(L.ptr(g), n, L.ptr(ws), nb - 1, st) == EINVAL
    ref = float(torch.linalg.vector_norm(g.double()))
    ref32 = float(torch.tensor(ref, dtype=torch.float32))
    seen, wants = [], []
    for max_norm in (INF, 2.0 * ref, 0.3 * ref):
        clip[0:1].view(torch.float32).fill_(max_norm)
        ws.fill_(float("nan"))
        L.check(lib.nunet_grad_sqnorm(L.ptr(g), n, L.ptr(ws), nb, st), "grad_sqnorm")
        L.check(lib.nunet_clip_finalize(L.ptr(ws), ws.numel(), 1.0, None, L.ptr(clip), st), "clip_finalize")
        mx, coef, norm, peak, nsum, clipped, steps = _clip_words(clip)
        print("n %d offset %d max_norm %g: norm %.9g (fp64 %.17g, rel %.2e) coef %.9g" % (n, offset, max_norm, norm, ref, abs(norm - ref) / ref, coef))
        assert abs(norm - ref) <= 1e-6 * ref
        want = _torch_coef(max_norm, ref32)
        assert abs(coef - want) <= 1e-6 * want
        if want == 1.0:
            assert coef == 1.0
        seen.append(norm)
        wants.append(want)
    assert wants[0] == 1.0 and wants[2] < 1.0
    mx, coef, norm, peak, nsum, clipped, steps = _clip_words(clip)
    assert seen[0] == seen[1] == seen[2] == peak == norm
    assert (clipped, steps) == (sum(1 for w in wants if w < 1.0), 3)
    assert nsum == 3.0 * norm
    assert torch.equal(g, vals)                      # read-only


def test_finalize_scales_the_norm_and_honours_found_inf(guard_bands):
    """grad_scale and the scaler's inv_scale multiply the norm; with found_inf set, coef = 1 and the statistics stay."""
    lib, st = L.lib(), L.stream()
    ws = torch.tensor([9.0, 16.0, 0.0], dtype=torch.float64, device=DEV)       # sum 25: norm 5
    clip = torch.zeros(L.CLIP_WORDS, dtype=torch.int32, device=DEV)
    clip[0:1].view(torch.float32).fill_(1.0)
    scaler = torch.zeros(L.SCALER_WORDS, dtype=torch.int32, device=DEV)
    scaler[0:2] = torch.tensor([4.0, 0.25], dtype=torch.float32).view(torch.int32).to(DEV)
    L.check(lib.nunet_clip_finalize(L.ptr(ws), 3, 0.5, L.ptr(scaler), L.ptr(clip), st), "clip_finalize")
    mx, coef, norm, peak, nsum, clipped, steps = _clip_words(clip)
    assert norm == 0.625 and (clipped, steps) == (0, 1) and coef == 1.0
    clip[0:1].view(torch.float32).fill_(0.25)
    L.check(lib.nunet_clip_finalize(L.ptr(ws), 3, 0.5, L.ptr(scaler), L.ptr(clip), st), "clip_finalize")
    before = _clip_words(clip)
    assert before[5:] == (1, 2) and abs(before[1] - _torch_coef(0.25, 0.625)) <= 1e-6
    scaler[3] = 1                                    # found_inf
    L.check(lib.nunet_clip_finalize(L.ptr(ws), 3, 0.5, L.ptr(scaler), L.ptr(clip), st), "clip_finalize")
    after = _clip_words(clip)
    assert after[1] == 1.0 and after[2:] == before[2:] and after[0] == before[0]


# -- 2. plan-scratch norm vs p.grad --------------------------------------------------------------------------------------------
CONFIGS = {
    "nested_k1_c3": dict(ncls=1, cin=3, ds=False, arch="NestedUNet"),
    "nested_k4_ds": dict(ncls=4, cin=3, ds=True, arch="NestedUNet"),       # four heads, each the sum of its slabs
    "nested_k2_c1": dict(ncls=2, cin=1, ds=False, arch="NestedUNet"),
    "unet_k1_c3": dict(ncls=1, cin=3, ds=False, arch="UNet"),
}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_plan_scratch_norm_equals_the_norm_of_p_grad(synth, config, dtype):
    """TrainStep(lr=0, use_graph=False, clip_grad_norm=inf), 2x32x32, in both update layouts: the reported norm equals
    vector_norm(cat(p.grad.double())) to 1e-6 (padding of cin up to cinpad - 16 in fp32, 32 in bf16 - does not count; heads are
    summed from their slabs before they are squared), and is bit-identical when the step runs again from the same parameters."""
    c = CONFIGS[config]
    if c["arch"] == "UNet":
        st = synth.closed_form_state_unet(c["ncls"], c["cin"])
    else:
        st = synth.closed_form_state(c["ncls"], c["cin"], c["ds"], True)
    (x, t), = _batches(synth, 2, 32, c["ncls"], [101], cin=c["cin"])
    for fused_update in (0, 2):
        m = _module(st, c["ncls"], dtype, c["cin"], c["ds"], c["arch"])
        ts = TrainStep(m, (2, c["cin"], 32, 32), lr=0.0, use_graph=False, fused_update=fused_update, clip_grad_norm=INF)
        print("executor_choice", ts.executor_choice)
        ts.step(x, t)
        s1 = ts.grad_norm_stats()
        ref = _grad_norm64(m)
        print("%s %s layout %d: norm %.9g, fp64 norm of p.grad %.17g, rel %.2e" % (config, dtype, fused_update, s1["last"], ref,
                                                                               abs(s1["last"] - ref) / ref))
        assert ref > 0 and abs(s1["last"] - ref) <= 1e-6 * ref
        ts.step(x, t)
        s2 = ts.grad_norm_stats()
        assert s2["last"] == s1["last"] and s2["steps"] == 2 and s2["clipped"] == 0
        assert s2["peak"] == s1["last"] and abs(s2["mean"] - s1["last"]) <= 1e-12 * s1["last"]
        del ts, m


# -- 3. inf is the identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
@pytest.mark.parametrize("fused_update", [0, 2])
def test_inf_is_the_identity(synth, dtype, optimizer, fused_update):
    """clip_grad_norm=inf: after 3 graph steps parameters, gradients, optimiser state, BN buffers and meters are bit-identical
    to clip_grad_norm=None; nothing was clipped, three steps were counted."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [11, 12, 13])
    res = []
    for clip in (None, INF):
        m = _module(st, 1, dtype)
        ts = TrainStep(m, (4, 3, 64, 64), lr=1e-2, optimizer=optimizer, fused_update=fused_update, clip_grad_norm=clip, **GRAPH)
        ts.capture(*data[0])
        print("executor_choice", ts.executor_choice)
        for x, t in data:
            ts.step(x, t)
        torch.cuda.synchronize()
        res.append(_state(ts))
        if clip is None:
            assert ts.grad_norm_stats() is None
        else:
            s = ts.grad_norm_stats()
            assert (s["clipped"], s["steps"]) == (0, 3) and s["last"] > 0 and s["peak"] >= s["mean"] > 0
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), k


# -- 4. a binding clip against stock torch -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unclipped(synth):
    """The unclipped mean gradient of one batch from the closed-form state (an lr = 0 step) and its norm: computed once."""
    st = synth.closed_form_state(1, 3, False, True)
    (x, t), = _batches(synth, 2, 32, 1, [202])
    m = _module(st)
    ts = TrainStep(m, (2, 3, 32, 32), lr=0.0, use_graph=False, clip_grad_norm=INF)
    ts.step(x, t)
    n0 = ts.grad_norm_stats()["last"]
    grads = [p.grad.detach().clone() for p in m.parameters()]
    return dict(st=st, x=x, t=t, n0=n0, grads=grads)


@pytest.mark.parametrize("fused_update", [0, 2])
@pytest.mark.parametrize("optimizer", ["SGD", "SGD-nesterov", "Adam"])
def test_binding_clip_against_torch(unclipped, optimizer, fused_update):
    """One real step with clip_grad_norm = 0.25 n0 against clones of the parameters with .grad = g, clip_grad_norm_, and one
    step of the stock torch optimiser: max|p - p_expected| <= 1e-4 max|p - p0| (the bound tests/test_adam_gpu.py uses between
    update layouts); ||p.grad|| = 0.25 n0 n0 / (n0 + 1e-6) to 1e-5; one step clipped.
    The learning rate is 1e-2 for every optimiser. The bound is relative to the largest move, which for a first Adam step is lr
    itself, while the parameters are stored in fp32: BatchNorm's gamma lies in [1, 2), where one ulp is 1.19e-7. The bound has
    to stay above that resolution to say anything about the clip: at lr = 1e-2 it is 1e-6, eight ulp of such a parameter. (At
    torch's default Adam lr of 1e-3 the bound would be 1.0e-7, below one ulp: measured on the MI355X there, layout 0,
    max|p - p_expected| = 1.19e-7 - a single last-bit difference to torch's own Adam rounding - against max|p - p0| = 1.00e-3.)"""
    u = unclipped
    n0, max_norm = u["n0"], 0.25 * u["n0"]
    m = _module(u["st"])
    kw = dict(optimizer="Adam", lr=1e-2) if optimizer == "Adam" else dict(optimizer="SGD", lr=1e-2, momentum=0.9,
                                                                           nesterov=optimizer == "SGD-nesterov")
    ts = TrainStep(m, (2, 3, 32, 32), weight_decay=1e-4, use_graph=False, fused_update=fused_update, clip_grad_norm=max_norm, **kw)
    print("executor_choice", ts.executor_choice)
    p0 = ts.eng.flat_params.detach().clone()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    for c, g in zip(clones, u["grads"]):
        c.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(clones, max_norm)
    if optimizer == "Adam":
        opt = torch.optim.Adam(clones, lr=1e-2, weight_decay=1e-4)
    else:
        opt = torch.optim.SGD(clones, lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=optimizer == "SGD-nesterov")
    opt.step()
    ts.step(u["x"], u["t"])
    s = ts.grad_norm_stats()
    assert abs(s["last"] - n0) <= 1e-6 * n0 and abs(float(total) - n0) <= 1e-5 * n0
    assert (s["clipped"], s["steps"]) == (1, 1)
    worst = max(float((p.detach() - c.detach()).abs().max()) for p, c in zip(m.parameters(), clones))
    moved = float((ts.eng.flat_params - p0).abs().max())
    print("%s layout %d: max|p - p_expected| %.3e, max|p - p0| %.3e" % (optimizer, fused_update, worst, moved))
    assert moved > 0 and worst <= 1e-4 * moved
    gn, want = _grad_norm64(m), 0.25 * n0 * n0 / (n0 + 1e-6)
    assert abs(gn - want) <= 1e-5 * want, (gn, want)


# -- 5. replay with a changing threshold ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("executor", [dict(segmented=False, schedule="lanes"), dict(segmented="flags", schedule="list")])
def test_threshold_changes_between_replays(synth, executor):
    """Captured with inf; step, set_clip_grad_norm(0.5 last), step, set_clip_grad_norm(inf), step - against an unclipped twin
    (plain SGD, so a clipped step is the unclipped one scaled): the first step is bit-identical to the twin's, the middle
    step moves the parameters less, one step was clipped, and the captured program was never replaced."""
    st = synth.closed_form_state(1, 3, False, True)
    data = _batches(synth, 4, 64, 1, [61, 62, 63])
    kw = dict(lr=1e-2, momentum=0.0, weight_decay=0.0)
    twin_m = _module(st)
    twin = TrainStep(twin_m, (4, 3, 64, 64), **kw, **executor)
    twin.capture(*data[0])
    m = _module(st)
    ts = TrainStep(m, (4, 3, 64, 64), clip_grad_norm=INF, **kw, **executor)
    ts.capture(*data[0])
    print("executor_choice", ts.executor_choice, executor)
    g = ts.g_fb
    assert g is not None
    moves = []
    for k, (x, t) in enumerate(data):
        pa, pb = ts.eng.flat_params.clone(), twin.eng.flat_params.clone()
        ts.step(x, t)
        twin.step(x, t)
        torch.cuda.synchronize()
        moves.append((float((ts.eng.flat_params - pa).double().norm()), float((twin.eng.flat_params - pb).double().norm())))
        if k == 0:
            assert torch.equal(ts.eng.flat_params, twin.eng.flat_params)
            ts.set_clip_grad_norm(0.5 * ts.grad_norm_stats()["last"])
        elif k == 1:
            ts.set_clip_grad_norm(INF)
    print("parameter moves (clipped run, twin):", moves)
    s = ts.grad_norm_stats()
    assert (s["clipped"], s["steps"]) == (1, 3)
    assert moves[0][0] == moves[0][1] > 0
    assert moves[1][0] < moves[1][1]
    assert ts.g_fb is g


# -- 6. with loss scaling ------------------------------------------------------------------------------------------------------
def test_norm_is_that_of_the_unscaled_gradient(synth):
    """fp32 storage: the norm reported under init_scale 1024 equals the one under init_scale 1 to 1e-5 (the fixed-point
    BatchNorm sums are not scale-equivariant in their last bits, tests/test_loss_scale_gpu.py test_power_of_two_scale_fp32)."""
    st = synth.closed_form_state(1, 3, False, True)
    (x, t), = _batches(synth, 2, 32, 1, [71])
    norms = []
    for init in (1024.0, 1.0):
        m = _module(st)
        ts = TrainStep(m, (2, 3, 32, 32), lr=1e-2, use_graph=False, loss_scale=dict(init_scale=init), clip_grad_norm=INF)
        print("executor_choice", ts.executor_choice)
        ts.step(x, t)
        assert ts.scaler_stats() == (init, 0)
        norms.append(ts.grad_norm_stats()["last"])
        assert abs(norms[-1] - _grad_norm64(m)) <= 1e-6 * norms[-1]
    print("norms under scale 1024 / 1:", norms)
    assert abs(norms[0] - norms[1]) <= 1e-5 * norms[1]


@pytest.mark.parametrize("optimizer,lr", [("SGD", 1e-3), ("Adam", 1e-5)])
def test_skipped_step_leaves_the_clip_statistics(synth, optimizer, lr):
    """fp16 with loss scaling: an inf written into the gradient scratch behind the backward pass skips the step - parameters,
    optimiser state and the clip statistics are unchanged, the scale backs off - and the next clean step clips and counts.
    The threshold of the last step is half the norm of the first, so the first step must not halve the gradient norm: a first
    Adam step moves EVERY parameter by lr whatever its gradient, so Adam runs at lr = 1e-5 (at 1e-3 the last step was not
    clipped on the MI355X: its norm did not exceed the threshold)."""
    st = synth.closed_form_state(1, 3, False, True)
    (x, t), = _batches(synth, 2, 32, 1, [81])
    m = _module(st, 1, "fp16")
    ts = TrainStep(m, (2, 3, 32, 32), lr=lr, use_graph=False, optimizer=optimizer, loss_scale=dict(init_scale=1024.0), clip_grad_norm=INF)
    print("executor_choice", ts.executor_choice)
    ts.step(x, t)
    s1 = ts.grad_norm_stats()
    assert ts.scaler_stats() == (1024.0, 0) and (s1["clipped"], s1["steps"]) == (0, 1) and math.isfinite(s1["last"]) and s1["last"] > 0
    ts.set_clip_grad_norm(0.5 * s1["last"])
    bwd = ts._bwd

    def poisoned(phases):
        bwd(phases)
        ts._scratch[12345] = float("inf")
    ts._bwd = poisoned
    before = [v.clone() for v in [ts.eng.flat_params] + ts.opt_state]
    ts.step(x, t)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [ts.eng.flat_params] + ts.opt_state))
    assert ts.scaler_stats() == (512.0, 1)
    s2 = ts.grad_norm_stats()
    assert s2 == s1, (s1, s2)
    assert _clip_words(ts._clip)[1] == 1.0           # coef of the skipped step
    ts._bwd = bwd
    ts.step(x, t)
    s3 = ts.grad_norm_stats()
    print("%s lr %g: norm of step 1 %.6g, of step 3 %.6g" % (optimizer, lr, s1["last"], s3["last"]))
    assert ts.scaler_stats() == (512.0, 1)
    assert (s3["clipped"], s3["steps"]) == (1, 2)
    assert not torch.equal(before[0], ts.eng.flat_params)
    coef = _clip_words(ts._clip)[1]
    assert abs(coef - _torch_coef(0.5 * s1["last"], s3["last"])) <= 1e-6
    gn = _grad_norm64(m)
    assert abs(gn - coef * s3["last"]) <= 1e-5 * gn


# -- 7. train.py ---------------------------------------------------------------------------------------------------------------
def test_train_py_clip_grad_norm(tmp_path):
    """train.py --clip_grad_norm 1.0 for one epoch: the fused step, the grad-norm text on the epoch line, log.csv as before."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--clip_grad_norm", "1.0", "--epochs", "1", "--train_size", "32",
           "--val_size", "16", "--batch_size", "4", "--input_h", "32", "--input_w", "32", "--name", "clip_e2e"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "=> fused training step (TrainStep)" in r.stdout and "grad norm clipped at 1" in r.stdout, r.stdout[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch [0/1]")]
    assert len(line) == 1 and " - grad norm " in line[0] and " steps clipped" in line[0], r.stdout[-2000:]
    rows = open(tmp_path / "models" / "clip_e2e" / "log.csv").read().strip().splitlines()
    assert rows[0].split(",") == ["epoch", "lr", "loss", "iou", "val_loss", "val_iou", "images_per_sec"]
    assert len(rows) == 2
