"""The three launch-saving choices of the plan - BatchNorm2 + ReLU inside the last head's launch (nunet_plan_set_head_bn), the x2
upsample inside the producer's BatchNorm2 launch (nunet_plan_set_bn_up) and the pruning of implied cross-lane waits
(nunet_plan_set_wait_prune) - change no bit of what a pass computes: each of them on against all of them off, on eager passes
of whole plans and on captured training steps under both executors. Runs on the MI355X only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
N, HW = 2, 32
BN_UP_NONE, BN_UP_CHAIN, BN_UP_ALL = 0, 1, 2          # NUNET_BN_UP_* in include/nunet_diag.h
OFF = dict(head_bn=0, bn_up=BN_UP_NONE, wait_prune=0)
VARIANTS = {
    "all off": OFF,
    "head_bn": dict(OFF, head_bn=1),
    "bn_up chain": dict(OFF, bn_up=BN_UP_CHAIN),
    "bn_up all": dict(OFF, bn_up=BN_UP_ALL),
    "wait_prune": dict(OFF, wait_prune=1),
    "all on": dict(head_bn=1, bn_up=BN_UP_ALL, wait_prune=1),
}


def set_switches(pl, head_bn, bn_up, wait_prune):
    lib = L.lib()
    L.check(lib.nunet_plan_set_head_bn(pl.handle, head_bn), "plan_set_head_bn")
    L.check(lib.nunet_plan_set_bn_up(pl.handle, bn_up), "plan_set_bn_up")
    L.check(lib.nunet_plan_set_wait_prune(pl.handle, wait_prune), "plan_set_wait_prune")


def assert_all_equal(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        assert torch.equal(ref[k], got[k]), "%s: %s differs" % (what, k)


def blocks_of(kind, depth=None):
    if kind == "unet":
        return [(i, 0) for i in range(5)] + [(i, 4 - i) for i in range(4)]
    top = 4 if depth is None else depth
    return [(i, j) for i in range(5) for j in range(5) if i + j <= top]


@pytest.fixture(scope="module")
def batch(synth):
    img, msk = synth.synth_batch(N, HW, HW, 3, 1, seed=77)
    g = torch.Generator().manual_seed(5)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV), torch.randn(4, N, 1, HW, HW, generator=g).to(DEV)


def build(kind, dtype, seed=3):
    torch.manual_seed(seed)
    if kind == "unet":
        return nunet_amd.archs.UNet(1, 3, dtype=dtype).to(DEV)
    return nunet_amd.archs.NestedUNet(1, 3, kind == "nested_ds", dtype=dtype).to(DEV)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["nested", "nested_ds", "unet"])
def test_training_pass_of_a_plan(kind, dtype, batch):
    """One eager forward + backward (the lanes as real streams): logits, every block output, the parameter gradients and the
    BatchNorm buffers."""
    x, _, r = batch
    ref = None
    for name, sw in VARIANTS.items():
        m = build(kind, dtype).train()
        pl = m.plan_for(x)
        set_switches(pl, **sw)
        out = m(x)
        outs = out if isinstance(out, list) else [out]
        sum((o * r[k]).sum() for k, o in enumerate(outs)).backward()
        torch.cuda.synchronize()
        eng = m.engine()
        got = {"logits%d" % k: o.detach().clone() for k, o in enumerate(outs)}
        got.update({"x%d_%d" % ij: pl.feature(*ij).clone() for ij in blocks_of(kind)})
        got.update(grads=eng.flat_grads.clone(), bn_running=eng.bnbuf.clone(), nbt=eng.nbt.clone())
        assert bool(torch.isfinite(got["grads"]).all())
        if ref is None:
            ref = got
        else:
            assert_all_equal(ref, got, "%s %s, %s" % (kind, dtype, name))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_pruned_plan_of_depth_2(dtype, batch):
    """An eval forward of the plan pruned to final2: its head is the fused launch (BatchNorm from the running statistics)."""
    x = batch[0]
    ref = None
    for name, sw in VARIANTS.items():
        m = build("nested_ds", dtype).eval()
        with torch.no_grad():
            pl = m.plan_for(x, depth=2)
            set_switches(pl, **sw)
            got = {"logits": m(x, depth=2).clone()}
        got.update({"x%d_%d" % ij: pl.feature(*ij).clone() for ij in blocks_of("nested_ds", 2)})
        torch.cuda.synchronize()
        if ref is None:
            ref = got
        else:
            assert_all_equal(ref, got, "pruned %s, %s" % (dtype, name))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("executor", [("flags", "list"), (False, "lanes")])
def test_captured_train_step(executor, dtype, synth):
    """The captured TrainStep forced to the flag executor and to the graph executor, 8 replays: the seven arrays bench.py
    --dump-outputs writes, read from the objects, and every block output. Under the flag executor wait pruning records no more
    waits, signals and kernel nodes (the ops are the same: the difference is sync kernels) than it does switched off."""
    from nunet_amd.trainer import TrainStep
    seg, sched = executor
    batches = [synth.synth_batch(N, HW, HW, 3, 1, seed=500 + k) for k in range(3)]
    batches = [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b in batches]
    ref, info = None, {}
    for name, sw in VARIANTS.items():
        m = build("nested", dtype, seed=9).train()
        ts = TrainStep(m, (N, 3, HW, HW), lr=1e-2, segmented=seg, schedule=sched)
        set_switches(ts.pl, **sw)
        ts.capture(*batches[0])
        for k in range(8):
            ts.step(*batches[k % 3])
        torch.cuda.synchronize()
        got = {"logits": ts.logits, "loss": ts.loss_out, "meters": ts.meters, "params": ts.eng.flat_params, "grads": ts.eng.flat_grads,
               "momentum": ts.mom, "bn_running": ts.eng.bnbuf}
        got = {k: v.clone() for k, v in got.items()}
        got.update({"x%d_%d" % ij: ts.pl.feature(*ij).clone() for ij in blocks_of("nested")})
        assert bool(torch.isfinite(got["params"]).all())
        if seg:
            info[name] = ts.g_fb.info()
        if ref is None:
            ref = got
        else:
            assert_all_equal(ref, got, "%s/%s %s, %s" % (seg, sched, dtype, name))
        del ts, m
    if seg:
        off, on = info["all off"], info["wait_prune"]
        print("flag program, wait pruning off:", off)
        print("flag program, wait pruning on: ", on)
        for k in ("event_waits", "event_records", "kernel_nodes"):
            assert on[k] <= off[k], (k, on, off)
        print("flag program, head_bn:", info["head_bn"], " bn_up chain:", info["bn_up chain"], " bn_up all:", info["bn_up all"],
              " all on:", info["all on"])
