"""Pruned UNet++ inference (nunet_plan_create_pruned, NestedUNet.forward(x, depth=L)) on the GPU.

A pruned plan issues exactly the launches the full eval forward issues for the blocks it keeps - same kernels, same inputs - so
its logits are held to BIT equality with head L of the full forward (which the golden tests pin), in every storage dtype; one
fp32 anchor compares with the CPU oracle under the bound tests/test_net_gpu.py applies to fp32 eval logits (1e-4, scaled by
the largest logit when that exceeds 1). The weights carry running statistics that are not the identity (fresh_bn=False)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from oracle import nunet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEPTHS = (1, 2, 3, 4)
# (N, H, W, K): level 4 is 1 x 1 | odd level sizes (3 x 2 at level 4), several classes, a batch that is no power of two | the plain case
SHAPES = [(1, 16, 16, 1), (3, 48, 32, 4), (2, 32, 32, 1)]
CENSUS = {1: 6, 2: 12, 3: 20, 4: 30}      # two 3x3 convolutions per kept block
GUARD, PATTERN = 4096, 0xA5


@functools.lru_cache(maxsize=None)
def _state(ncls):
    return nunet_amd.synth.closed_form_state(ncls, 3, True, False)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """-> (model in eval mode, input on the device, the full forward's four logits): computed once, shared - do not write to them"""
    n, h, w, ncls = shape
    m = nunet_amd.archs.NestedUNet(ncls, 3, True, dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _state(ncls).items()})
    m = m.to(DEV).eval()
    img, _ = nunet_amd.synth.synth_batch(n, h, w, 3, ncls, seed=1234)
    x = torch.from_numpy(img).to(DEV)
    with torch.no_grad():
        full = [o.clone() for o in m(x)]
    return m, x, full


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_%dx%d_k%d" % s)
def test_pruned_logits_equal_the_full_forwards_head_bit_for_bit(shape, dtype):
    m, x, full = _case(shape, dtype)
    n, h, w, ncls = shape
    assert len(full) == 4
    for d in DEPTHS:
        with torch.no_grad():
            got = m(x, depth=d)
        assert tuple(got.shape) == (n, ncls, h, w) and got.dtype == torch.float32
        assert bool(torch.isfinite(got).all())
        diff = float((got - full[d - 1]).abs().max())
        print("%s %s depth %d: max |pruned - full| = %.3g" % (shape, dtype, d, diff))
        assert torch.equal(got, full[d - 1]), (shape, dtype, d, diff)
        pl = m._engine.plans[(n, h, w, m.compute_dtype, d)]
        assert pl.depth == d and pl.heads == 1 and len(pl.census(False)) == CENSUS[d]
        assert pl.arena_bytes < m._engine.plans[(n, h, w, m.compute_dtype)].arena_bytes
    # the heads differ from each other: equality above is not four copies of one tensor
    assert not torch.equal(full[0], full[3])
    # a second call reuses the cached plan and repeats the bits; the full forward is untouched by the pruned ones
    with torch.no_grad():
        assert torch.equal(m(x, depth=2), full[1])
        again = m(x)
    assert all(torch.equal(a, b) for a, b in zip(again, full))


def test_depth_2_against_the_cpu_oracle():
    """the bound of tests/test_net_gpu.py for fp32 eval logits: 1e-4 x max(1, largest |logit|)"""
    shape = (2, 32, 32, 1)
    m, x, _ = _case(shape, "fp32")
    net = O.OracleNet(_state(1), 1, 3, True, dtype=torch.float64)
    net.eval()
    with torch.no_grad():
        ref = net(x.cpu().double())[1]
        got = m(x, depth=2)
    scale = max(1.0, float(ref.abs().max()))
    err = float((got.cpu().double() - ref).abs().max())
    print("depth 2 fp32 vs the fp64 oracle's head 2: max |diff| = %.3g (scale %.3g)" % (err, scale))
    assert err < 1e-4 * scale


def _raw_plan(lib, shape, dtype, depth):
    n, h, w, ncls = shape
    cfg = L.PlanCfg(n, h, w, 3, ncls, 1, dtype, 0)
    p = lib.nunet_plan_create_pruned(C.byref(cfg), depth) if depth else lib.nunet_plan_create(C.byref(cfg))
    assert p, lib.nunet_last_error()
    return p


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_stays_inside_the_arena_and_the_logits(dtype):
    """nunet_plan_forward called directly, arena and logits with a patterned guard region behind nunet_plan_arena_bytes and
    behind [1, N, K, H, W]: intact at every depth, and the logits are the full forward's"""
    shape = (3, 48, 32, 4)
    n, h, w, ncls = shape
    m, x, full = _case(shape, dtype)
    eng, lib = m._engine, L.lib()
    for d in DEPTHS:
        p = _raw_plan(lib, shape, m.compute_dtype, d)
        try:
            nb = lib.nunet_plan_arena_bytes(p)
            raw = torch.full((nb + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
            nl = n * ncls * h * w
            lg = torch.full((nl + GUARD // 4,), -12345.0, dtype=torch.float32, device=DEV)
            assert raw.data_ptr() % 256 == 0
            for flags in (0, 2):      # pack + forward, then a forward on the packed weights
                L.check(lib.nunet_plan_forward(p, L.ptr(eng.flat_params), L.ptr(eng.bnbuf), L.ptr(eng.nbt), L.ptr(x), L.ptr(raw), nb,
                                               L.ptr(lg), flags, L.stream()), "nunet_plan_forward")
                torch.cuda.synchronize()
                assert bool((raw[nb:] == PATTERN).all()), ("write past the arena", d, flags)
                assert bool((lg[nl:] == -12345.0).all()), ("write past the logits", d, flags)
                assert torch.equal(lg[:nl].view(n, ncls, h, w), full[d - 1]), (d, flags)
            assert lib.nunet_plan_census_count(p, 0) == CENSUS[d]
            # an arena one byte short is refused
            assert lib.nunet_plan_forward(p, L.ptr(eng.flat_params), L.ptr(eng.bnbuf), L.ptr(eng.nbt), L.ptr(x), L.ptr(raw), nb - 1,
                                          L.ptr(lg), 0, L.stream()) == -1
            L.check(lib.nunet_plan_repack(p, L.ptr(eng.flat_params), L.ptr(raw), nb, L.stream()), "nunet_plan_repack")
            torch.cuda.synchronize()
            assert bool((raw[nb:] == PATTERN).all()), ("repack wrote past the arena", d)
        finally:
            lib.nunet_plan_destroy(p)


def test_training_entries_are_refused_and_touch_nothing():
    shape = (2, 32, 32, 1)
    n, h, w, ncls = shape
    m, x, _ = _case(shape, "fp32")
    eng, lib = m._engine, L.lib()
    p = _raw_plan(lib, shape, L.F32, 2)
    try:
        nb = lib.nunet_plan_arena_bytes(p)
        arena = torch.full((nb,), 0x3C, dtype=torch.uint8, device=DEV)
        params = eng.flat_params.clone()
        bnbuf, nbt = eng.bnbuf.clone(), eng.nbt.clone()
        grads = torch.zeros_like(params)
        state = torch.zeros_like(params)
        logits = torch.zeros(1, n, ncls, h, w, device=DEV)
        dlogits = torch.ones(1, n, ncls, h, w, device=DEV)
        lr = torch.full((1,), 0.1, device=DEV)
        ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
        out = torch.zeros(n, h, w, 32, device=DEV)
        opt = L.Optim(kind=L.OPT_SGD, momentum=0.9, weight_decay=1e-4, nesterov=0, lr=L.ptr(lr).value, state0=L.ptr(state).value)
        off, b0, tot = C.c_int64(), C.c_int64(), C.c_int64()
        before = (arena.clone(), params.clone(), bnbuf.clone(), nbt.clone())
        st = L.stream()
        calls = {
            "nunet_plan_forward (training)": lambda: lib.nunet_plan_forward(p, L.ptr(params), L.ptr(bnbuf), L.ptr(nbt), L.ptr(x), L.ptr(arena), nb,
                                                                            L.ptr(logits), 1, st),
            "nunet_plan_backward": lambda: lib.nunet_plan_backward(p, L.ptr(params), L.ptr(dlogits), L.ptr(arena), nb, L.ptr(grads), 0, st),
            "nunet_plan_backward_phase": lambda: lib.nunet_plan_backward_phase(p, L.ptr(params), L.ptr(dlogits), L.ptr(arena), nb, L.ptr(grads), 0, 3, st),
            "nunet_plan_opt_step": lambda: lib.nunet_plan_opt_step(p, L.ptr(params), C.byref(opt), L.ptr(arena), nb, 1.0, L.ptr(grads), st),
            "nunet_plan_grad_sqnorm": lambda: lib.nunet_plan_grad_sqnorm(p, L.ptr(arena), nb, L.ptr(ws), L.nbytes(ws), st),
            "nunet_plan_grad_scratch": lambda: lib.nunet_plan_grad_scratch(p, C.byref(off), C.byref(b0), C.byref(tot)),
            "nunet_plan_bucket0_wait": lambda: lib.nunet_plan_bucket0_wait(p, st),
            "nunet_plan_set_wgrad_dy": lambda: lib.nunet_plan_set_wgrad_dy(p, 1),
            "nunet_plan_block_act1": lambda: lib.nunet_plan_block_act1(p, L.ptr(params), L.ptr(arena), nb, 0, 0, L.ptr(out), st),
        }
        for what, call in calls.items():
            assert call() == -1, what
            assert b"pruned" in lib.nunet_last_error(), (what, lib.nunet_last_error())
        assert lib.nunet_plan_grad_sqnorm_ws_bytes(p) == 0
        torch.cuda.synchronize()
        for a, b in zip(before, (arena, params, bnbuf, nbt)):
            assert torch.equal(a, b)
        assert not bool(grads.any()) and not bool(logits.any()) and not bool(out.any()) and not bool(ws.any())
    finally:
        lib.nunet_plan_destroy(p)


def test_python_surface_refuses_what_a_pruned_network_cannot_do():
    m, x, full = _case((2, 32, 32, 1), "fp32")
    m.train()
    try:
        with pytest.raises(L.NunetError, match="eval"):
            m(x, depth=2)
    finally:
        m.eval()
    for bad in (0, 5, True, 2.0, "2"):
        with pytest.raises(L.NunetError, match="depth"):
            m(x, depth=bad)
    plain = nunet_amd.archs.NestedUNet(1, 3, False).to(DEV).eval()
    with pytest.raises(L.NunetError, match="deep_supervision"):
        plain(x, depth=2)
    unet = nunet_amd.archs.UNet(1, 3).to(DEV).eval()
    with pytest.raises(L.NunetError, match="UNet"):
        unet(x, depth=2)
    with torch.no_grad():      # depth=None is the forward as before
        assert torch.equal(m(x, depth=None)[3], full[3])
