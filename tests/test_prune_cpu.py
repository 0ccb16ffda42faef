"""Host-only: nunet_plan_create_pruned (include/nunet.h). Plan creation is host code, so the layout facts of a pruned plan -
the parameter layout of the whole deep-supervision model, one head, an arena that grows with the depth and stays below the
full plan's, the kept blocks - are checked without a GPU, and so is every refusal that needs no device buffer."""
import ctypes as C

import pytest

from nunet_amd import _lib as L

NUNET_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def _cfg(ncls=1, ds=1, unet=0, dtype=L.F32):
    return L.PlanCfg(2, 32, 32, 3, ncls, ds, dtype, unet)


@pytest.fixture(scope="module", params=[1, 4], ids=["k1", "k4"])
def plans(request, lib):
    """(K, full plan, {depth: pruned plan}) at (2, 32, 32, 3, K, ds=1), destroyed after the module's tests"""
    cfg = _cfg(request.param)
    full = lib.nunet_plan_create(C.byref(cfg))
    assert full, lib.nunet_last_error()
    pruned = {}
    for d in (1, 2, 3, 4):
        pruned[d] = lib.nunet_plan_create_pruned(C.byref(cfg), d)
        assert pruned[d], (d, lib.nunet_last_error())
    yield request.param, full, pruned
    for p in [full] + list(pruned.values()):
        lib.nunet_plan_destroy(p)


def test_version_is_unchanged(lib):
    assert lib.nunet_version() == 104


@pytest.mark.parametrize("depth,ds,unet", [(0, 1, 0), (5, 1, 0), (-1, 1, 0), (2, 0, 0), (2, 1, 1), (2, 0, 1)])
def test_bad_arguments_return_null_with_a_message(lib, depth, ds, unet):
    cfg = _cfg(1, ds, unet)
    # a successful creation first, so that the message read below is this call's
    ok = lib.nunet_plan_create(C.byref(_cfg()))
    assert ok
    lib.nunet_plan_destroy(ok)
    p = lib.nunet_plan_create_pruned(C.byref(cfg), depth)
    assert not p
    msg = lib.nunet_last_error().decode()
    assert msg.startswith("plan_create_pruned:") and len(msg) > len("plan_create_pruned: "), msg
    assert not lib.nunet_plan_create_pruned(None, 2) and lib.nunet_last_error()


def test_shape_rules_of_the_full_plan_hold(lib):
    """the multiple-of-16 rule on H and W stays, whatever the depth"""
    for bad in (L.PlanCfg(2, 40, 32, 3, 1, 1, L.F32, 0), L.PlanCfg(2, 32, 24, 3, 1, 1, L.F32, 0), L.PlanCfg(2, 8, 8, 3, 1, 1, L.F32, 0)):
        assert not lib.nunet_plan_create_pruned(C.byref(bad), 1)


def test_parameter_layout_is_the_full_models(lib, plans):
    _, full, pruned = plans
    assert lib.nunet_plan_depth(full) == 0 and lib.nunet_plan_num_heads(full) == 4
    for d, p in pruned.items():
        assert lib.nunet_plan_param_count(p) == lib.nunet_plan_param_count(full)
        assert lib.nunet_plan_bnbuf_count(p) == lib.nunet_plan_bnbuf_count(full)
        assert lib.nunet_plan_bn_layers(p) == lib.nunet_plan_bn_layers(full) == 30
        assert lib.nunet_plan_num_heads(p) == 1
        assert lib.nunet_plan_depth(p) == d
    assert lib.nunet_plan_depth(None) == 0


@pytest.mark.parametrize("dtype", [L.F32, L.BF16, L.F16])
def test_arena_grows_with_the_depth_and_stays_below_the_full_plans(lib, dtype):
    cfg = _cfg(4, dtype=dtype)
    full = lib.nunet_plan_create(C.byref(cfg))
    ps = [lib.nunet_plan_create_pruned(C.byref(cfg), d) for d in (1, 2, 3, 4)]
    sizes = [lib.nunet_plan_arena_bytes(p) for p in ps] + [lib.nunet_plan_arena_bytes(full)]
    for p in ps + [full]:
        lib.nunet_plan_destroy(p)
    print("arena bytes, depths 1..4 and the full plan:", sizes)
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] < sizes[4], sizes
    assert all(s % 256 == 0 for s in sizes)


def test_kept_blocks_are_the_anti_diagonals_up_to_the_depth(lib, plans):
    _, full, pruned = plans
    for d, p in pruned.items():
        for i in range(5):
            for j in range(5):
                pitch, ch = C.c_int32(-7), C.c_int32(-7)
                off = lib.nunet_plan_feature(p, i, j, C.byref(pitch), C.byref(ch))
                if i + j <= d:
                    assert off >= 0 and off % 16 == 0 and off < lib.nunet_plan_arena_bytes(p), (d, i, j, off)
                    # level i keeps depth + 1 - i slots of 32 * 2^i channels
                    assert ch.value == 32 << i and pitch.value == (d + 1 - i) * (32 << i), (d, i, j, pitch.value, ch.value)
                else:
                    assert off == -1 and pitch.value == -7, (d, i, j, off)
                assert lib.nunet_plan_feature_grad(p, i, j, None, None) == -1
    assert lib.nunet_plan_feature(full, 0, 4, None, None) >= 0 and lib.nunet_plan_feature_grad(full, 0, 4, None, None) >= 0


def test_training_entries_are_refused_before_any_pointer_is_read(lib, plans):
    """with NULL buffers: a refusal that came after the null-pointer check would answer "null pointer", one that dereferenced
    would crash - the message names the pruned plan"""
    _, full, pruned = plans
    p = pruned[2]
    opt = L.Optim(kind=L.OPT_SGD, momentum=0.9, lr=0x1000, state0=0x1000)      # a descriptor the entry accepts; never dereferenced
    off, b0, tot = C.c_int64(-3), C.c_int64(-3), C.c_int64(-3)
    calls = {
        "plan_forward": lambda: lib.nunet_plan_forward(p, None, None, None, None, None, 0, None, 1, None),
        "plan_forward 1|2": lambda: lib.nunet_plan_forward(p, None, None, None, None, None, 0, None, 3, None),
        "plan_backward": lambda: lib.nunet_plan_backward(p, None, None, None, 0, None, 0, None),
        "plan_backward_phase": lambda: lib.nunet_plan_backward_phase(p, None, None, None, 0, None, 0, 3, None),
        "plan_backward_phase open": lambda: lib.nunet_plan_backward_phase(p, None, None, None, 0, None, 0, 9, None),
        "plan_opt_step": lambda: lib.nunet_plan_opt_step(p, None, C.byref(opt), None, 0, 1.0, None, None),
        "plan_grad_sqnorm": lambda: lib.nunet_plan_grad_sqnorm(p, None, 0, None, 0, None),
        "plan_grad_scratch": lambda: lib.nunet_plan_grad_scratch(p, C.byref(off), C.byref(b0), C.byref(tot)),
        "plan_bucket0_wait": lambda: lib.nunet_plan_bucket0_wait(p, None),
        "plan_set_wgrad_dy": lambda: lib.nunet_plan_set_wgrad_dy(p, 1),
        "plan_block_act1": lambda: lib.nunet_plan_block_act1(p, None, None, 0, 0, 0, None, None),
    }
    for what, call in calls.items():
        assert call() == NUNET_EINVAL, what
        msg = lib.nunet_last_error().decode()
        assert "pruned to depth 2" in msg and msg.startswith(what.split()[0].replace("_phase", "") + ":"), (what, msg)
    assert (off.value, b0.value, tot.value) == (-3, -3, -3)
    assert lib.nunet_plan_grad_sqnorm_ws_bytes(p) == 0 and lib.nunet_plan_grad_sqnorm_ws_bytes(full) > 0
    # the entries that work as on a full plan (host state only)
    assert lib.nunet_plan_set_multistream(p, 0) == 0 and lib.nunet_plan_set_multistream(p, 1) == 0
    assert lib.nunet_plan_set_schedule(p, 2) == 0 and lib.nunet_plan_set_schedule(p, 0) == 0
    assert lib.nunet_plan_census_count(p, 0) == 0
    # ... and a full plan still answers these
    assert lib.nunet_plan_set_wgrad_dy(full, 0) == 0
    assert lib.nunet_plan_grad_scratch(full, C.byref(off), C.byref(b0), C.byref(tot)) == 0 and 0 < b0.value < tot.value


def test_eval_step_heads_argument_checks(lib):
    """every argument of nunet_eval_step_heads is checked on the host, before the first launch"""
    q = lib.nunet_eval_step_heads_ws_bytes
    assert q(3, 1, 257, 4, L.LOSS_BCE_DICE) > q(3, 1, 257, 1, L.LOSS_BCE_DICE) > 0
    assert q(3, 1, 257, 4, L.LOSS_BCE_DICE) % 256 == 0
    for n, k, hw, heads in ((0, 1, 257, 4), (3, 9, 257, 4), (3, 1, 0, 4), (3, 1, 257, 0), (3, 1, 257, 5)):
        assert q(n, k, hw, heads, L.LOSS_BCE_DICE) == 0, (n, k, hw, heads)
    one = C.c_void_p(256)      # never dereferenced: each call fails an argument check first
    for n, k, hw, heads, kind in ((3, 1, 257, 5, 0), (3, 1, 257, 0, 0), (3, 9, 257, 4, 0), (3, 1, (1 << 24) + 1, 4, 0), (0, 1, 257, 4, 0),
                                  (3, 1, 257, 4, 7), (3, 2, 257, 4, L.LOSS_LOVASZ_HINGE)):
        rc = lib.nunet_eval_step_heads(one, one, n, k, hw, heads, kind, one, 1 << 40, one, one, one, 0.0, None)
        assert rc == NUNET_EINVAL and lib.nunet_last_error().decode().startswith("eval_step_heads:"), (n, k, hw, heads, kind)
    assert lib.nunet_eval_step_heads(one, one, 3, 1, 257, 4, 0, one, 1 << 40, one, one, None, 0.0, None) == NUNET_EINVAL
    need = q(3, 1, 257, 4, L.LOSS_BCE_DICE)
    assert lib.nunet_eval_step_heads(one, one, 3, 1, 257, 4, 0, one, need - 1, one, one, one, 0.0, None) == NUNET_EINVAL
    assert "workspace" in lib.nunet_last_error().decode()
