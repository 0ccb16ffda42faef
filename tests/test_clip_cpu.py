"""Gradient-norm clipping, host side: the train.py flag, the ABI structs as _lib.py mirrors them, and argument validation of the
new entries that happens before any launch."""
import ctypes as C
import os
import subprocess
import sys

from nunet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_py_help_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--clip_grad_norm" in r.stdout


def test_optim_struct_grew_by_one_pointer():
    """nunet_optim: ... state0, state1, scaler, clip - the clip pointer is the trailing field."""
    names = [f[0] for f in L.Optim._fields_]
    assert names[-2:] == ["scaler", "clip"]
    before = type("OptimBefore", (C.Structure,), {"_fields_": L.Optim._fields_[:-1]})
    assert C.sizeof(L.Optim) == C.sizeof(before) + C.sizeof(C.c_void_p)
    assert L.Optim.clip.offset == L.Optim.scaler.offset + C.sizeof(C.c_void_p)


def test_clip_words():
    """nunet_clip is 32 bytes of device memory: 4 floats, one double, two int32."""
    assert L.CLIP_WORDS == 8
    hdr = open(os.path.join(ROOT, "include", "nunet.h")).read()
    body = hdr[hdr.index("typedef struct nunet_clip {"):hdr.index("} nunet_clip;")]
    assert body.count("float ") == 4 and body.count("double ") == 1 and "int32_t clipped, steps;" in body


def test_workspace_sizes_and_refusals():
    """The flat norm's grid is a pure function of n (one double per workgroup); null pointers, short workspaces and entries
    that cannot honour a clip are refused before any launch."""
    lib = L.lib()
    assert lib.nunet_grad_sqnorm_ws_bytes(0) == 0
    assert lib.nunet_grad_sqnorm_ws_bytes(1) == 8
    sizes = [lib.nunet_grad_sqnorm_ws_bytes(n) for n in (1, 8192, 8193, 1 << 20, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[2] == 16 and sizes[-1] % 8 == 0
    assert lib.nunet_grad_sqnorm_ws_bytes(1 << 20) == lib.nunet_grad_sqnorm_ws_bytes(1 << 20)
    assert lib.nunet_grad_sqnorm(None, 4, None, 8, None) != 0
    assert lib.nunet_grad_sqnorm(C.c_void_p(4096), 8193, C.c_void_p(8192), 15, None) != 0      # 16 bytes needed
    assert b"workspace" in lib.nunet_last_error()
    assert lib.nunet_clip_finalize(None, 1, 1.0, None, None, None) != 0
    assert lib.nunet_clip_finalize(C.c_void_p(4096), 0, 1.0, None, C.c_void_p(8192), None) != 0
    cfg = L.PlanCfg(2, 32, 32, 3, 4, 1, L.F32, 0)
    p = lib.nunet_plan_create(C.byref(cfg))
    try:
        nb = lib.nunet_plan_grad_sqnorm_ws_bytes(p)
        assert nb > 0 and nb % 8 == 0
        total = lib.nunet_plan_arena_bytes(p)
        assert lib.nunet_plan_grad_sqnorm(p, C.c_void_p(1 << 20), total, C.c_void_p(1 << 12), nb - 1, None) != 0
        assert b"workspace" in lib.nunet_last_error()
        assert lib.nunet_plan_grad_sqnorm(p, C.c_void_p(1 << 20), total - 1, C.c_void_p(1 << 12), nb, None) != 0
        opt = L.Optim(kind=L.OPT_ADAM, momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, nesterov=0,
                      lr=4096, adam_scal=4096, state0=4096, state1=4096, clip=4096)
        assert lib.nunet_adam_step(C.c_void_p(4096), C.c_void_p(4096), C.byref(opt), 16, 1.0, None) != 0
        assert b"clipping" in lib.nunet_last_error()
    finally:
        lib.nunet_plan_destroy(p)
