"""CPU-side checks of BCEWithLogitsLoss, the reference's third `--loss` (trains.py:27-28,210-211): tests/bce_logits_cases.py, the
module the GPU tests (tests/test_bce_logits_gpu.py) stand on, claims the launch regimes the grid formulas give and the library's
own nunet_loss_launch_info answers; an fp32 evaluation of the kernels' formulas stays within the per-element gradient bound
with c = 2, half of what the GPU test allows the device; the entries refuse bad arguments on the host, before any launch; the
command line takes the name and `losses.__all__` stays the reference's."""
import ctypes as C

import pytest
import torch

import loss_cases as LC
import bce_logits_cases as BC
from nunet_amd import _lib as L

C_EMULATION = 2.0
EINVAL = -1
# every input the BCE-Dice tests use goes through this loss as well
EMULATION_CASES = BC.CASES + [c for c in LC.CASES + LC.SOFT_UNIFORM_CASES if c not in BC.CASES]


def test_case_list_reaches_every_regime():
    """the claimed figures are the formulas', and the stand-alone list holds what it is for: one element, one partial block, a
    second block with one element, the cap exactly and plus one, 64 trips and more, every n % 4, the patterns on one shape"""
    for case in BC.CASES:
        kind, n, per, heads, _ = case
        assert BC.REGIME[case] == BC.expected_regime(kind, BC.count(case) if kind == "alone" else per), case
    sizes = {BC.count(c): BC.REGIME[c] for c in BC.ALONE_SHAPE_CASES}
    assert sizes[1] == (1, 1, 0) and sizes[255] == (1, 1, 0) and sizes[257] == (2, 1, 0)
    assert sizes[65536] == (BC.ALONE_CAP, 1, 1) and sizes[65537] == (BC.ALONE_CAP, 2, 1)
    assert BC.expected_regime("alone", 256)[0] == 1 and BC.expected_regime("alone", 65536 - 256)[0] == BC.ALONE_CAP - 1      # the smallest sizes of their regimes
    assert any(r[2] >= 64 and r[1] > r[2] for r in sizes.values())
    assert {n % 4 for n in sizes} == {0, 1, 2, 3} and BC.MISALIGNED_SIZE in sizes
    assert {c[4] for c in BC.ALONE_PATTERN_CASES} == set(LC.PATTERNS) | {"soft_uniform"}
    assert set(LC.FUSED_CASES) < set(BC.FUSED_CASES) and LC.EDGE_CASE in BC.FUSED_CASES
    assert any(c[4] == "soft_uniform" for c in BC.FUSED_CASES)
    assert len(set(BC.CASES)) == len(BC.CASES)


@pytest.mark.parametrize("case", EMULATION_CASES, ids=LC.case_id)
def test_fp32_emulation_stays_within_the_bound(case):
    """c = 2 for the kernels' formulas in fp32 with the host's exp / log1p and torch's sum - the uniform soft targets under the
    same bound as every other case; the loss within 2e-6. The ratio printed is the smallest c that would pass."""
    t = LC.build(case)[1]
    heads = case[3]
    for k in range(heads):
        x = LC.head(case, k)
        ref_loss, ref_dx = BC.reference(case, k)
        loss, dx = BC.emulate_fp32(x, t, heads)
        ratio = BC.worst_ratio(dx.double(), ref_dx, BC.unit_of(case, k), 1.0 / heads)
        print("%s head %d: emulation needs c = %.3f; |loss - ref| / max(1, |ref|) = %.2e"
              % (LC.case_id(case), k, ratio, abs(loss - ref_loss) / max(1.0, abs(ref_loss))))
        assert ratio <= C_EMULATION
        assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))


def test_reference_is_the_closed_form():
    """the fp64 reference (torch's kernel through autograd) against the definition written out: the mean of
    max(x, 0) - x t + log1p(exp(-|x|)) and (sigmoid(x) - t) / count"""
    case = ("alone",) + BC.ALONE_PATTERN_SHAPE + (1, "soft_uniform")
    x, t = (v.double() for v in LC.build(case))
    loss, dx = BC.reference(case)
    assert abs(loss - float((x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean())) < 1e-14
    assert float((dx - (torch.sigmoid(x) - t) / x.numel()).abs().max()) < 1e-18


def test_launch_info_query_on_the_host():
    """nunet_loss_launch_info, entries 5 and 6: the regime every stand-alone case claims, whatever N and heads say; the items
    covered over a sweep of sizes; the loss step's entry describes kind 2's first launch (the grid of kind 0); entry 7 and
    negative entries stay refused"""
    lib = L.lib()
    assert (L.LOSS_ENTRY_BCE_LOGITS_FWD, L.LOSS_ENTRY_BCE_LOGITS_BWD, L.LOSS_BCE_LOGITS) == (5, 6, 2)
    assert lib.nunet_version() == 104
    o = L.LossLaunchInfo()
    for case in BC.ALONE_CASES:
        n = BC.count(case)
        for entry in (L.LOSS_ENTRY_BCE_LOGITS_FWD, L.LOSS_ENTRY_BCE_LOGITS_BWD):
            for n_img, heads in ((1, 1), (0, 0), (7, 9)):
                assert lib.nunet_loss_launch_info(entry, n_img, n, heads, C.byref(o)) == 0
                assert (o.grid_x, o.trips_max, o.trips_min) == BC.REGIME[case] and (o.grid_y, o.grid_z, o.block, o.items) == (1, 1, 256, n)
                assert lib.nunet_bce_logits_ws_bytes(n) == 4 * o.grid_x
    for entry in (L.LOSS_ENTRY_BCE_LOGITS_FWD, L.LOSS_ENTRY_BCE_LOGITS_BWD):
        for size in [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 2 ** 21 + 3073, 2 ** 24 + 1, 2 ** 31 + 5]:
            assert lib.nunet_loss_launch_info(entry, 1, size, 1, C.byref(o)) == 0
            threads = o.grid_x * o.block
            assert 1 <= o.grid_x <= BC.ALONE_CAP and o.items == size and (o.grid_x, o.trips_max, o.trips_min) == BC.expected_regime("alone", size)
            assert o.trips_min * threads <= size <= o.trips_max * threads and o.trips_max - o.trips_min <= 1
            assert o.grid_x == BC.ALONE_CAP or o.trips_max == 1
        assert lib.nunet_loss_launch_info(entry, 1, 0, 1, C.byref(o)) == EINVAL and lib.nunet_last_error()
        assert lib.nunet_loss_launch_info(entry, 1, 5, 1, None) == EINVAL
    for case in BC.FUSED_CASES:
        _, n, per, heads, _ = case
        assert lib.nunet_loss_launch_info(L.LOSS_ENTRY_LOSS_STEP, n, per, heads, C.byref(o)) == 0
        assert (o.grid_x, o.trips_max, o.trips_min) == BC.REGIME[case] and (o.grid_y, o.grid_z, o.block, o.items) == (n, heads, 256, per)
    for bad in (7, 8, -1, -5):
        assert lib.nunet_loss_launch_info(bad, 1, 5, 1, C.byref(o)) == EINVAL and b"entry" in lib.nunet_last_error()


def test_workspace_sizes():
    """the stated sizes: one float per block stand-alone (0 for no elements), three floats per slab of the loss step's kind 2;
    kinds 0 and 1 answer what they answered"""
    lib = L.lib()
    assert lib.nunet_bce_logits_ws_bytes(0) == 0 and lib.nunet_bce_logits_ws_bytes(-3) == 0
    assert lib.nunet_bce_logits_ws_bytes(1) == 4 and lib.nunet_bce_logits_ws_bytes(2 ** 33) == 4 * BC.ALONE_CAP
    for n, per, heads in ((1, 1, 1), (4, 1024, 1), (16, 96 * 96, 4), (3, 2 ** 24, 8)):
        assert lib.nunet_loss_step_ws_bytes(n, per, heads, L.LOSS_BCE_LOGITS) == heads * n * 64 * 3 * 4 > 0
        assert lib.nunet_loss_step_ws_bytes(n, per, heads, L.LOSS_BCE_DICE) == heads * n * 64 * 6 * 4
    assert lib.nunet_loss_step_ws_bytes(4, 1024, 1, L.LOSS_LOVASZ_HINGE) > 0
    for bad in ((0, 5, 1), (1, 0, 1), (1, 5, 0)):
        assert lib.nunet_loss_step_ws_bytes(*bad, L.LOSS_BCE_LOGITS) == 0


def test_bad_arguments_are_refused_on_the_host():
    """NUNET_EINVAL with a message before any launch (the pointers are never dereferenced: no GPU is needed): null pointers,
    n <= 0, a short workspace - named after the query that states the size - and a loss kind the step does not have"""
    lib = L.lib()
    p = C.c_void_p(256)          # a non-null address nothing reads
    n = 1000
    need = lib.nunet_bce_logits_ws_bytes(n)
    assert need == 16
    for args in ((None, p, n, p, need, p), (p, None, n, p, need, p), (p, p, n, None, need, p), (p, p, n, p, need, None), (p, p, 0, p, need, p),
                 (p, p, -4, p, need, p)):
        assert lib.nunet_bce_logits_fwd(*args, None) == EINVAL and b"bce_logits_fwd: bad args" in lib.nunet_last_error()
    for short in (0, need - 1):
        assert lib.nunet_bce_logits_fwd(p, p, n, p, short, p, None) == EINVAL
        msg = lib.nunet_last_error()
        assert b"bce_logits_fwd" in msg and b"nunet_bce_logits_ws_bytes" in msg and str(need).encode() in msg, msg
    for args in ((None, p, n, None, p), (p, None, n, None, p), (p, p, n, None, None), (p, p, 0, None, p), (p, p, -1, p, p)):
        assert lib.nunet_bce_logits_bwd(*args, None) == EINVAL and b"bce_logits_bwd: bad args" in lib.nunet_last_error()
    # the loss step: kind 3 does not exist; kind 2 checks its workspace and its image size like the others
    step = lambda kind, per, ws_bytes: lib.nunet_loss_step(p, p, 2, per, 1, kind, p, ws_bytes, p, p, None, 0.0, None)
    big = 1 << 30
    assert step(3, 100, big) == EINVAL and b"loss_kind 3" in lib.nunet_last_error()
    assert step(-1, 100, big) == EINVAL and b"loss_kind -1" in lib.nunet_last_error()
    need = lib.nunet_loss_step_ws_bytes(2, 100, 1, L.LOSS_BCE_LOGITS)
    assert step(L.LOSS_BCE_LOGITS, 100, need - 1) == EINVAL
    msg = lib.nunet_last_error()
    assert b"nunet_loss_step_ws_bytes" in msg and str(need).encode() in msg, msg
    assert step(L.LOSS_BCE_LOGITS, 2 ** 24 + 1, big) == EINVAL and b"image too large" in lib.nunet_last_error()
    assert lib.nunet_loss_step_scaled(p, p, 2, 100, 1, L.LOSS_BCE_LOGITS, p, need, p, p, None, 0.0, None, None) == EINVAL
    assert b"seed_scale" in lib.nunet_last_error()


def test_train_py_takes_the_name_and_the_module_list_stays_the_reference(monkeypatch):
    """`--loss BCEWithLogitsLoss` parses (trains.py:27-28 appends the name to its choices); nunet_amd.losses has the class and
    keeps it out of __all__, as the reference's losses module does"""
    import importlib.util
    import os
    import nunet_amd
    spec = importlib.util.spec_from_file_location("nunet_train_driver", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    monkeypatch.setattr("sys.argv", ["train.py", "--loss", "BCEWithLogitsLoss"])
    assert vars(train.parse_args())["loss"] == "BCEWithLogitsLoss"
    assert train.LOSS_NAMES == ["BCEDiceLoss", "LovaszHingeLoss", "BCEWithLogitsLoss"]
    assert train.LOSS_NAMES is not nunet_amd.losses.__all__
    assert nunet_amd.losses.__all__ == ["BCEDiceLoss", "LovaszHingeLoss"]
    crit = getattr(nunet_amd.losses, "BCEWithLogitsLoss")()
    assert isinstance(crit, torch.nn.Module) and not list(crit.parameters())
    with pytest.raises(L.NunetError):
        crit(torch.zeros(2, 3), torch.zeros(2, 3))          # CPU tensors: no silent fallback
