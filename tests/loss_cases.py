"""Inputs, the fp64 reference, the per-pixel gradient bound and an fp32 emulation for the BCE-Dice tests
(tests/test_bce_dice_cpu.py, tests/test_bce_dice_gpu.py). Nothing here touches a GPU.

A case is (kind, N, per, heads, pattern): kind "alone" is the stand-alone loss (nunet_bce_dice_fwd / _bwd), "fused" the
BCE-Dice nunet_loss_step; per = K * H * W elements per image. Next to every shape stands the launch regime it is there for,
(gx, most trips, fewest trips) of the grid-stride loops: gx = min(64, ceil(per / 1024)) blocks per image stand-alone,
min(64, ceil(per / 256)) fused, 256 threads each. test_bce_dice_cpu.py holds these figures against the formulas,
test_bce_dice_gpu.py against the library's own answer (nunet_loss_launch_info).

The gradient criterion. With p = sigmoid(x), I = sum p t, P = sum p, T = sum t per image, D = P + T + 1e-5, num = 2 I + 1e-5,
    dx_i = kb (p_i - t_i) - (1 / N) (2 t_i D - num) / D^2 * p_i (1 - p_i),      kb = 0.5 / (N per)
and the kernels evaluate exactly this in fp32. Every factor but one carries a relative fp32 error; the sigmoid carries an
absolute one: p (1 - p) and p - t are formed from a p that is off by 2^-24 p, so for x >~ 17, where the fp32 sigmoid is exactly
1, the computed gradient of a foreground pixel is exactly 0 and its relative error 1. The two terms have the same sign for
either hard label (t = 1: both negative, t = 0: both positive), so nothing cancels, and
    bound_i = 1e-6 |ref_i| + c (2^-24 p_i + 2^-126) (kb + coef_i / N),      coef_i = |2 t_i D - num| / D^2
times 1 / heads and any upstream scale; 2^-126 covers a denormal or flushed p below x = -87.

Soft targets. For 0 < t < 1 the two terms have the same sign only while t lies outside the interval between p and
t* = num / (2 D), which is at most 1/2 (2 I <= P + T). Targets uniform in [0, 1] put pixels inside it, where the terms cancel and
the fp32 evaluation needs c between 2.1 and 2.8 (four draws on the two pattern shapes), so the "soft" pattern keeps the derivation's premise
instead: foreground pixels whose logit is negative get a target uniform in (0.5, 1] (p < 1/2 < t and t* <= 1/2 < t: both terms
negative), every other pixel keeps its hard label. Fractional targets still pass through every product of the kernels
(x t, p t, 2 t D).

Targets uniform in [0, 1] stay as the extra pattern "soft_uniform" (SOFT_UNIFORM_CASES, not part of CASES) under the criterion
that allows for the cancellation: the relative part is taken of the sum of the magnitudes of all four addends,
    m_i = kb (p_i + t_i) + (1 / N) (2 t_i D + num) / D^2 * p_i (1 - p_i),      |dx_i - ref_i| <= 1e-6 m_i + c unit_i,
since each addend carries a relative error of a few 2^-24 whatever the others do. For hard labels this is the laxer bound (by
up to (1 + p) / (1 - p) at a foreground pixel), which is why the other cases do not use it."""
import functools

import numpy as np
import torch

# (N, per, gx, most trips, fewest trips); each is the smallest shape that reaches the regime named next to it
ALONE_SHAPES = [
    (2, 1, 1, 1, 0),                    # one element, 255 idle threads
    (3, 255, 1, 1, 0),                  # one block, not full
    (2, 1025, 2, 3, 2),                 # a second block and its partial slab; element 1024 is block 0's third trip
    (3, 2240, 3, 3, 2),                 # three blocks, uneven trips
    (2, 65536, 64, 4, 4),               # the block cap, four trips, no tail
    (2, 65537, 64, 5, 4),               # a fifth trip for one thread
    (1, 2 ** 20 + 3, 64, 65, 64),       # 64 trips and three threads with one more
    (33, 300, 1, 2, 1),                 # bce_dice_final_kernel's serial loop over images
]
FUSED_SHAPES = [
    (2, 1, 1, 1, 0),
    (3, 257, 2, 1, 0),                  # a second block with one element
    (3, 2240, 9, 1, 0),                 # the shape tests/test_ops_gpu.py runs
    (2, 16384, 64, 1, 1),               # the block cap, one element per thread
    (2, 16385, 64, 2, 1),               # a second trip for one thread
    (2, 65537, 64, 5, 4),               # 256 x 256 and one: a fifth trip
] + [(n, 300, 2, 1, 0) for n in (1, 4, 5, 16, 17, 33)]    # the owning block: one image, one per wave, unequal counts, a full pass, a second and a third pass
FUSED_HEADS_SHAPE, FUSED_HEADS = (5, 16385, 64, 2, 1), (2, 4, 8)
PATTERNS = ["empty_full", "saturated", "wide", "beyond_exp", "soft", "zeros"]
ALONE_PATTERN_SHAPE = (3, 9216, 9, 4, 4)
FUSED_PATTERN_SHAPE = (3, 16385, 64, 2, 1)

REGIME = {}


def _case(kind, shape, heads=1, pattern="rand"):
    case = (kind, shape[0], shape[1], heads, pattern)
    REGIME[case] = tuple(shape[2:])
    return case


ALONE_CASES = [_case("alone", s) for s in ALONE_SHAPES] + [_case("alone", ALONE_PATTERN_SHAPE, 1, p) for p in PATTERNS]
FUSED_CASES = ([_case("fused", s) for s in FUSED_SHAPES] + [_case("fused", FUSED_HEADS_SHAPE, h) for h in FUSED_HEADS]
               + [_case("fused", FUSED_PATTERN_SHAPE, 1, p) for p in PATTERNS])
CASES = ALONE_CASES + FUSED_CASES
SOFT_UNIFORM_CASES = [_case("alone", ALONE_PATTERN_SHAPE, 1, "soft_uniform"), _case("fused", FUSED_PATTERN_SHAPE, 1, "soft_uniform")]
EDGE_CASE = ("fused", 5, 16385, 4, "rand")      # its last head carries the sigmoid-threshold edge values (any fused "rand" case of 257 or more elements does)


def case_id(case):
    kind, n, per, heads, pattern = case
    return "%s-%dx%d-h%d-%s" % (kind, n, per, heads, pattern)


def expected_regime(kind, per):
    """(gx, most trips, fewest trips) from the formulas in this module's docstring"""
    gx = min(64, -(-per // (1024 if kind == "alone" else 256)))
    return gx, -(-per // (gx * 256)), per // (gx * 256)


def iou_edges():
    """logits around the smallest one whose fp32 sigmoid exceeds 0.5 (tests/test_ops_gpu.py::test_iou_counts_at_the_sigmoid_threshold,
    the finite ones), then a ramp across it: 235 values"""
    from nunet_amd.metrics import iou_logit_threshold
    f32 = np.float32
    thr = iou_logit_threshold()
    below, above = float(np.nextafter(f32(thr), f32(0))), float(np.nextafter(f32(thr), f32(1)))
    edges = [0.0, -0.0, 1e-30, 1e-12, 1e-9, 2e-8, 5.9e-8, 6e-8, below, thr, above, 1e-7, 1.2e-7, 1e-6, -thr, -1e-9, 1.0, -1.0]
    return np.concatenate([np.array(edges, f32), np.linspace(-3e-7, 3e-7, 235 - len(edges)).astype(f32)])


@functools.lru_cache(maxsize=None)
def build(case):
    """-> (x fp32 [heads, N, per] for a fused case, [N, per] for a stand-alone one; t fp32 [N, per]). Every head has its own
    logits, all share the target. The tensors are shared between tests: do not write to them."""
    kind, n, per, heads, pattern = case
    seed = (n * 1000003 + per * 10007 + heads * 101 + sum(map(ord, kind + pattern)) * 7) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(heads, n, per, generator=g) * 2
    t = (torch.rand(n, per, generator=g) < 0.4).float()
    if pattern == "empty_full":
        t[0], t[1] = 0, 1
    elif pattern == "saturated":
        x[:, 0], t[0] = -30, 0
        x[:, 1], t[1] = 30, 1
        x[:, 2], t[2] = -30, 1
    elif pattern == "wide":
        x = x * 20                                  # N(0, 40^2)
    elif pattern == "beyond_exp":
        x[:, 0], x[:, 1] = -95, 95
        x[:, 2, :per // 2] = -88.5
    elif pattern == "soft":
        frac = 0.5 + 0.5 * (1 - torch.rand(n, per, generator=g))         # (0.5, 1]
        t = torch.where((t == 1) & (x[-1] < 0), frac, t)
    elif pattern == "soft_uniform":
        t = torch.rand(n, per, generator=g)
    elif pattern == "zeros":
        x = torch.zeros(heads, n, per)
    else:
        assert pattern == "rand", pattern
        if kind == "fused" and per >= 257:
            x[-1, 0, :235] = torch.from_numpy(iou_edges())
    assert bool(torch.isfinite(x).all())
    return (x if kind == "fused" else x[0]), t


def head(case, k):
    """logits [N, per] of head k (stand-alone cases have one)"""
    x, _ = build(case)
    return x[k] if case[0] == "fused" else x


def oracle(x, t):
    """BCE-Dice (oracle.bce_dice_loss, the reference's losses.py:107-117) on fp64 copies of x, t [N, per], through autograd
    -> (loss: float, dx fp64 [N, per], I, P, T: fp64 [N], the per-image sums of p t, p and t)"""
    from oracle import nunet_oracle as O
    xo, td = x.double().requires_grad_(True), t.double()
    loss = O.bce_dice_loss(xo, td)
    loss.backward()
    p = torch.sigmoid(x.double())
    return float(loss.detach()), xo.grad, (p * td).sum(1), p.sum(1), td.sum(1)


@functools.lru_cache(maxsize=None)
def reference(case, k=0):
    """oracle() of head k of build(case), computed once"""
    return oracle(head(case, k), build(case)[1])


def bound_unit(x, t):
    """the absolute term of the bound for c = 1, heads = 1 and no upstream scale: fp64 [N, per]"""
    n, per = x.shape
    xd, td = x.double(), t.double()
    p = torch.sigmoid(xd)
    I, P, T = (p * td).sum(1, keepdim=True), p.sum(1, keepdim=True), td.sum(1, keepdim=True)
    D, num = P + T + 1e-5, 2 * I + 1e-5
    coef = (2 * td * D - num).abs() / (D * D)
    kb = 0.5 / (n * per)
    return (2.0 ** -24 * p + 2.0 ** -126) * (kb + coef / n)


def addend_magnitudes(x, t):
    """m of the module docstring, for one head and no upstream scale: fp64 [N, per]"""
    n, per = x.shape
    xd, td = x.double(), t.double()
    p = torch.sigmoid(xd)
    I, P, T = (p * td).sum(1, keepdim=True), p.sum(1, keepdim=True), td.sum(1, keepdim=True)
    D, num = P + T + 1e-5, 2 * I + 1e-5
    return 0.5 / (n * per) * (p + td) + (2 * td * D + num) / (D * D) * p * (1 - p) / n


@functools.lru_cache(maxsize=None)
def unit_of(case, k=0):
    return bound_unit(head(case, k), build(case)[1])


def worst_ratio(got, ref, unit, factor=1.0, rel=None):
    """The smallest c for which every pixel of `got` is within factor * (1e-6 |ref| + c unit) of factor * ref (fp64 tensors;
    ref and unit are those of the unscaled single-head loss). rel: what the 1e-6 is taken of in place of |ref|
    (addend_magnitudes, for the soft_uniform cases)."""
    excess = (got - factor * ref).abs() - 1e-6 * factor * (ref.abs() if rel is None else rel)
    return float((excess.clamp(min=0) / (factor * unit)).max())


def emulate_fp32(x, t):
    """The kernels' formulas in torch fp32 on the CPU, multiplies in the kernels' order; the sums are torch's.
    -> (loss: float, dx fp32 [N, per], I, P, T: fp32 [N])"""
    f = torch.float32
    n, per = x.shape
    x, t = x.to(f), t.to(f)
    one, smooth = torch.tensor(1.0, dtype=f), torch.tensor(1e-5, dtype=f)
    p = one / (one + torch.exp(-x))
    I, P, T = (p * t).sum(1), p.sum(1), t.sum(1)
    bce = (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum()
    nf, pf = torch.tensor(float(n), dtype=f), torch.tensor(float(per), dtype=f)
    d = ((2 * I + smooth) / (P + T + smooth)).sum()
    loss = 0.5 * (bce / (nf * pf)) + (one - d / nf)
    D = (P + T + smooth)[:, None]
    num = (2 * I + smooth)[:, None]
    kb = torch.tensor(0.5, dtype=f) / (nf * pf)
    inv_d2, inv_n = one / (D * D), one / nf
    ddice = (2 * t * D - num) * inv_d2 * p * (one - p)
    dx = kb * (p - t) - inv_n * ddice
    assert dx.dtype == f and loss.dtype == f
    return float(loss), dx, I, P, T
