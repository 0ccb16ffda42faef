"""Cases, the fp64 reference, the per-element gradient bound and an fp32 emulation for the BCEWithLogitsLoss tests
(tests/test_bce_logits_cpu.py, tests/test_bce_logits_gpu.py). Nothing here touches a GPU. Inputs come from tests/loss_cases.py
(LC.build / LC.head): a case is its tuple (kind, N, per, heads, pattern).

kind "alone" is the stand-alone pair nunet_bce_logits_fwd / _bwd, which sees a flat n = N * per elements; its shape cases have
N = 1. Both launches run gx = min(256, ceil(n / 256)) blocks of 256 threads, one grid-stride loop: one element per thread up to
n = 65536, n / 65536 trips above. kind "fused" is nunet_loss_step with NUNET_LOSS_BCE_LOGITS, whose first launch runs on the grid
of the BCE-Dice kind, min(64, ceil(per / 256)) blocks per (image, head): the fused cases are LC.FUSED_CASES themselves. Next to
every stand-alone size stands (gx, most trips, fewest trips), the regime it is the smallest size to reach.

The loss is torch.nn.BCEWithLogitsLoss() with its defaults: the mean over all count = N * per elements of
    l_i = max(x_i, 0) - x_i t_i + log1p(exp(-|x_i|)),        dx_i = (p_i - t_i) k,     p = sigmoid(x), k = 1 / count.
The gradient is a single term, so nothing cancels between addends whatever the targets are; the only absolute error is the
sigmoid's, 2^-24 p (2^-126 covers a denormal or flushed p below x = -87):
    |dx_i - ref_i| <= factor (1e-6 |ref_i| + c (2^-24 p_i + 2^-126) k),
factor = 1 / heads times any upstream scale. Targets uniform in [0, 1] ("soft_uniform") are held to the SAME bound. The fp32
emulation on the CPU is pinned at c = 2, the device at c = 4 (an expf, log1pf or reciprocal one ulp off the host's), the margins
of the BCE-Dice tests; the loss at |got - ref| <= 2e-6 max(1, |ref|)."""
import functools

import torch
import torch.nn.functional as F

import loss_cases as LC

ALONE_CAP = 256
# n: (gx, most trips, fewest trips)
ALONE_SIZES = {
    1: (1, 1, 0),                       # one element, 255 idle threads
    255: (1, 1, 0),                     # one block, not full
    257: (2, 1, 0),                     # a second block with one element (n % 4 == 1)
    1022: (4, 1, 0),                    # n % 4 == 2
    1023: (4, 1, 0),                    # n % 4 == 3
    65536: (256, 1, 1),                 # the block cap exactly, one element per thread
    65537: (256, 2, 1),                 # cap plus one element: thread 0 of block 0 takes a second trip
    2 ** 22 + 3: (256, 65, 64),         # 64 trips for every thread, one more for three
}
ALONE_PATTERN_SHAPE = LC.ALONE_PATTERN_SHAPE[:2]        # 3 x 9216 = 27648 elements: 108 blocks, one element per thread
MISALIGNED_SIZE = 1023                                  # the case the GPU test also runs 4 bytes off a 16-byte boundary

REGIME = {}


def _alone(n_img, per, pattern, regime):
    case = ("alone", n_img, per, 1, pattern)
    REGIME[case] = regime
    return case


ALONE_SHAPE_CASES = [_alone(1, n, "rand", r) for n, r in ALONE_SIZES.items()]
ALONE_PATTERN_CASES = [_alone(*ALONE_PATTERN_SHAPE, p, (108, 1, 1)) for p in LC.PATTERNS + ["soft_uniform"]]
ALONE_CASES = ALONE_SHAPE_CASES + ALONE_PATTERN_CASES
FUSED_CASES = LC.FUSED_CASES + [c for c in LC.SOFT_UNIFORM_CASES if c[0] == "fused"]
for _c in FUSED_CASES:
    REGIME[_c] = LC.REGIME[_c]
CASES = ALONE_CASES + FUSED_CASES


def count(case):
    return case[1] * case[2]


def expected_regime(kind, size):
    """(gx, most trips, fewest trips) from the formulas in this module's docstring; size = n stand-alone, per fused"""
    if kind == "fused":
        return LC.expected_regime(kind, size)
    gx = min(ALONE_CAP, -(-size // 256))
    return gx, -(-size // (gx * 256)), size // (gx * 256)


def oracle(x, t):
    """torch's own binary_cross_entropy_with_logits (mean) on fp64 copies, through autograd on the CPU
    -> (loss: float, dx fp64 of x's shape)"""
    xo = x.double().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xo, t.double())
    loss.backward()
    return float(loss.detach()), xo.grad


@functools.lru_cache(maxsize=None)
def reference(case, k=0):
    """oracle() of head k of LC.build(case), computed once: shared, do not write to it"""
    return oracle(LC.head(case, k), LC.build(case)[1])


def bound_unit(x):
    """the absolute term of the bound for c = 1, one head and no upstream scale: fp64 of x's shape"""
    return (2.0 ** -24 * torch.sigmoid(x.double()) + 2.0 ** -126) / x.numel()


@functools.lru_cache(maxsize=None)
def unit_of(case, k=0):
    return bound_unit(LC.head(case, k))


def worst_ratio(got, ref, unit, factor=1.0):
    """the smallest c for which every element of `got` is within factor (1e-6 |ref| + c unit) of factor ref (fp64 tensors)"""
    return LC.worst_ratio(got, ref, unit, factor)


def emulate_fp32(x, t, heads=1):
    """The kernels' formulas in torch fp32 on the CPU, multiplies in the kernels' order; the sum is torch's.
    -> (loss: float, dx fp32 of x's shape, as the loss step stores it for one of `heads` heads)"""
    f = torch.float32
    x, t = x.to(f), t.to(f)
    one = torch.tensor(1.0, dtype=f)
    cnt = torch.tensor(float(x.numel()), dtype=f)
    p = one / (one + torch.exp(-x))
    loss = (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum() / cnt
    k = one / (cnt * torch.tensor(float(heads), dtype=f))
    dx = (p - t) * k
    assert dx.dtype == f and loss.dtype == f
    return float(loss), dx
