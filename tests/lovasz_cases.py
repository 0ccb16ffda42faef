"""Inputs and fp64 references for the Lovasz-hinge tests (tests/test_lovasz_cpu.py, tests/test_lovasz_gpu.py).

Tie-free by construction: per image P distinct integers k give the errors e = k * step - 3 in [-3, 5) (step = 2^-12 up to
2048 pixels, 2^-15 above, where the 2^18 grid points are exactly enough for 512 x 512), and the logits are
x = (1 - e) * (2t - 1). 1 - e is a multiple of step of magnitude <= 4 (at most 18 significant bits), so x is exact in fp32, and the
device's e = 1 - x * (2t - 1) is exact as well: the sign factor is +-1, the product is exact with or without an fma, and the
difference is again a multiple of step below 8. The fp32 and the fp64 sort orders are therefore the same and unique, and every
pixel can be compared with the fp64 reference on its own.

Every image of two or more pixels holds e == 0 (pixel 0), every image of three or more a negative error too (pixel 1), whatever
the draw."""
import functools

import numpy as np
import torch

# [N, H, W]; each is the smallest shape that reaches the path named next to it
SHAPES = [
    (2, 1, 1), (2, 1, 2), (3, 1, 63), (2, 1, 2047), (2, 1, 2048), (2, 1, 2049),   # in-LDS: fewer pixels than threads, odd counts, padding to 2048
    (3, 24, 40),                                                                  # in-LDS: 960 pixels, not a power of two
    (2, 1, 16383), (2, 128, 128),                                                 # in-LDS: the LDS limit, pixel index 16383 in the 15-bit field
    (2, 1, 16385),                                                                # global: two chunks, almost half of them padding
    (2, 128, 256),                                                                # global: two chunks, no padding
    (1, 1, 65537),                                                                # global: eight chunks, three merge stages with global passes
    (1, 512, 512),                                                                # global: the workload's geometry, 16 chunks
    (130, 8, 8),                                                                  # lovasz_mean_kernel strides past 64 images
    (33, 1, 16385),                                                               # lv_mean_kernel strides past 64 chunk partials (66)
]
PATTERNS = ["zero_one", "one_top", "one_bottom", "half_free", "all_nonpos"]
PATTERN_SHAPES = [(3, 24, 40), (2, 1, 16385)]
TIE_SHAPES = [(2, 24, 40), (2, 1, 16385)]
FUSED_SHAPE, FUSED_HEADS = (2, 1, 16385), 2

CASES = [(s, "p30") for s in SHAPES] + [(s, p) for s in PATTERN_SHAPES for p in PATTERNS]


def case_id(case):
    (n, h, w), pattern = case
    return "%dx%dx%d-%s" % (n, h, w, pattern)


def _seed(shape, pattern, salt):
    n, h, w = shape
    return (n * 1000003 + h * 10007 + w * 101 + sum(map(ord, pattern)) * 7 + salt) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def build(shape, pattern="p30", salt=0, labels_of=None):
    """-> (x fp32 [N, H, W], t fp32 [N, H, W], e fp64 [N, P]): logits, labels and the constructed errors.
    labels_of = (pattern, salt) takes the labels of that other case of the same shape (heads of one step share their target).
    The tensors are shared between tests: do not write to them."""
    n, h, w = shape
    p = h * w
    step = 2.0 ** -12 if p <= 2048 else 2.0 ** -15
    rng = np.random.default_rng(_seed(shape, pattern, salt))
    k_zero = int(round(3 / step))                               # e == 0
    hi = k_zero + 1 if pattern == "all_nonpos" else int(round(8 / step))
    e = np.empty((n, p))
    for i in range(n):
        k = rng.permutation(hi)[:p]
        fixed = [k_zero, k_zero - 5][:max(0, p - 1)]              # e == 0 at pixel 0 and, from 3 pixels on, a negative error at pixel 1
        k = np.concatenate([fixed, k[~np.isin(k, fixed)][:p - len(fixed)]]).astype(np.int64)
        if p == 1:
            k[0] = k_zero + (7 * (i + 1) if i % 2 == 0 else -7)     # one image with a positive error, one with a negative
        e[i] = k * step - 3
    assert e.min() >= -3 and e.max() < 5
    if labels_of is not None:
        t = build(shape, *labels_of)[1].reshape(n, p).double().numpy()
    else:
        t = (rng.random((n, p)) < 0.3).astype(np.float64)
        if pattern == "zero_one":
            t[0], t[1] = 0, 1
        elif pattern == "one_top":
            t[:] = 0
            t[np.arange(n), e.argmax(1)] = 1
        elif pattern == "one_bottom":
            t[:] = 0
            t[np.arange(n), e.argmin(1)] = 1
        elif pattern == "half_free":
            t[0, :p // 2] = 0
    x = (1 - e) * (2 * t - 1)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return torch.from_numpy(x32).reshape(n, h, w), torch.from_numpy(t.astype(np.float32)).reshape(n, h, w), torch.from_numpy(e)


@functools.lru_cache(maxsize=None)
def build_ties(shape, kind):
    """-> (x fp32, t fp32) with ties: "init" is x == 0 (every error is 1, the state at initialisation), "quarter" has the
    logits rounded to multiples of 0.25 (many tie groups of mixed labels, e == 0 among them)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, kind, 0))
    x = torch.round(torch.randn(n, h, w, generator=g) * 2 * 4) / 4
    t = (torch.rand(n, h, w, generator=g) < 0.3).float()
    if kind == "init":
        x = torch.zeros(n, h, w)
    return x, t


def oracle(x, t):
    """oracle.lovasz_hinge and its gradient on fp64 copies of the inputs -> (loss: float, dx: fp64 [N, P])"""
    from oracle import nunet_oracle as O
    xo = x.double().requires_grad_(True)
    loss = O.lovasz_hinge(xo, t.double())
    loss.backward()
    return float(loss.detach()), xo.grad.reshape(x.shape[0], -1)


@functools.lru_cache(maxsize=None)
def reference(shape, pattern="p30", salt=0, labels_of=None):
    """oracle() of build(...), computed once per case"""
    x, t, _ = build(shape, pattern, salt, labels_of)
    return oracle(x, t)


@functools.lru_cache(maxsize=None)
def reference_ties(shape, kind):
    return oracle(*build_ties(shape, kind))


def closed_form(e, t):
    """The Jaccard increments without the difference of two numbers near 1, in fp64. With k 1-based in descending order of e,
    cum the inclusive count of positives, I_k = gts - cum_k and U_k = gts + k - cum_k:
        g_1 = 1 - I_1 / U_1;   k > 1: g_k = 1 / U_k at a positive, I_k / (U_{k-1} U_k) at a negative (U_{k-1} = U_k - 1).
    e: fp64 [N, P] without ties inside an image, t: [N, P] of 0 / 1.
    -> (loss: float, dx fp64 [N, P], zero: bool [N, P], the pixels whose gradient is exactly zero: e <= 0, or a negative
    sorted after the last positive (I_k = 0, k > 1))."""
    e = e.numpy() if torch.is_tensor(e) else e
    t = t.double().numpy() if torch.is_tensor(t) else t
    n, p = e.shape
    loss, dx, zero = 0.0, np.zeros((n, p)), np.zeros((n, p), bool)
    for i in range(n):
        order = np.argsort(-e[i], kind="stable")
        es, lab = e[i][order], t[i][order]
        cum = np.cumsum(lab)
        gts = cum[-1]
        k = np.arange(1, p + 1, dtype=np.float64)
        I, U = gts - cum, gts + k - cum
        g = np.where(lab == 1, 1 / U, I / (np.maximum(U - 1, 1) * U))
        g[0] = 1 - I[0] / U[0]
        on = es > 0
        loss += float(np.sum(es[on] * g[on]))
        dx[i, order] = np.where(on, -(2 * lab - 1) * g, 0.0) / n
        zero[i, order] = ~on | ((lab == 0) & (I == 0) & (k > 1))
    return loss / n, dx, zero


def worst_rel(got, ref):
    """max |got - ref| / |ref| over the entries with ref != 0 (0.0 if there are none); fp64 arrays"""
    nz = ref != 0
    return float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
