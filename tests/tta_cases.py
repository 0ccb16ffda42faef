"""numpy restatement of test-time augmentation (EvalStep(tta=...), nunet_dihedral_nchw, nunet_tta_merge; include/nunet.h),
independent of the kernels' index function and of its Python twins in tests/pipeline_cases.py.

Geometry. code = rot90 count (bits 0-1, counter-clockwise like np.rot90) | hflip (bit 2) | vflip (bit 3). view() states the
map FORWARD with library calls on the last two axes of an [..., H, W] array, in the reference transform's order: rotate,
then flip horizontally, then flip vertically. unview() applies the inverses in the opposite order.

Merges. A merge takes the views' logits, each in ITS view frame, in view order:
  merge_logit   un-view each, fp32 sum in view order starting FROM the first view (no 0 + v0: -0 stays -0), one fp32 division
                by the number of views: what the device must produce bit for bit;
  merge_prob64  the definition in fp64: mean of the sigmoids, clamped to [2^-23, 1 - 2^-23], log(p) - log1p(-p);
  merge_prob32  the same formula with one np.float32 ufunc per operation: the yardstick of what fp32 arithmetic costs.
"""
import numpy as np

FLIPS = (0, 4, 8, 12)
D4 = (0, 1, 2, 3, 4, 5, 6, 7)
ALL_CODES = tuple(range(16))
EVEN_CODES = tuple(c for c in range(16) if not c & 1)
P_LO, P_HI = 2.0 ** -23, 1.0 - 2.0 ** -23


def view(x, code):
    out = np.rot90(x, k=code & 3, axes=(-2, -1))
    if code & 4:
        out = np.flip(out, axis=-1)
    if code & 8:
        out = np.flip(out, axis=-2)
    return np.ascontiguousarray(out)


def unview(v, code):
    out = v
    if code & 8:
        out = np.flip(out, axis=-2)
    if code & 4:
        out = np.flip(out, axis=-1)
    return np.ascontiguousarray(np.rot90(out, k=-(code & 3), axes=(-2, -1)))


def merge_logit(views, codes):
    assert len(views) == len(codes) >= 1
    with np.errstate(invalid="ignore"):
        acc = unview(np.asarray(views[0], dtype=np.float32), codes[0])
        for v, c in zip(views[1:], codes[1:]):
            acc = (acc + unview(np.asarray(v, dtype=np.float32), c)).astype(np.float32)
        return (acc / np.float32(len(codes))).astype(np.float32)


def finish_prob(mean, dtype):
    p = np.clip(mean, dtype(P_LO), dtype(P_HI))
    return (np.log(p) - np.log1p(-p)).astype(dtype)


def _merge_prob(views, codes, dtype):
    one = dtype(1)
    acc = None
    for v, c in zip(views, codes):
        u = unview(np.asarray(v, dtype=np.float32), c).astype(dtype)
        s = (one / (one + np.exp(-u))).astype(dtype)
        acc = s if acc is None else (acc + s).astype(dtype)
    return finish_prob((acc / dtype(len(codes))).astype(dtype), dtype)


def merge_prob64(views, codes):
    return _merge_prob(views, codes, np.float64)


def merge_prob32(views, codes):
    return _merge_prob(views, codes, np.float32)


def ramp(n, c, h, w):
    """fp32 [n, c, h, w] whose every element is a distinct integer (exact in fp32 below 2^24): a wrong pixel is a wrong value"""
    assert n * c * h * w < 2 ** 24
    return np.arange(n * c * h * w, dtype=np.float32).reshape(n, c, h, w)


def planted_logits(shape, lo, hi, seed, specials=True):
    """random fp32 logits in [lo, hi]; specials: +inf, -inf, +0, -0 and NaN planted at flat positions that do not depend on the
    seed - tensors of one shape drawn with different seeds meet there, so a sum over them keeps inf, -inf, +0, -0 and NaN - and
    two more positions whose value depends on the seed's parity: +inf / -inf (the sum is NaN) and +0 / -0 (the sum is +0)"""
    g = np.random.default_rng(seed)
    x = g.uniform(lo, hi, size=shape).astype(np.float32)
    if specials:
        f = x.reshape(-1)
        vals = [np.inf, -np.inf, 0.0, -0.0, np.nan, (np.inf, -np.inf)[seed & 1], (0.0, -0.0)[seed & 1]]
        for i, v in enumerate(vals):
            f[(i * 7919 + 5) % f.size] = np.float32(v)
    return x
