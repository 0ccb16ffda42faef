"""Inputs, the fp64 restatement and the launch regimes for the validation-step tests (tests/test_eval_cpu.py,
tests/test_eval_gpu.py, tests/golden/make_golden_eval.py). Nothing here touches a GPU.

A case is (N, K, hw, pattern): logits and targets [N, K, hw] fp32. nunet_seg_metrics runs gx = min(64, ceil(hw / 256)) blocks of
256 threads per (class, image) plane, one grid-stride loop per plane, then ONE workgroup of 256 threads in which thread j adds
the partials j, j + 256, ... of the N * gx partials of each class. Next to every shape stands (gx, most trips, fewest trips) of
the first launch, the regime it is the smallest shape to reach; FINAL_TRIPS names the second launch's.

The restatement (fp64, torch on the CPU):
    predicted foreground iff x >= thr (metrics.iou_logit_threshold: the reference's `sigmoid(x) > 0.5` in fp32; NaN is not),
    labelled foreground iff t > 0.5; tp / fp / fn / tn per class are the four conjunctions (the definition of the reference's
    numeric_score, metrics.py:31-44, which itself raises under current numpy);
    soft_i = sum sigmoid(x) t, soft_p = sum sigmoid(x), soft_t = sum t per class (the terms of dice_coef, metrics.py:21-29);
    batch IoU = (sum tp + 1e-5) / (sum (tp + fp + fn) + 1e-5), dice = (2 sum soft_i + 1e-5) / (sum soft_p + sum soft_t + 1e-5),
    acc = sum (tp + tn) / (N K hw) (the definition of the reference's Acc, metrics.py:47-53, which itself raises);
    Meter: AverageMeter (utils.py:17-33), update(value, n)."""
import functools

import numpy as np
import torch

import loss_cases as LC

# (N, K, hw): (gx, most trips, fewest trips)
SHAPES = {
    (2, 1, 1): (1, 1, 0),               # one element
    (3, 1, 255): (1, 1, 0),             # one block, not full
    (3, 1, 257): (2, 1, 0),             # a second block with one element
    (2, 1, 16384): (64, 1, 1),          # the block cap, one trip
    (2, 1, 16385): (64, 2, 1),          # a second trip for one thread
    (2, 1, 65537): (64, 5, 4),          # a fifth trip
    (3, 2, 300): (2, 1, 0),             # class planes
    (3, 4, 300): (2, 1, 0),
    (2, 8, 300): (2, 1, 0),
    (33, 8, 300): (2, 1, 0),            # more (image, class) pairs than the final workgroup has threads
    (5, 1, 16384): (64, 1, 1),          # 320 partials of a class: a second trip in the final workgroup
}
PATTERN_SHAPE = (3, 1, 16385)
PATTERNS = ["edges", "saturated", "all_background", "nan", "soft"]
CASES = [s + ("rand",) for s in SHAPES] + [PATTERN_SHAPE + (p,) for p in PATTERNS]
MAX_CLASSES = 8


def case_id(case):
    return "%dx%dx%d-%s" % case


def expected_regime(hw):
    gx = min(64, -(-hw // 256))
    return gx, -(-hw // (gx * 256)), hw // (gx * 256)


def final_trips(n, hw):
    """most trips of a thread of the one-workgroup launch: ceil(N * gx / 256)"""
    return -(-n * expected_regime(hw)[0] // 256)


@functools.lru_cache(maxsize=None)
def build(case):
    """-> (x, t) fp32 [N, K, hw], shared between tests: do not write to them"""
    n, k, hw, pattern = case
    seed = (n * 1000003 + k * 7919 + hw * 10007 + sum(map(ord, pattern)) * 7) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, k, hw, generator=g) * 2
    t = (torch.rand(n, k, hw, generator=g) < 0.4).float()
    if pattern == "edges":          # tests/loss_cases.py's values around the sigmoid threshold, against both labels
        e = torch.from_numpy(LC.iou_edges())
        x[0, 0, :e.numel()] = e
        x[1, 0, -e.numel():] = e
    elif pattern == "saturated":
        x[0], t[0] = -30, 0
        x[1], t[1] = 30, 1
        x[2], t[2] = -30, 1
    elif pattern == "all_background":   # union 0: IoU = 1 exactly
        x = -x.abs() - 1e-3
        t = torch.zeros_like(t)
    elif pattern == "nan":
        x[0, 0, ::7] = float("nan")
    elif pattern == "soft":
        t = torch.rand(n, k, hw, generator=g)
    else:
        assert pattern == "rand", pattern
    return x, t


def restate(x, t, thr):
    """dict of per-class lists over [N, K, ...] tensors: tp, fp, fn, tn (python ints), soft_i, soft_p, soft_t (python floats, fp64 sums)"""
    n, k = x.shape[:2]
    xd, td = x.double().reshape(n, k, -1), t.double().reshape(n, k, -1)
    a = x.reshape(n, k, -1) >= np.float32(thr)        # NaN compares false
    b = t.reshape(n, k, -1) > 0.5
    p = torch.sigmoid(xd)
    cnt = lambda m: [int(v) for v in m.sum((0, 2))]
    sm = lambda v: [float(q) for q in v.sum((0, 2))]
    return dict(tp=cnt(a & b), fp=cnt(a & ~b), fn=cnt(~a & b), tn=cnt(~a & ~b), soft_i=sm(p * td), soft_p=sm(p), soft_t=sm(td))


def batch_values(r, count):
    """(iou, dice, acc) of a restate() dict (or anything with the same keys) over `count` = N K hw decisions"""
    tp, fp, fn, tn = (sum(r[q]) for q in ("tp", "fp", "fn", "tn"))
    iou = (tp + 1e-5) / (tp + fp + fn + 1e-5)
    dice = (2.0 * sum(r["soft_i"]) + 1e-5) / (sum(r["soft_p"]) + sum(r["soft_t"]) + 1e-5)
    return iou, dice, (tp + tn) / float(count)


@functools.lru_cache(maxsize=None)
def reference(case, thr):
    """restate() of build(case), computed once: shared, do not write to it"""
    return restate(*build(case), thr)


class Meter:
    """AverageMeter of the reference's utils.py:17-33"""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / self.count


# the network cases of tests/golden/make_golden_eval.py: tag -> (num_classes, deep_supervision); 10 images of 32 x 32 in batches of 4
NET = {"k1": (1, False), "k4ds": (4, True)}
NET_SPLIT = (10, 32, 32, 3, 2000)      # images, H, W, input channels, seed
NET_BATCH = 4
