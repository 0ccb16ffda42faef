"""Drop-in `metrics` (reference metrics.py): global batch IoU (:6-18), dice_coef (:21-29), and what numeric_score (:31-44)
and Acc (:47-53) define - per-class TP / FP / FN / TN and the pixel accuracy - computed on the device."""
import ctypes as C

import torch

from . import _lib as L


_IOU_THR = None


def iou_logit_threshold():
    """The smallest fp32 logit x with `torch.sigmoid(x) > 0.5` as the REFERENCE evaluates it (metrics.py:10-12: fp32 sigmoid
    on the host, then `> 0.5`). It is not 0: in fp32 sigmoid(x) rounds to exactly 0.5 for 0 < x <~ 6e-8, and those pixels
    are background in the reference's integer counts. Found once by bisection over fp32 bit patterns with the host's
    torch.sigmoid (padded to a full vector: torch's scalar tail can differ from its vectorised path by an ulp)."""
    global _IOU_THR
    if _IOU_THR is None:
        import numpy as np

        def fg(bits):
            xp = np.zeros(256, np.float32)
            xp[0] = np.array([bits], np.uint32).view(np.float32)[0]
            return bool(torch.sigmoid(torch.from_numpy(xp)).numpy()[0] > np.float32(0.5))
        lo, hi = 0, int(np.array([1.0], np.float32).view(np.uint32)[0])     # sigmoid(+0) = 0.5: not foreground; sigmoid(1) is
        assert not fg(lo) and fg(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fg(mid):
                hi = mid
            else:
                lo = mid
        _IOU_THR = float(np.array([hi], np.uint32).view(np.float32)[0])
    return _IOU_THR


def iou_counts(output, target, counts=None):
    """Device-side (intersection, union) counts as a uint64[2] tensor; no host sync.
    `counts` may be passed to accumulate over several batches."""
    L.require_gpu_tensor(output, torch.float32, "output")
    L.require_gpu_tensor(target, torch.float32, "target")
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device=output.device)
    L.check(L.lib().nunet_iou_counts(L.ptr(output), L.ptr(target), output.numel(), iou_logit_threshold(), L.ptr(counts), L.stream()),
            "nunet_iou_counts")
    return counts


def iou_from_counts(counts):
    smooth = 1e-5
    i, u = (int(v) for v in counts.tolist())
    return (i + smooth) / (u + smooth)


def iou_score(output, target):
    """Same value and return type (python float) as reference metrics.py:6-18;
    like the reference it synchronises with the device."""
    return iou_from_counts(iou_counts(output.detach().contiguous(), target.contiguous()))


def _nk_hw(output, target):
    L.require_gpu_tensor(output, torch.float32, "output")
    L.require_gpu_tensor(target, torch.float32, "target")
    if output.shape != target.shape or output.dim() < 2:
        raise L.NunetError("segmentation metrics: output %s vs target %s ([N, K, ...] expected)" % (tuple(output.shape), tuple(target.shape)))
    n, k = output.size(0), output.size(1)
    return n, k, output.numel() // (n * k)


def seg_sums(output, target, sums=None):
    """nunet_seg_sums of [N, K, ...] fp32 logits against targets of the same shape, as a device byte tensor of one L.SegSums
    (read it with L.read_struct(sums, L.SegSums)); no host sync. `sums` may be passed to accumulate over several batches."""
    n, k, hw = _nk_hw(output, target)
    lib = L.lib()
    acc = sums is not None
    if sums is None:
        sums = torch.zeros(C.sizeof(L.SegSums), dtype=torch.uint8, device=output.device)
    ws = torch.empty((lib.nunet_seg_metrics_ws_bytes(n, k, hw) + 7) // 8, dtype=torch.float64, device=output.device)
    L.check(lib.nunet_seg_metrics(L.ptr(output), L.ptr(target), n, k, hw, iou_logit_threshold(), L.ptr(ws), L.nbytes(ws), L.ptr(sums),
                                  1 if acc else 0, L.stream()), "nunet_seg_metrics")
    return sums


def seg_counts(output, target, sums=None):
    """Per-class (tp, fp, fn, tn) of [N, K, ...] logits as four int64[K] views of a device buffer; no host sync. Pass the
    returned tuple's `sums` buffer (seg_counts(...).sums) back in to accumulate over batches.
    A pixel is predicted foreground iff sigmoid(x) > 0.5 as the reference's iou_score evaluates it (iou_logit_threshold) and
    labelled foreground iff t > 0.5. This restates the DEFINITION of the reference's numeric_score (metrics.py:31-44: FP =
    sum(pred == 1 & gt == 0), FN, TP, TN); the function itself cannot serve as an oracle: it calls np.float, which current
    numpy no longer has, and raises."""
    sums = seg_sums(output, target, sums)
    k = output.size(1)
    v = sums.view(torch.int64)
    return SegCounts(v[0:k], v[8:8 + k], v[16:16 + k], v[24:24 + k], sums)


class SegCounts(tuple):
    """(tp, fp, fn, tn) with the underlying device buffer as .sums"""

    def __new__(cls, tp, fp, fn, tn, sums):
        self = super().__new__(cls, (tp, fp, fn, tn))
        self.sums = sums
        return self


def dice_coef(output, target):
    """Same value and return type (python float) as reference metrics.py:21-29: (2 sum(sigmoid(o) t) + 1e-5) /
    (sum(sigmoid(o)) + sum(t) + 1e-5) over the whole tensor; the three sums are taken on the device (fp32 sigmoid, added in
    double), the quotient in double on the host. Like the reference it synchronises with the device."""
    s = L.read_struct(seg_sums(output.detach().contiguous(), target.contiguous()), L.SegSums)
    smooth = 1e-5
    return (2.0 * sum(s.soft_i) + smooth) / (sum(s.soft_p) + sum(s.soft_t) + smooth)


def pixel_accuracy(output, target):
    """Fraction of (pixel, class) decisions that are right, (TP + TN) / count. This restates the DEFINITION of the reference's
    Acc (metrics.py:47-53: 1 - sum(pred != gt) / nelement); the function itself cannot serve as an oracle: it calls
    .nelement() on a numpy array and raises. One host sync."""
    s = L.read_struct(seg_sums(output.detach().contiguous(), target.contiguous()), L.SegSums)
    return (sum(s.tp) + sum(s.tn)) / float(sum(s.tp) + sum(s.tn) + sum(s.fp) + sum(s.fn))


def scores_from_counts(tp, fp, fn, tn):
    """Per-class and micro-averaged scores of integer counts (sequences of equal length, one entry per class): an OrderedDict
    name -> (list per class, micro) for iou = tp / (tp + fp + fn), dice = 2 tp / (2 tp + fp + fn), accuracy = (tp + tn) / all,
    sensitivity = tp / (tp + fn), specificity = tn / (tn + fp), precision = tp / (tp + fp). An empty denominator gives 1.0 for
    iou / dice (nothing to find, nothing found: the reference's smooth terms give the same) and nan elsewhere."""
    from collections import OrderedDict
    tp, fp, fn, tn = ([int(v) for v in q] for q in (tp, fp, fn, tn))

    def ratio(a, b, empty):
        return a / b if b else empty

    def row(a, b, c, d):
        nan = float("nan")
        return (ratio(a, a + b + c, 1.0), ratio(2 * a, 2 * a + b + c, 1.0), ratio(a + d, a + b + c + d, nan), ratio(a, a + c, nan),
                ratio(d, d + b, nan), ratio(a, a + b, nan))
    per = [row(*q) for q in zip(tp, fp, fn, tn)]
    micro = row(sum(tp), sum(fp), sum(fn), sum(tn))
    names = ("iou", "dice", "accuracy", "sensitivity", "specificity", "precision")
    return OrderedDict((nm, ([p[i] for p in per], micro[i])) for i, nm in enumerate(names))


_U8_THRESHOLDS = {}


def sigmoid_u8_thresholds(device):
    """thr[k-1], k = 1..255: the smallest fp32 logit x with `(torch.sigmoid(x) * 255).astype('uint8') >= k`, found by
    bisection over fp32 bit patterns with the host's torch.sigmoid - the function the reference's export applies
    (val.py:100-105). The device kernel counts thresholds <= x, so its bytes equal the reference's exactly."""
    import numpy as np
    import torch
    key = str(device)
    if key not in _U8_THRESHOLDS:
        def byte(x):        # the reference expression, float32 throughout; padded to 256 so that every element takes
            xp = np.zeros(256, np.float32); xp[:x.size] = x      # torch's vectorised path (its scalar tail can differ by an ulp)
            return (torch.sigmoid(torch.from_numpy(xp)).numpy() * np.float32(255)).astype("uint8").astype(np.int64)[:x.size]

        def key_of(x):      # order-preserving int64 key of a float32
            b = x.view(np.int32).astype(np.int64)
            return np.where(b >= 0, b, -(b & 0x7fffffff) - 1)

        def from_key(k):
            b = np.where(k >= 0, k, (-(k + 1)) | 0x80000000).astype(np.uint32)
            return b.view(np.float32)
        ks = np.arange(1, 256, dtype=np.int64)
        lo = np.full(255, key_of(np.array([-200.0], np.float32))[0], np.int64)   # byte(lo) = 0 < k
        hi = np.full(255, key_of(np.array([200.0], np.float32))[0], np.int64)    # byte(hi) = 255 >= k
        assert byte(from_key(lo))[0] == 0 and byte(from_key(hi))[0] == 255
        while np.any(hi - lo > 1):
            mid = (lo + hi) // 2
            ge = byte(from_key(mid)) >= ks
            hi = np.where(ge, mid, hi)
            lo = np.where(ge, lo, mid)
        _U8_THRESHOLDS[key] = torch.from_numpy(from_key(hi).copy()).to(device)
    return _U8_THRESHOLDS[key]


def sigmoid_masks_u8(output):
    """uint8 masks of the evaluation driver, `(sigmoid(output) * 255).astype('uint8')` (reference val.py:100-105),
    computed on the device, byte-exact against the host expression: [N, K, H, W] fp32 logits -> [N, K, H, W] uint8."""
    import torch
    from . import _lib as L
    out = output.detach().contiguous()
    if out.dtype != torch.float32 or not out.is_cuda:
        raise L.NunetError("sigmoid_masks_u8: CUDA fp32 logits expected")
    m = torch.empty(out.shape, dtype=torch.uint8, device=out.device)
    thr = sigmoid_u8_thresholds(out.device)
    L.check(L.lib().nunet_sigmoid_u8(L.ptr(out), L.ptr(thr), L.ptr(m), out.numel(), L.stream()), "sigmoid_u8")
    return m
