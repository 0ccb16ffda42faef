"""Cost of test-time augmentation in the captured validation pass: EvalStep.evaluate over a split resident in HBM with tta None,
"flips" (4 views) and "d4" (8 views) - bf16, BCEDiceLoss, 96 x 96, batch 16, the bench shape; device events around whole
passes (each ends in its own read of the results), the forms alternating inside every round so that box drift hits all alike.
Beside it, per form, the time of the dihedral and merge launches one batch adds, issued back to back on buffers of the step's
shapes, and their share of a pass; and nunet_tta_merge alone on [32, 4, 256, 256] for codes 0, 1, 4, 5 next to a torch device
copy of the same bytes (the floor of any kernel that reads a view and writes an accumulator once).

    python tools/tta_overhead.py [--images 128] [--size 96] [--batch 16] [--warmup 3] [--rounds 7] [--launches 200]
                                 [--out profiles/tta_overhead.json]

Prints one line per form and per code and a JSON summary. `pass_ratio` is median ms over the plain pass's (expected: about the
number of views); `odd_over_code0` the slowest odd-rotation merge over code 0's (expected: about 1 - the LDS staging keeps the
transposed side coalesced; above 1.5 it is not doing its job)."""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import numpy as np
import torch

import parent_compare  # noqa: E402

sys.path.insert(0, parent_compare.tree())
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.trainer import EvalStep, TTA_SETS  # noqa: E402


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def tta_launches(ev, reps):
    """run: `reps` times the dihedral and merge launches one batch of `ev` adds, on buffers of its shapes"""
    b, lib = ev.main, L.lib()

    def run():
        st = L.stream()
        for _ in range(reps):
            for i, code in enumerate(ev.tta):
                if code:
                    L.check(lib.nunet_dihedral_nchw(L.ptr(b.x), b.n, ev.cin, ev.h, ev.w, code, L.ptr(b.x_view), st), "dihedral_nchw")
                L.check(lib.nunet_tta_merge(L.ptr(b.view_logits), b.heads * b.n, ev.ncls, ev.h, ev.w, code, ev.tta_mode, i, len(ev.tta), L.ptr(b.logits), st),
                        "tta_merge")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200, help="stand-alone launches between a pair of events")
    ap.add_argument("--merge_shape", default="32,4,256,256")
    ap.add_argument("--out", default=os.path.join("profiles", "tta_overhead.json"))
    a = ap.parse_args()
    st = nunet_amd.synth.closed_form_state(1, 3, False, False)
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype=a.dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda()
    img, msk = nunet_amd.synth.synth_split(a.images, a.size, a.size, 3, 1, seed=2000)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    shape = (a.batch, 3, a.size, a.size)
    steps = OrderedDict((str(k), EvalStep(m, shape, tta=k)) for k in (None, "flips", "d4"))
    forms = OrderedDict((k, (lambda ev=ev: ev.evaluate(x, t))) for k, ev in steps.items())
    alone = OrderedDict((k, tta_launches(ev, a.launches)) for k, ev in steps.items() if ev.tta)
    # nunet_tta_merge alone, as a middle view (acc = acc + v: one read of the view, one read and one write of the accumulator)
    n, k, h, w = (int(v) for v in a.merge_shape.split(","))
    view = torch.randn(n, k, h, w, device="cuda")
    acc = torch.zeros(n, k, h, w, device="cuda")
    lib = L.lib()

    def merge_run(code):
        def run():
            s = L.stream()
            for _ in range(a.launches):
                L.check(lib.nunet_tta_merge(L.ptr(view), n, k, h, w, code, L.TTA_LOGIT, 1, 3, L.ptr(acc), s), "tta_merge")
        return run

    def copy_run():
        for _ in range(a.launches):
            acc.copy_(view)

    merges = OrderedDict([("code%d" % c, merge_run(c)) for c in (0, 1, 4, 5)] + [("torch_copy", copy_run)])
    for _ in range(a.warmup):
        for run in list(forms.values()) + list(alone.values()) + list(merges.values()):
            run()
    ms = {k_: [] for k_ in forms}
    us = {k_: [] for k_ in alone}
    mus = {k_: [] for k_ in merges}
    res = {}
    for _ in range(a.rounds):
        for k_, run in forms.items():
            dt, res[k_] = timed(run)
            ms[k_].append(dt)
        for k_, run in alone.items():
            us[k_].append(timed(run)[0] * 1e3 / a.launches)
        for k_, run in merges.items():
            mus[k_].append(timed(run)[0] / a.launches)
    out = {"images": a.images, "size": a.size, "batch": a.batch, "dtype": a.dtype, "launches": a.launches, "merge_shape": [n, k, h, w]}
    batches = -(-a.images // a.batch)
    base = statistics.median(ms["None"])
    for k_ in forms:
        med, spread = statistics.median(ms[k_]), max(ms[k_]) - min(ms[k_])
        views = len(TTA_SETS[k_]) if k_ in TTA_SETS else 1
        out[k_] = {"views": views, "ms": ms[k_], "median_ms": med, "spread_ms": spread, "pass_ratio": med / base, "loss": res[k_]["loss"],
                   "iou": res[k_]["iou"], "dice": res[k_]["dice"]}
        if k_ in us:
            per_batch = statistics.median(us[k_])
            out[k_]["tta_launches_us_per_batch"] = per_batch
            out[k_]["tta_launch_share"] = per_batch * 1e-3 * batches / med
        print("%-6s %s ms per pass; median %.3f, spread %.3f, x%.2f the plain pass; iou %.6f%s"
              % (k_, " ".join("%.3f" % v for v in ms[k_]), med, spread, med / base, res[k_]["iou"],
                 "; dihedral + merge launches %.1f us per batch, %.1f%% of the pass" % (out[k_]["tta_launches_us_per_batch"], 100 * out[k_]["tta_launch_share"])
                 if k_ in us else ""))
    out["merge_ms"] = {k_: {"ms": v, "median_ms": statistics.median(v), "spread_ms": max(v) - min(v)} for k_, v in mus.items()}
    for k_, v in mus.items():
        print("%-10s %s ms per launch; median %.4f" % (k_, " ".join("%.4f" % q for q in v), statistics.median(v)))
    med = {k_: out["merge_ms"][k_]["median_ms"] for k_ in mus}
    out["odd_over_code0"] = max(med["code1"], med["code5"]) / med["code0"]
    out["code0_over_torch_copy"] = med["code0"] / med["torch_copy"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
