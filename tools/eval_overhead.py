"""Cost of one validation pass in its three forms: the module loop (train.py validate() without EvalStep: model(xb), the
stand-alone loss and IoU entries, two host round trips per batch), EvalStep issued eagerly and EvalStep captured. bf16,
BCEDiceLoss, the split resident in HBM; device events around whole passes (each pass ends in its own read of the results, as
in train.py); the forms alternate inside every round so that box drift hits all alike.

    python tools/eval_overhead.py [--images 128] [--size 96] [--batch 16] [--classes 1] [--ds 0] [--warmup 3] [--rounds 7]

Prints one line per form (ms per pass of every round, median, spread = max - min), the three results side by side (loss and
iou must be equal to the bit) and a JSON summary with `captured_beats_module`: median(module) - median(captured) > the larger
of the two spreads - the rule by which train.py's --eval_step default was set.
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nunet_amd  # noqa: E402
from nunet_amd.metrics import iou_counts, iou_from_counts  # noqa: E402
from nunet_amd.trainer import EvalStep  # noqa: E402
from nunet_amd.utils import AverageMeter  # noqa: E402


def module_loop(model, crit, x, t, bs, ds):
    avg = {'loss': AverageMeter(), 'iou': AverageMeter()}
    model.eval()
    with torch.no_grad():
        for k in range(0, x.size(0), bs):
            xb, tb = x[k:k + bs].contiguous(), t[k:k + bs].contiguous()
            out = model(xb)
            if ds:
                loss = sum(crit(o, tb) for o in out) / len(out)
                last = out[-1]
            else:
                loss = crit(out, tb)
                last = out
            avg['loss'].update(loss.item(), xb.size(0))
            avg['iou'].update(iou_from_counts(iou_counts(last.contiguous(), tb)), xb.size(0))
    return OrderedDict([('loss', avg['loss'].avg), ('iou', avg['iou'].avg)])


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=1)
    ap.add_argument("--ds", type=int, default=0)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    ds = bool(a.ds)
    st = nunet_amd.synth.closed_form_state(a.classes, 3, ds, False)
    m = nunet_amd.archs.NestedUNet(a.classes, 3, ds, dtype=a.dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda()
    img, msk = nunet_amd.synth.synth_split(a.images, a.size, a.size, 3, a.classes, seed=2000)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    crit = nunet_amd.losses.BCEDiceLoss().cuda()
    shape = (a.batch, 3, a.size, a.size)
    eager, captured = EvalStep(m, shape, use_graph=False), EvalStep(m, shape)
    forms = OrderedDict([("module_loop", lambda: module_loop(m, crit, x, t, a.batch, ds)),
                         ("evalstep_eager", lambda: eager.evaluate(x, t)),
                         ("evalstep_captured", lambda: captured.evaluate(x, t))])
    for _ in range(a.warmup):
        for run in forms.values():
            run()
    ms = {k: [] for k in forms}
    res = {}
    for _ in range(a.rounds):
        for k, run in forms.items():
            dt, res[k] = timed(run)
            ms[k].append(dt)
    out = {"images": a.images, "size": a.size, "batch": a.batch, "classes": a.classes, "ds": ds, "dtype": a.dtype}
    for k in forms:
        med, spread = statistics.median(ms[k]), max(ms[k]) - min(ms[k])
        out[k] = {"ms": ms[k], "median_ms": med, "spread_ms": spread, "loss": res[k]["loss"], "iou": res[k]["iou"]}
        print("%-18s %s ms per pass; median %.3f, spread %.3f; loss %.9g iou %.9g"
              % (k, " ".join("%.3f" % v for v in ms[k]), med, spread, res[k]["loss"], res[k]["iou"]))
    same = all(res[k]["loss"] == res["module_loop"]["loss"] and res[k]["iou"] == res["module_loop"]["iou"] for k in forms)
    gain = out["module_loop"]["median_ms"] - out["evalstep_captured"]["median_ms"]
    out["bit_identical"] = same
    out["captured_beats_module"] = bool(gain > max(out["module_loop"]["spread_ms"], out["evalstep_captured"]["spread_ms"]))
    print(json.dumps(out))
    if not same:
        raise SystemExit("the three forms disagree on loss / iou")


if __name__ == "__main__":
    main()
