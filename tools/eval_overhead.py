"""Cost of one validation pass in its three forms: the module loop (train.py validate() without EvalStep: model(xb), the
stand-alone loss and IoU entries, two host round trips per batch), EvalStep issued eagerly and EvalStep captured. bf16,
BCEDiceLoss, the split resident in HBM; device events around whole passes (each pass ends in its own read of the results, as
in train.py); the forms alternate inside every round so that box drift hits all alike.

    python tools/eval_overhead.py [--images 128] [--size 96] [--batch 16] [--classes 1] [--ds 0] [--warmup 3] [--rounds 7]
    python tools/eval_overhead.py --parent DIR [--procs 3] [--out profiles/eval_overhead.json] [the options above]

Prints one line per form (ms per pass of every round, median, spread = max - min), the three results side by side (loss and
iou must be equal to the bit) and a JSON summary with `captured_beats_module`: median(module) - median(captured) > the larger
of the two spreads - the rule by which train.py's --eval_step default was set. Every round also times the two
stand-alone launches the validation step is built from, nunet_seg_metrics and nunet_bce_dice_fwd on one batch of logits
(--launches calls between a pair of events, us per call).

--parent DIR (a built checkout of the parent commit) alternates processes of this file on the two checkouts
(tools/parent_compare.py) and judges the captured pass and the two launches against the parent's own spread; the summary
written is this commit's last process with the comparison under "against_parent".
"""
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


def standalone_launches(batch, classes, size, launches):
    """{name: run} of `launches` calls of nunet_seg_metrics / nunet_bce_dice_fwd on [batch, classes, size, size] logits"""
    lib, n, hw = L.lib(), batch, size * size
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(n, classes, hw, generator=g) * 2).cuda()
    t = (torch.rand(n, classes, hw, generator=g) < 0.4).float().cuda()
    thr = nunet_amd.metrics.iou_logit_threshold()
    seg_ws = torch.empty(lib.nunet_seg_metrics_ws_bytes(n, classes, hw) // 8, dtype=torch.float64, device="cuda")
    sums = torch.zeros(1024, dtype=torch.float64, device="cuda")
    bd_ws = torch.empty((lib.nunet_bce_dice_ws_bytes(n) + 3) // 4, device="cuda")
    loss = torch.zeros(1, device="cuda")

    def seg():
        for _ in range(launches):
            L.check(lib.nunet_seg_metrics(L.ptr(x), L.ptr(t), n, classes, hw, thr, L.ptr(seg_ws), L.nbytes(seg_ws), L.ptr(sums), 0, L.stream()), "nunet_seg_metrics")

    def bce_dice():
        for _ in range(launches):
            L.check(lib.nunet_bce_dice_fwd(L.ptr(x), L.ptr(t), n, classes * hw, L.ptr(bd_ws), L.nbytes(bd_ws), L.ptr(loss), L.stream()), "nunet_bce_dice_fwd")

    return OrderedDict([("seg_metrics", seg), ("bce_dice_fwd", bce_dice)])


def write(out, path):
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


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
    ap.add_argument("--launches", type=int, default=300, help="stand-alone launches between a pair of events")
    ap.add_argument("--out", default="", help="write the JSON summary here too")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: alternate processes of it and of this commit")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is measured")
    a = ap.parse_args()
    if a.parent:
        argv = ["--images", str(a.images), "--size", str(a.size), "--batch", str(a.batch), "--classes", str(a.classes), "--ds", str(a.ds), "--dtype", a.dtype,
                "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--launches", str(a.launches)]
        runs = parent_compare.alternate(__file__, a.parent, argv, a.procs)
        out = runs["this"][-1]
        out["against_parent"] = cmp = {"processes_each": a.procs}
        picks = (("evalstep_captured_ms", lambda r: r["evalstep_captured"]["ms"]), ("seg_metrics_us", lambda r: r["launch_us"]["seg_metrics"]),
                 ("bce_dice_fwd_us", lambda r: r["launch_us"]["bce_dice_fwd"]))
        for k, pick in picks:
            cmp[k] = parent_compare.judge([pick(r) for r in runs["parent"]], [pick(r) for r in runs["this"]])
            print("%s: %+.5f against a parent spread of %.5f" % (k, cmp[k]["median_minus_parent"], cmp[k]["parent_spread"]))
        cmp["all_inside_parent_spread"] = all(cmp[k]["inside_parent_spread"] for k, _ in picks)
        write(out, a.out or os.path.join("profiles", "eval_overhead.json"))
        return
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
    alone = standalone_launches(a.batch, a.classes, a.size, a.launches)
    for _ in range(a.warmup):
        for run in list(forms.values()) + list(alone.values()):
            run()
    ms = {k: [] for k in forms}
    us = {k: [] for k in alone}
    res = {}
    for _ in range(a.rounds):
        for k, run in forms.items():
            dt, res[k] = timed(run)
            ms[k].append(dt)
        for k, run in alone.items():
            us[k].append(timed(run)[0] * 1e3 / a.launches)
    out = {"images": a.images, "size": a.size, "batch": a.batch, "classes": a.classes, "ds": ds, "dtype": a.dtype}
    for k in forms:
        med, spread = statistics.median(ms[k]), max(ms[k]) - min(ms[k])
        out[k] = {"ms": ms[k], "median_ms": med, "spread_ms": spread, "loss": res[k]["loss"], "iou": res[k]["iou"]}
        print("%-18s %s ms per pass; median %.3f, spread %.3f; loss %.9g iou %.9g"
              % (k, " ".join("%.3f" % v for v in ms[k]), med, spread, res[k]["loss"], res[k]["iou"]))
    out["launches"], out["launch_us"] = a.launches, us
    for k in alone:
        print("%-18s %s us per call; median %.3f, spread %.3f" % (k, " ".join("%.3f" % v for v in us[k]), statistics.median(us[k]), max(us[k]) - min(us[k])))
    same = all(res[k]["loss"] == res["module_loop"]["loss"] and res[k]["iou"] == res["module_loop"]["iou"] for k in forms)
    gain = out["module_loop"]["median_ms"] - out["evalstep_captured"]["median_ms"]
    out["bit_identical"] = same
    out["captured_beats_module"] = bool(gain > max(out["module_loop"]["spread_ms"], out["evalstep_captured"]["spread_ms"]))
    write(out, a.out)
    if not same:
        raise SystemExit("the three forms disagree on loss / iou")


if __name__ == "__main__":
    main()
