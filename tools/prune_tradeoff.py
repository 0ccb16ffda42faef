"""What pruning a deep-supervision UNet++ to depth L buys and costs: for L = 1..4 (EvalStep(depth=L)), for the unpruned step
and for the unpruned step with per-head metrics (EvalStep(per_head=True)), one JSON line with

    arena_bytes      nunet_plan_arena_bytes of the step's plan
    conv_launches    3x3 convolutions of one forward, from the plan's census
    median_ms        ms per captured validation pass over the split (device events around whole passes, each ending in its own
    spread_ms        read of the results; median and max - min over the rounds after the warm-up passes)
    iou, dice        of the pass (depth L: head L's; the other rows: the last head's)

The rows alternate inside every round, so that box drift hits all alike (tools/eval_overhead.py measures the same way).

    python tools/prune_tradeoff.py [--name MODEL | closed-form weights] [--images 128] [--size 96] [--batch 16] [--classes 1]
                                   [--dtype bf16] [--warmup 3] [--rounds 9]

--name reads models/<name>/config.yml and model.pth (a checkpoint trained with --deep_supervision true) and its validation
split; without it the weights are synth.closed_form_state and the split is synthetic.
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
from nunet_amd.trainer import EvalStep  # noqa: E402


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
    ap.add_argument("--name", default=None, help="model directory under models/ (default: closed-form weights)")
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=1)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if a.name is not None:
        import yaml
        with open("models/%s/config.yml" % a.name) as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)
        if cfg["arch"] != "NestedUNet" or not cfg["deep_supervision"]:
            raise SystemExit("error: models/%s was not trained as a NestedUNet with --deep_supervision true" % a.name)
        classes, cin, h, w, images = cfg["num_classes"], cfg["input_channels"], cfg["input_h"], cfg["input_w"], cfg["val_size"]
        m = nunet_amd.archs.NestedUNet(classes, cin, True, dtype=cfg.get("dtype", a.dtype))
        m.load_state_dict(torch.load("models/%s/model.pth" % a.name, map_location="cpu"))
    else:
        classes, cin, h, w, images = a.classes, 3, a.size, a.size, a.images
        st = nunet_amd.synth.closed_form_state(classes, cin, True, False)
        m = nunet_amd.archs.NestedUNet(classes, cin, True, dtype=a.dtype)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().eval()
    img, msk = nunet_amd.synth.synth_split(images, h, w, cin, classes, seed=2000)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    shape = (min(a.batch, images), cin, h, w)
    steps = OrderedDict(("depth%d" % d, EvalStep(m, shape, depth=d)) for d in (1, 2, 3, 4))
    steps["unpruned"] = EvalStep(m, shape)
    steps["unpruned_per_head"] = EvalStep(m, shape, per_head=True)
    for _ in range(a.warmup):
        for ev in steps.values():
            ev.evaluate(x, t)
    ms, res = {k: [] for k in steps}, {}
    for _ in range(a.rounds):
        for k, ev in steps.items():
            dt, res[k] = timed(lambda ev=ev: ev.evaluate(x, t))
            ms[k].append(dt)
    for k, ev in steps.items():
        pl = ev.main.pl
        row = OrderedDict([("row", k), ("depth", ev.depth), ("images", images), ("size", [h, w]), ("batch", shape[0]), ("dtype", a.dtype),
                           ("arena_bytes", int(pl.arena_bytes)), ("conv_launches", len(pl.census(False))),
                           ("median_ms", statistics.median(ms[k])), ("spread_ms", max(ms[k]) - min(ms[k])), ("ms", ms[k]),
                           ("iou", res[k]["iou"]), ("dice", res[k]["dice"])])
        if "heads" in res[k]:
            row["head_iou"] = [hd["iou"] for hd in res[k]["heads"]]
            row["head_dice"] = [hd["dice"] for hd in res[k]["heads"]]
        print(json.dumps(row))


if __name__ == "__main__":
    main()
