"""Cost of the colour augmentation in the captured training step: TrainStep(input_u8=True).step_u8 ms/step with color_aug off,
on with every op NONE, and on with every op HSV (the worst case: the other two ops are one fp32 operation per channel), bf16,
SGD, rounds alternating between the modes so that box drift hits all alike.

    python tools/color_aug_overhead.py [--geom 96:16,256:32] [--modes off,none,hsv] [--executor auto] [--steps 50] [--rounds 3] [--out FILE]
    python tools/color_aug_overhead.py --parent DIR [--procs 3] [the options above]       against a built checkout of the parent commit

--geom: comma-separated size:batch. --executor: auto (each TrainStep times its two forms and keeps the faster; executor_choice
holds both timings), graph (the one-hipGraph executor) or flags (flag-synchronised lanes, list-scheduled): a forced form
compares the modes on the same executor. With --modes off alone the script also runs on a checkout that has no colour
augmentation (the off-path comparison against an earlier commit). The staging launch heads the step's critical chain, so the
number to read is the all-HSV step minus the off step. Prints one line per geometry and mode, then a JSON summary (also
written to --out): per mode the rounds, their minimum and spread, and the difference of every mode to off. Every round also
times the mode's staging launch alone (launch_us: --steps launches of nunet_plan_stage_u8 / _color back to back on the step's
own plan and buffers, device events around them). --parent DIR alternates processes of this file on the two checkouts
(tools/parent_compare.py) and judges, per geometry and mode, the step's ms and the launch's us against the parent's own spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

import parent_compare  # noqa: E402

sys.path.insert(0, parent_compare.tree())
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd.trainer import TrainStep  # noqa: E402

EXECUTORS = {"auto": {}, "graph": dict(segmented=False, schedule="lanes"), "flags": dict(segmented="flags", schedule="list")}
HSV_CODE = (1, 13.7, -22.4, 9.2)      # NUNET_COLOR_HSV with three non-zero shifts


def build(hw, bs, mode, executor):
    st = nunet_amd.synth.closed_form_state(1, 3, False, True)
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    raw, m8 = nunet_amd.synth.synth_blob_pairs_u8(bs, hw, hw, seed=5)
    x, t = torch.from_numpy(raw).cuda(), torch.from_numpy(m8).cuda()
    kw = dict(EXECUTORS[executor])
    color = None
    if mode != "off":
        kw["color_aug"] = True
        if mode == "hsv":
            color = nunet_amd.dataset.color_codes([HSV_CODE[0]] * bs, [HSV_CODE[1:]] * bs).cuda()
    ts = TrainStep(m, (bs, 3, hw, hw), lr=1e-3, input_u8=True, **kw)
    ts.capture(x, t)
    aug = nunet_amd.dataset.draw_augmentation(bs, torch.Generator().manual_seed(1), "cuda")
    args = (x, t, aug) if mode == "off" else (x, t, aug, color)
    return ts, args


def time_steps(ts, args, steps):
    for _ in range(5):
        ts.step_u8(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ts.step_u8(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def time_launches(ts, launches):
    """us per staging launch of the step (the entry TrainStep._fwd_loss calls, on its plan and static buffers), alone on the stream"""
    lib, pl, st = L.lib(), ts.pl, L.stream()
    head = (pl.handle, L.ptr(ts.x_u8), L.ptr(ts._mean), L.ptr(ts._std), L.ptr(ts.aug))
    tail = (1.0 / 255.0, L.ptr(pl.arena), L.nbytes(pl.arena), st)

    def launch():
        if ts.color is not None:
            L.check(lib.nunet_plan_stage_u8_color(*head, L.ptr(ts.color), *tail), "plan_stage_u8_color")
        else:
            L.check(lib.nunet_plan_stage_u8(*head, *tail), "plan_stage_u8")
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def compare(a, argv):
    runs = parent_compare.alternate(__file__, a.parent, argv, a.procs)
    out = {"method": "tools/color_aug_overhead.py --parent: %d processes of each commit alternating, %s" % (a.procs, " ".join(argv)), "geometries": {}}
    for key in runs["this"][0]:
        out["geometries"][key] = g = {}
        for c in a.modes.split(","):
            g[c] = {"step_ms": parent_compare.judge([r[key][c]["ms"] for r in runs["parent"]], [r[key][c]["ms"] for r in runs["this"]]),
                    "launch_us": parent_compare.judge([r[key][c]["launch_us"] for r in runs["parent"]], [r[key][c]["launch_us"] for r in runs["this"]])}
            print("%s %s: step %+.4f ms against a parent spread of %.4f, launch %+.3f us against %.3f" % (
                key, c, g[c]["step_ms"]["median_minus_parent"], g[c]["step_ms"]["parent_spread"], g[c]["launch_us"]["median_minus_parent"],
                g[c]["launch_us"]["parent_spread"]))
    out["all_inside_parent_spread"] = all(v["inside_parent_spread"] for g in out["geometries"].values() for m in g.values() for v in m.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", default="96:16,256:32")
    ap.add_argument("--modes", default="off,none,hsv")
    ap.add_argument("--executor", default="auto", choices=sorted(EXECUTORS))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: alternate processes of it and of this commit")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is measured")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if not set(modes) <= {"off", "none", "hsv"}:
        raise SystemExit("--modes takes off, none and hsv")
    out = {}
    for g in ([] if a.parent else a.geom.split(",")):
        hw, bs = (int(v) for v in g.split(":"))
        runs = {c: build(hw, bs, c, a.executor) for c in modes}
        ms, us = {c: [] for c in modes}, {c: [] for c in modes}
        for _ in range(a.rounds):
            for c in modes:
                ms[c].append(time_steps(*runs[c], a.steps))
                us[c].append(time_launches(runs[c][0], a.steps))
        key = "%dx%d_bs%d" % (hw, hw, bs)
        out[key] = {"executor": a.executor, "dtype": "bf16", "steps": a.steps}
        for c in modes:
            ts = runs[c][0]
            out[key][c] = {"ms": ms[c], "min_ms": min(ms[c]), "spread_ms": max(ms[c]) - min(ms[c]), "launch_us": us[c],
                           "executor_choice": str(ts.executor_choice), "form": "%s/%s" % (ts.segmented, ts.schedule)}
            print("%s color_aug=%s: %s ms/step (executor %s/%s, choice %s)" % (key, c, " ".join("%.3f" % v for v in ms[c]),
                                                                              ts.segmented, ts.schedule, ts.executor_choice))
        if "off" in ms:
            for c in modes:
                if c != "off":
                    out[key][c]["minus_off_ms"] = min(ms[c]) - min(ms["off"])
                    out[key][c]["minus_off_pct"] = 100.0 * (min(ms[c]) / min(ms["off"]) - 1.0)
        del runs
        torch.cuda.empty_cache()
    if a.parent:
        out = compare(a, ["--geom", a.geom, "--modes", a.modes, "--executor", a.executor, "--steps", str(a.steps), "--rounds", str(a.rounds)])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
