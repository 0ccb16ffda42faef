"""Cost of the colour augmentation in the captured training step: TrainStep(input_u8=True).step_u8 ms/step with color_aug off,
on with every op NONE, and on with every op HSV (the worst case: the other two ops are one fp32 operation per channel), bf16,
SGD, rounds alternating between the modes so that box drift hits all alike.

    python tools/color_aug_overhead.py [--geom 96:16,256:32] [--modes off,none,hsv] [--executor auto] [--steps 50] [--rounds 3] [--out FILE]

--geom: comma-separated size:batch. --executor: auto (each TrainStep times its two forms and keeps the faster; executor_choice
holds both timings), graph (the one-hipGraph executor) or flags (flag-synchronised lanes, list-scheduled): a forced form
compares the modes on the same executor. With --modes off alone the script also runs on a checkout that has no colour
augmentation (the off-path comparison against an earlier commit). The staging launch heads the step's critical chain, so the
number to read is the all-HSV step minus the off step. Prints one line per geometry and mode, then a JSON summary (also
written to --out): per mode the rounds, their minimum and spread, and the difference of every mode to off.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nunet_amd  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", default="96:16,256:32")
    ap.add_argument("--modes", default="off,none,hsv")
    ap.add_argument("--executor", default="auto", choices=sorted(EXECUTORS))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if not set(modes) <= {"off", "none", "hsv"}:
        raise SystemExit("--modes takes off, none and hsv")
    out = {}
    for g in a.geom.split(","):
        hw, bs = (int(v) for v in g.split(":"))
        runs = {c: build(hw, bs, c, a.executor) for c in modes}
        ms = {c: [] for c in modes}
        for _ in range(a.rounds):
            for c in modes:
                ms[c].append(time_steps(*runs[c], a.steps))
        key = "%dx%d_bs%d" % (hw, hw, bs)
        out[key] = {"executor": a.executor, "dtype": "bf16", "steps": a.steps}
        for c in modes:
            ts = runs[c][0]
            out[key][c] = {"ms": ms[c], "min_ms": min(ms[c]), "spread_ms": max(ms[c]) - min(ms[c]),
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
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
