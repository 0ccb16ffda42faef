"""Cost of the weight EMA in the captured training step: TrainStep ms/step for each --ema mode (none = ema_decay=None, or a decay),
bf16, SGD, rounds alternating between the modes so that box drift hits all alike.

    python tools/ema_overhead.py [--geom 96:16:1,256:32:1] [--ema none,0.999] [--executor auto] [--steps 50] [--rounds 3] [--out FILE]

--geom: comma-separated size:batch:classes. --executor: auto (each TrainStep times its two forms and keeps the faster;
executor_choice holds both timings), graph (the one-hipGraph executor) or flags (flag-synchronised lanes, list-scheduled):
a forced form compares the modes on the same executor. With --ema none alone the script also runs on a checkout that has no
EMA (the off-path comparison against an earlier commit). Prints one line per geometry and mode, then a JSON summary (also
written to --out): per mode the rounds, their minimum and spread, and the overhead of every decay over none.
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


def build(hw, bs, ncls, ema, executor):
    st = nunet_amd.synth.closed_form_state(ncls, 3, False, True)
    m = nunet_amd.archs.NestedUNet(ncls, 3, False, dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    img, msk = nunet_amd.synth.synth_batch(bs, hw, hw, 3, ncls, seed=5)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    kw = dict(EXECUTORS[executor])
    if ema is not None:
        kw["ema_decay"] = ema
    ts = TrainStep(m, (bs, 3, hw, hw), lr=1e-3, **kw)
    ts.capture(x, t)
    return ts, x, t


def time_steps(ts, x, t, steps):
    for _ in range(5):
        ts.step(x, t)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ts.step(x, t)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", default="96:16:1,256:32:1")
    ap.add_argument("--ema", default="none,0.999")
    ap.add_argument("--executor", default="auto", choices=sorted(EXECUTORS))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    a = ap.parse_args()
    modes = [None if v == "none" else float(v) for v in a.ema.split(",")]
    out = {}
    for g in a.geom.split(","):
        hw, bs, ncls = (int(v) for v in g.split(":"))
        runs = {c: build(hw, bs, ncls, c, a.executor) for c in modes}
        ms = {c: [] for c in modes}
        for _ in range(a.rounds):
            for c in modes:
                ms[c].append(time_steps(*runs[c], a.steps))
        key = "%dx%d_bs%d_k%d" % (hw, hw, bs, ncls)
        out[key] = {"executor": a.executor}
        for c in modes:
            ts = runs[c][0]
            stats = ts.ema_stats() if c is not None else None
            out[key][str(c)] = {"ms": ms[c], "min_ms": min(ms[c]), "spread_ms": max(ms[c]) - min(ms[c]),
                                "executor_choice": str(ts.executor_choice), "form": "%s/%s" % (ts.segmented, ts.schedule), "ema": stats}
            print("%s ema_decay=%s: %s ms/step (executor %s/%s, choice %s)" % (key, c, " ".join("%.3f" % v for v in ms[c]),
                                                                              ts.segmented, ts.schedule, ts.executor_choice))
        if None in ms and len(modes) > 1:
            for c in modes:
                if c is not None:
                    out[key][str(c)]["overhead_pct"] = 100.0 * (min(ms[c]) / min(ms[None]) - 1.0)
        del runs
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
