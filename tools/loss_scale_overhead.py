"""Cost of dynamic loss scaling in the captured training step: TrainStep ms/step with loss_scale=None against "dynamic" (fp16,
SGD, the executor each TrainStep chooses), rounds alternating between the two so that box drift hits both alike.

    python tools/loss_scale_overhead.py [--geom 96:16:1,512:8:4] [--steps 50] [--rounds 3]

--geom: comma-separated size:batch:classes. Prints one line per geometry and mode, then a JSON summary.
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


def build(hw, bs, ncls, scaling):
    st = nunet_amd.synth.closed_form_state(ncls, 3, False, True)
    m = nunet_amd.archs.NestedUNet(ncls, 3, False, dtype="fp16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    img, msk = nunet_amd.synth.synth_batch(bs, hw, hw, 3, ncls, seed=5)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    ts = TrainStep(m, (bs, 3, hw, hw), lr=1e-3, loss_scale="dynamic" if scaling else None)
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
    ap.add_argument("--geom", default="96:16:1,512:8:4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    out = {}
    for g in a.geom.split(","):
        hw, bs, ncls = (int(v) for v in g.split(":"))
        runs = {False: build(hw, bs, ncls, False), True: build(hw, bs, ncls, True)}
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for scaling in (False, True):
                ms[scaling].append(time_steps(*runs[scaling], a.steps))
        key = "%dx%d_bs%d_k%d" % (hw, hw, bs, ncls)
        out[key] = {"off_ms": ms[False], "on_ms": ms[True],
                    "overhead_pct": 100.0 * (min(ms[True]) / min(ms[False]) - 1.0),
                    "executor_off": str(runs[False][0].executor_choice), "executor_on": str(runs[True][0].executor_choice),
                    "scaler": runs[True][0].scaler_stats()}
        for scaling in (False, True):
            print("%s loss_scale=%s: %s ms/step (executor %s)" % (key, "dynamic" if scaling else "None",
                                                                 " ".join("%.3f" % v for v in ms[scaling]), runs[scaling][0].executor_choice))
        del runs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
