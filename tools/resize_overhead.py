"""Cost of the device-side Resize in the captured training step: ms per replay of the captured step, bf16, SGD, 96 x 96, batch 16,
rot90 / flip codes on, the one-hipGraph executor forced (the modes are compared on one executor).

    python tools/resize_overhead.py --parent DIR [--parent_modes u8] [--procs 3] [--steps 200] [--rounds 3] [--out FILE]     the comparison
    python tools/resize_overhead.py --modes u8,equal,ragged,ragged_hsv [--steps 200] [--rounds 3]        one process (also runs
                                                                                                         on a checkout without
                                                                                                         the resize: --modes u8)

Modes: u8 = TrainStep(input_u8=True) (resize=False on this commit, all there is on its parent); equal = resize=True fed sources
of the plan's own size; ragged = resize=True fed sources of 2 - 6 times the linear size (192 .. 576 pixels a side, drawn per
sample and per axis from a seeded generator); ragged_hsv = the same with every colour op HSV (13.7, -22.4, 9.2). The static
buffers are loaded once and the captured step is replayed: the timed window holds the step's launches and no host copy, so the
modes differ by their two head launches only. --parent DIR (a built checkout of the parent commit) alternates processes: the
parent's --parent_modes (u8 is all a parent without the resize has; a parent that has it takes all four), this commit's --modes,
--procs times. Every mode both trees ran is judged on its own: the difference of this commit's median and the parent's must lie
inside the parent's own round-to-round and process-to-process spread of that mode (<mode>_inside_parent_spread). Prints one line
per process, then a JSON summary (also written to --out).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW, BS = 96, 16
GRAPH = dict(segmented=False, schedule="lanes")
HSV = (1, 13.7, -22.4, 9.2)


def measure(modes, steps, rounds):
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    import nunet_amd
    from nunet_amd import dataset as D
    from nunet_amd.trainer import TrainStep

    raw, m8 = nunet_amd.synth.synth_blob_pairs_u8(BS, HW, HW, seed=5)
    aug = D.draw_augmentation(BS, torch.Generator().manual_seed(3), "cuda")

    def build(mode):
        st = nunet_amd.synth.closed_form_state(1, 3, False, True)
        m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="bf16")
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
        m = m.cuda().train()
        if mode == "u8":
            ts = TrainStep(m, (BS, 3, HW, HW), lr=1e-3, input_u8=True, **GRAPH)
            x, t = torch.from_numpy(raw).cuda(), torch.from_numpy(m8).cuda()
            ts.capture(x, t)
            ts.step_u8(x, t, aug)
            return ts, 0
        g = np.random.default_rng(11)
        if mode == "equal":
            imgs, msks = list(raw), list(m8)
        else:
            sizes = [(int(g.integers(2 * HW, 6 * HW + 1)), int(g.integers(2 * HW, 6 * HW + 1))) for _ in range(BS)]
            imgs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
            msks = [(g.integers(0, 2, (h, w, 1), dtype=np.uint8) * 255).astype(np.uint8) for h, w in sizes]
        cap = BS * (6 * HW) ** 2 * 3
        ts = TrainStep(m, (BS, 3, HW, HW), lr=1e-3, input_u8=True, color_aug=mode == "ragged_hsv", resize=True, source_capacity=cap, **GRAPH)
        ts.capture(D.pack_ragged(list(raw)), D.pack_ragged(list(m8)))
        col = D.color_codes([HSV[0]] * BS, [HSV[1:]] * BS).cuda() if mode == "ragged_hsv" else None
        ip, idesc = D.pack_ragged(imgs)
        mp, mdesc = D.pack_ragged(msks)
        ts.step_u8_ragged(ip, idesc, mp, mdesc, aug, col)
        return ts, int(ip.numel())

    def replays(ts):
        for _ in range(10):
            ts.step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            ts.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    runs = {mo: build(mo) for mo in modes}
    ms = {mo: [] for mo in modes}
    for _ in range(rounds):
        for mo in modes:
            ms[mo].append(replays(runs[mo][0]))
    return {mo: {"ms": ms[mo], "nodes": runs[mo][0].g_fb.info()["nodes"], "source_bytes": runs[mo][1]} for mo in modes}


def child(tree, modes, steps, rounds):
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "resize_overhead.py") if os.path.exists(os.path.join(tree, "tools", "resize_overhead.py"))
                        else os.path.abspath(__file__), "--modes", modes, "--steps", str(steps), "--rounds", str(rounds), "--tree", tree],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("child on %s failed (%d):\n%s\n%s" % (tree, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    global HERE
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="u8,equal,ragged,ragged_hsv")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: alternate processes of it and of this commit")
    ap.add_argument("--parent_modes", default="u8", help="the modes the parent checkout runs")
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is measured")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parent is None:
        if a.tree:
            HERE = os.path.abspath(a.tree)
        print(json.dumps(measure(a.modes.split(","), a.steps, a.rounds)))
        return
    acc = {}
    for p in range(a.procs):
        for prefix, tree, modes in (("parent_", os.path.abspath(a.parent), a.parent_modes), ("", HERE, a.modes)):
            res = child(tree, modes, a.steps, a.rounds)
            for mo, v in res.items():
                key = prefix + mo
                e = acc.setdefault(key, {"ms_by_process": [], "nodes": v["nodes"], "source_bytes": v["source_bytes"]})
                e["ms_by_process"].append(v["ms"])
                print("process %d %s: %s ms/step, %d graph nodes" % (p, key, " ".join("%.4f" % x for x in v["ms"]), v["nodes"]), flush=True)
    for e in acc.values():
        flat = [x for pr in e["ms_by_process"] for x in pr]
        e["min_ms"], e["median_ms"], e["spread_ms"] = min(flat), sorted(flat)[len(flat) // 2], max(flat) - min(flat)
        e["round_spread_ms"] = max(max(pr) - min(pr) for pr in e["ms_by_process"])
    base = acc["parent_u8"]
    out = {"method": "tools/resize_overhead.py --parent: ms per replay of the captured step (one hipGraph, static buffers loaded once), bf16, SGD, "
                     "%dx%d bs%d, rot90 / flip codes on; %d processes of each commit alternating, %d rounds of %d replays per mode and process"
                     % (HW, HW, BS, a.procs, a.rounds, a.steps),
           "modes": acc}
    for mo in acc:
        if not mo.startswith("parent_"):
            acc[mo]["minus_parent_u8_ms"] = acc[mo]["min_ms"] - base["min_ms"]
            acc[mo]["median_minus_parent_u8_ms"] = acc[mo]["median_ms"] - base["median_ms"]
            if "parent_" + mo in acc:
                acc[mo]["median_minus_parent_ms"] = acc[mo]["median_ms"] - acc["parent_" + mo]["median_ms"]
                out[mo + "_inside_parent_spread"] = abs(acc[mo]["median_minus_parent_ms"]) <= acc["parent_" + mo]["spread_ms"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
