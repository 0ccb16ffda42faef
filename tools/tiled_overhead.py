"""Cost of full-resolution tiled inference (nunet_amd.tiled.TiledPredictor) next to the resized validation pass (EvalStep on
images squeezed to the tile's size), on the validation blobs drawn at --source_size. bf16, the sources resident on the host as
train.py / val.py hold them; device events around whole passes; the forms alternate inside every round.

    python tools/tiled_overhead.py [--images 32] [--source_size 192,576] [--tile 96] [--batch 16] [--overlap O] [--rounds 7]
                                   [--out profiles/tiled_overhead.json]
    python tools/tiled_overhead.py --parent DIR [--procs 3] [the options above]      against a built checkout of the parent commit

Reports, per image: ms of the full-resolution pass (predict(): host tables, copies, one replay per N tiles, one stitch), ms of
the resized pass (device Resize + EvalStep), tiles per image. The full-resolution time is then split on the device: the same
number of replays of the captured crop/stage + forward graph, of a captured forward alone (same plan, same staged image), and
the stitch launch on the same tile store - crop/stage = graph - forward. `outside_forward_share` is (crop/stage + stitch) /
(crop/stage + forward + stitch); `host_and_copies_share` is what predict() spends beyond those replays and the stitch. The
stitch's bytes/s come from its algorithmic traffic: every tile-logit element that lies inside its source read once (4 bytes),
every output element written once (4 + 1 bytes). --parent DIR alternates processes of this file on the two checkouts
(tools/parent_compare.py) and judges the full-resolution ms per image and the per-round outside-forward share against the
parent's own spread; the summary written is this commit's last process with the comparison under "against_parent".
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

import parent_compare  # noqa: E402

sys.path.insert(0, parent_compare.tree())
import nunet_amd  # noqa: E402
from nunet_amd import _lib as L  # noqa: E402
from nunet_amd import dataset as D  # noqa: E402
from nunet_amd import tiled as T  # noqa: E402
from nunet_amd.trainer import EvalStep, _NativeGraph  # noqa: E402


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def write(out, path):
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--source_size", default="192,576")
    ap.add_argument("--tile", type=int, default=96)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--overlap", type=int, default=None)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "tiled_overhead.json"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: alternate processes of it and of this commit")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is measured")
    a = ap.parse_args()
    if a.parent:
        argv = ["--images", str(a.images), "--source_size", a.source_size, "--tile", str(a.tile), "--batch", str(a.batch), "--dtype", a.dtype,
                "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--out", ""] + (["--overlap", str(a.overlap)] if a.overlap is not None else [])
        runs = parent_compare.alternate(__file__, a.parent, argv, a.procs)
        out = runs["this"][-1]
        out["against_parent"] = cmp = {"processes_each": a.procs}
        for k, pick in (("full_res_ms_per_image", lambda r: [v / a.images for v in r["ms"]["full_res"]]), ("outside_forward_share", lambda r: r["outside_forward_share_rounds"])):
            cmp[k] = parent_compare.judge([pick(r) for r in runs["parent"]], [pick(r) for r in runs["this"]])
            print("%s: %+.5f against a parent spread of %.5f" % (k, cmp[k]["median_minus_parent"], cmp[k]["parent_spread"]))
        cmp["all_inside_parent_spread"] = all(cmp[k]["inside_parent_spread"] for k in ("full_res_ms_per_image", "outside_forward_share"))
        write(out, a.out)
        return
    from train import ragged_sets
    samples = ragged_sets({"dataset": "synthetic_blobs", "source_size": a.source_size, "train_size": 0, "val_size": a.images})[1]
    st = nunet_amd.synth.closed_form_state(1, 3, False, False)
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype=a.dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().eval()
    ip, idesc = D.pack_ragged([s[0] for s in samples])
    mp, mdesc = D.pack_ragged([s[1] for s in samples])
    tp = T.TiledPredictor(m, (a.batch, 3, a.tile, a.tile), overlap=a.overlap, source_capacity=ip.numel())
    ev = EvalStep(m, (a.batch, 3, a.tile, a.tile))

    def full_res():
        return tp.predict(ip, idesc)

    def resized():
        x = D.resize_images(ip, idesc, (a.tile, a.tile))
        t = D.resize_masks(mp, mdesc, (a.tile, a.tile))
        return ev.evaluate(x, t)

    r = full_res()
    tiles = r["tiles"]
    nb = -(-sum(tiles) // a.batch)
    # the device split: replays of the predictor's own graph, of the forward alone, and the stitch on a store of the same size
    # (the forward alone runs on a second predictor's plan, packed and staged by one eager predict: one captured program per plan)
    fo = T.TiledPredictor(m, (a.batch, 3, a.tile, a.tile), overlap=a.overlap, source_capacity=ip.numel(), use_graph=False)
    fo.predict(ip, idesc)
    lib, pl = L.lib(), fo.pl

    def forward_only():
        L.check(lib.nunet_plan_forward(pl.handle, L.ptr(fo.flat_params), L.ptr(fo.bnbuf), L.ptr(fo.eng.nbt), None, L.ptr(pl.arena), L.nbytes(pl.arena),
                                       L.ptr(fo.logits), 2 | 4, L.stream()), "plan_forward")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        forward_only()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    fwd_graph = _NativeGraph(s, forward_only)
    torch.cuda.synchronize()
    tl, grids, out_elems = tp.tables(idesc)
    store = torch.randn((nb * a.batch, 1, a.tile, a.tile), dtype=torch.float32, device="cuda")
    d_desc, d_grids = idesc.cuda(), torch.from_numpy(grids).cuda()

    def replays(g):
        for _ in range(nb):
            g.replay()

    forms = {"full_res": full_res, "resized": resized, "graph_replays": lambda: replays(tp.graph), "forward_replays": lambda: replays(fwd_graph),
             "stitch": lambda: T.stitch_tiles(store, d_desc, d_grids, out_elems, tp.window)}
    for _ in range(a.warmup):
        for run in forms.values():
            run()
    ms = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, run in forms.items():
            ms[k].append(timed(run)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    shapes = [(int(h), int(w)) for h, w in idesc.numpy()[:, 2:4]]
    read = sum(4 * min(a.tile, h - y0) * min(a.tile, w - x0) for s_, y0, x0, _ in tl for h, w in [shapes[s_]])
    traffic = read + 5 * sum(h * w for h, w in shapes)
    stage = med["graph_replays"] - med["forward_replays"]
    dev_total = med["graph_replays"] + med["stitch"]
    out = {"images": a.images, "source_size": a.source_size, "tile": a.tile, "batch": a.batch, "overlap": tp.overlap, "dtype": a.dtype,
           "rounds": a.rounds, "tiles_per_image": sum(tiles) / float(a.images), "tiles": sum(tiles), "replays": nb,
           "source_pixels_per_image": sum(h * w for h, w in shapes) / float(a.images),
           "ms": ms, "median_ms": med, "spread_ms": spread,
           "full_res_ms_per_image": med["full_res"] / a.images, "resized_ms_per_image": med["resized"] / a.images,
           "forward_ms": med["forward_replays"], "crop_stage_ms": stage, "stitch_ms": med["stitch"],
           "outside_forward_share": (stage + med["stitch"]) / dev_total,
           "outside_forward_share_rounds": [(g - f + s_) / (g + s_) for g, f, s_ in zip(ms["graph_replays"], ms["forward_replays"], ms["stitch"])],
           "host_and_copies_share": (med["full_res"] - dev_total) / med["full_res"],
           "crop_plus_stitch_exceeds_forward": bool(stage + med["stitch"] > med["forward_replays"]),
           "stitch_algorithmic_bytes": traffic, "stitch_bytes_per_s": traffic / (med["stitch"] * 1e-3)}
    for k in forms:
        print("%-16s %s ms; median %.3f, spread %.3f" % (k, " ".join("%.3f" % v for v in ms[k]), med[k], spread[k]))
    write(out, a.out)


if __name__ == "__main__":
    main()
