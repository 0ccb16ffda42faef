"""Bit identity of the loss, metric, validation-step and mask-export entries between two checkouts: SHA-256 of every output
buffer and of the WHOLE workspace after each call (the slab layout is part of the contract), over the case tables of
tests/loss_cases.py, tests/bce_logits_cases.py, tests/lovasz_cases.py and tests/eval_cases.py. A one-off comparison tool for a
change that must not move a bit (the kernels are deterministic run to run: plain stores, fixed-order trees, integer atomics).

    python tools/loss_parity_digest.py --parent DIR [--out profiles/loss_parity_digest.json]    DIR: a built checkout of the parent commit
    python tools/loss_parity_digest.py [--tree DIR]                                             the digests of one checkout, as JSON

--parent runs one process per checkout (tools/parent_compare.py picks the package by --tree; the case tables are this
checkout's for both), compares digest by digest and exits non-zero if any differs. Workspaces and outputs start from a fixed
byte pattern, so bytes a call leaves alone compare equal too.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import parent_compare  # noqa: E402

sys.path.insert(0, os.path.join(parent_compare.HERE, "tests"))
sys.path.insert(0, parent_compare.tree())


def digests():
    import torch
    import nunet_amd  # noqa: F401
    from nunet_amd import _lib as L
    from nunet_amd.metrics import iou_logit_threshold, sigmoid_u8_thresholds
    import bce_logits_cases as BC
    import eval_cases as EC
    import loss_cases as LC
    import lovasz_cases as VC

    dev, lib, thr = "cuda:0", L.lib(), iou_logit_threshold()
    out = {}

    def buf(nbytes):
        return torch.full(((nbytes + 7) // 8 * 8,), 0xC3, dtype=torch.uint8, device=dev)

    def put(name, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            assert name + "/" + k not in out, name
            out[name + "/" + k] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def call(rc, what):
        L.check(rc, what)

    def loss_step(name, xd, td, n, per, heads, kind):
        """all four forms: with / without meters, scaled / unscaled"""
        need = lib.nunet_loss_step_ws_bytes(n, per, heads, kind)
        seed = torch.tensor([1024.0], device=dev)
        for scaled in (0, 1):
            for with_m in (0, 1):
                ws, dx, lo = buf(need), buf(4 * xd.numel()), buf(4 * (heads + 1))
                m = torch.tensor([0.25, 0.5, -1.0, -1.0], dtype=torch.float64, device=dev)
                args = (L.ptr(xd), L.ptr(td), n, per, heads, kind, L.ptr(ws), need, L.ptr(dx), L.ptr(lo), L.ptr(m) if with_m else None, thr)
                if scaled:
                    call(lib.nunet_loss_step_scaled(*args, L.ptr(seed), L.stream()), "nunet_loss_step_scaled")
                else:
                    call(lib.nunet_loss_step(*args, L.stream()), "nunet_loss_step")
                put("%s/scaled%d/meters%d" % (name, scaled, with_m), ws=ws, dlogits=dx, loss_out=lo, meters=m)

    # BCE-Dice: the stand-alone pair and the step
    for case in LC.CASES + LC.SOFT_UNIFORM_CASES:
        kind, n, per, heads, _ = case
        x, t = LC.build(case)
        xd, td = x.contiguous().to(dev), t.contiguous().to(dev)
        name = "bce_dice/" + LC.case_id(case)
        if kind == "alone":
            need = lib.nunet_bce_dice_ws_bytes(n)
            ws, loss, dx = buf(need), buf(4), buf(4 * xd.numel())
            call(lib.nunet_bce_dice_fwd(L.ptr(xd), L.ptr(td), n, per, L.ptr(ws), need, L.ptr(loss), L.stream()), "nunet_bce_dice_fwd")
            put(name + "/fwd", ws=ws, loss=loss)
            for g in (None, torch.tensor([0.375], device=dev)):
                call(lib.nunet_bce_dice_bwd(L.ptr(xd), L.ptr(td), n, per, L.ptr(ws), need, L.ptr(g), L.ptr(dx), L.stream()), "nunet_bce_dice_bwd")
                put(name + "/bwd/g%d" % (g is not None), ws=ws, dlogits=dx)
            cnt = torch.zeros(2, dtype=torch.int64, device=dev)
            call(lib.nunet_iou_counts(L.ptr(xd), L.ptr(td), xd.numel(), thr, L.ptr(cnt), L.stream()), "nunet_iou_counts")
            put(name + "/iou_counts", counts=cnt)
            u8, th = buf(xd.numel()), sigmoid_u8_thresholds(torch.device(dev))
            call(lib.nunet_sigmoid_u8(L.ptr(xd), L.ptr(th), L.ptr(u8), xd.numel(), L.stream()), "nunet_sigmoid_u8")
            put(name + "/sigmoid_u8", out=u8)
        else:
            loss_step(name, xd, td, n, per, heads, L.LOSS_BCE_DICE)

    # BCEWithLogits: the stand-alone pair and the step
    for case in BC.CASES:
        kind, n, per, heads, _ = case
        x, t = LC.build(case)
        xd, td = x.contiguous().to(dev), t.contiguous().to(dev)
        name = "bce_logits/" + LC.case_id(case)
        if kind == "alone":
            cnt_ = xd.numel()
            need = lib.nunet_bce_logits_ws_bytes(cnt_)
            ws, loss, dx = buf(need), buf(4), buf(4 * cnt_)
            call(lib.nunet_bce_logits_fwd(L.ptr(xd), L.ptr(td), cnt_, L.ptr(ws), need, L.ptr(loss), L.stream()), "nunet_bce_logits_fwd")
            put(name + "/fwd", ws=ws, loss=loss)
            for g in (None, torch.tensor([0.375], device=dev)):
                call(lib.nunet_bce_logits_bwd(L.ptr(xd), L.ptr(td), cnt_, L.ptr(g), L.ptr(dx), L.stream()), "nunet_bce_logits_bwd")
                put(name + "/bwd/g%d" % (g is not None), dlogits=dx)
        else:
            loss_step(name, xd, td, n, per, heads, L.LOSS_BCE_LOGITS)

    # Lovasz hinge inside the step: heads 1 and 4 (head j > 0: the case's labels under other errors)
    for case in VC.CASES:
        shape, pattern = case
        n, per = shape[0], shape[1] * shape[2]
        if n * per > (1 << 20):
            continue
        for heads in (1, 4):
            xs = [VC.build(shape, pattern, j, None if j == 0 else (pattern, 0))[0] for j in range(heads)]
            xd = torch.stack(xs).reshape(heads, n, per).contiguous().to(dev)
            td = VC.build(shape, pattern)[1].reshape(n, per).contiguous().to(dev)
            loss_step("lovasz/%s/h%d" % (VC.case_id(case), heads), xd, td, n, per, heads, L.LOSS_LOVASZ_HINGE)

    # segmentation sums (assign, then accumulate) and both eval steps, every loss kind, heads 1 and 4 (nunet_eval_step: 8 too)
    kinds = {"bce_dice": L.LOSS_BCE_DICE, "lovasz": L.LOSS_LOVASZ_HINGE, "bce_logits": L.LOSS_BCE_LOGITS}
    for case in EC.CASES:
        n, k, hw, pattern = case
        x, t = EC.build(case)
        xd, td = x.to(dev), t.to(dev)
        name = "eval/" + EC.case_id(case)
        need = lib.nunet_seg_metrics_ws_bytes(n, k, hw)
        ws, sums = buf(need), buf(C.sizeof(L.SegSums))
        for acc in (0, 1):
            call(lib.nunet_seg_metrics(L.ptr(xd), L.ptr(td), n, k, hw, thr, L.ptr(ws), need, L.ptr(sums), acc, L.stream()), "nunet_seg_metrics")
            put(name + "/seg_metrics/acc%d" % acc, ws=ws, sums=sums)
        if pattern == "nan" or n * k * hw > (1 << 18):
            continue
        for kn, kind in kinds.items():
            if kind == L.LOSS_LOVASZ_HINGE and k != 1:
                continue
            for heads in (1, 4, 8):
                hs = torch.stack([x * (0.5 + 0.25 * j) + 0.1 * (heads - 1 - j) for j in range(heads - 1)] + [x]).contiguous().to(dev)
                msz = C.sizeof(L.EvalMeters)
                need = lib.nunet_eval_step_ws_bytes(n, k, hw, heads, kind)
                ws, lo, m = buf(need), buf(4 * (heads + 1)), torch.zeros(msz, dtype=torch.uint8, device=dev)
                for rep in (0, 1):
                    call(lib.nunet_eval_step(L.ptr(hs), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need, L.ptr(lo), L.ptr(m), thr, L.stream()), "nunet_eval_step")
                    put("%s/eval_step/%s/h%d/call%d" % (name, kn, heads, rep), ws=ws, loss_out=lo, meters=m)
                if heads > 4:
                    continue
                need = lib.nunet_eval_step_heads_ws_bytes(n, k, hw, heads, kind)
                ws, lo, m, hm = buf(need), buf(4 * (heads + 1)), torch.zeros(msz, dtype=torch.uint8, device=dev), torch.zeros(heads * msz, dtype=torch.uint8, device=dev)
                for rep in (0, 1):
                    call(lib.nunet_eval_step_heads(L.ptr(hs), L.ptr(td), n, k, hw, heads, kind, L.ptr(ws), need, L.ptr(lo), L.ptr(m), L.ptr(hm), thr, L.stream()),
                         "nunet_eval_step_heads")
                    put("%s/eval_step_heads/%s/h%d/call%d" % (name, kn, heads, rep), ws=ws, loss_out=lo, meters=m, head_meters=hm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: compare its digests with this commit's")
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is loaded")
    ap.add_argument("--out", default=os.path.join("profiles", "loss_parity_digest.json"))
    a = ap.parse_args()
    if not a.parent:
        print(json.dumps(digests()))
        return
    runs = parent_compare.alternate(__file__, a.parent, [], 1)
    pa, th = runs["parent"][0], runs["this"][0]
    differ = sorted(k for k in set(pa) | set(th) if pa.get(k) != th.get(k))
    res = {"method": "tools/loss_parity_digest.py --parent: SHA-256 of every output buffer and of the whole workspace after each call",
           "digests": len(th), "equal": len(th) - len([k for k in differ if k in th]), "differ": differ}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if differ or len(pa) != len(th):
        raise SystemExit("%d digests differ: %s" % (len(differ), ", ".join(differ[:20])))


if __name__ == "__main__":
    main()
