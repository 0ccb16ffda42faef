"""Bit identity of the plan's passes, the weight-layout kernels and the lane scheduler between two checkouts: SHA-256 of the
training state after three steps of four tiny configurations, each run eager on one lane, eager on the lanes, captured as one
hipGraph (segmented False, schedule 'lanes') and as the flag-synchronised program ('flags', 'list'); of a pruned eval forward; of
the stand-alone weight pack / gradient unpack; of the gradient square norm's workspace; and of the text the list scheduler prints
for one eager pass with its built-in costs (NUNET_LIST_DEBUG=2: order, lane, simulated start and cost of every op). A one-off
comparison tool for a change that must not move a bit, as tools/loss_parity_digest.py is for the losses.

    python tools/step_parity_digest.py --parent DIR [--out profiles/plan_split_parity.json]    DIR: a built checkout of the parent commit
    python tools/step_parity_digest.py [--tree DIR]                                            the digests of one checkout, as JSON

--parent runs one process per checkout (tools/parent_compare.py picks the package by --tree), compares digest by digest and
exits non-zero if any differs.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import parent_compare  # noqa: E402

sys.path.insert(0, parent_compare.tree())

STEPS = 3
FORMS = {"eager_1lane": dict(use_graph=False), "eager_lanes": dict(use_graph=False),
         "graph_lanes": dict(segmented=False, schedule="lanes"), "flags_list": dict(segmented="flags", schedule="list")}


def cases():
    import nunet_amd
    A = nunet_amd.archs
    return {"nested_ds_n2_32x32_bf16_sgd": (lambda: A.NestedUNet(1, 3, True, dtype="bf16"), (2, 3, 32, 32), {}),
            "nested_n3_48x32_fp16_adam_scale_clip_ema": (lambda: A.NestedUNet(1, 3, False, dtype="fp16"), (3, 3, 48, 32),
                                                         dict(optimizer="Adam", loss_scale="dynamic", clip_grad_norm=1.0, ema_decay=0.9)),
            "unet_n2_32x32_fp32_sgd": (lambda: A.UNet(1, 3, False, dtype="fp32"), (2, 3, 32, 32), {}),
            "nested_n2_32x32_bf16_unfused": (lambda: A.NestedUNet(1, 3, False, dtype="bf16"), (2, 3, 32, 32), dict(fused_update=0))}


def digests():
    os.environ["NUNET_LIST_DEBUG"] = "2"      # (read once per process, at the first list-scheduled pass)
    import torch
    import nunet_amd
    from nunet_amd import _lib as L
    from nunet_amd.synth import synth_batch
    from nunet_amd.trainer import EvalStep, TrainStep

    dev, lib = "cuda:0", L.lib()
    out = {}

    def put(name, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            assert name + "/" + k not in out, name
            out[name + "/" + k] = hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def batch(shape, seed):
        img, msk = synth_batch(shape[0], shape[2], shape[3], shape[1], 1, seed=seed)
        return torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev)

    def model(make, sd):
        m = make()
        m.load_state_dict(sd)
        return m.to(dev).train()

    for cname, (make, shape, kw) in cases().items():
        torch.manual_seed(7)
        sd = {k: v.clone() for k, v in make().state_dict().items()}
        batches = [batch(shape, 500 + k) for k in range(STEPS)]
        for fname, form in FORMS.items():
            m = model(make, sd)
            ts = TrainStep(m, shape, lr=1e-2, keep_grads=True, **dict(kw, **form))
            if fname == "eager_1lane":
                L.check(lib.nunet_plan_set_multistream(ts.pl.handle, 0), "plan_set_multistream")
            ts.capture(*batches[0])
            for x, t in batches:
                ts.step(x, t)
            name = cname + "/" + fname
            state = dict(flat_params=ts.eng.flat_params, bnbuf=ts.eng.bnbuf, nbt=ts.eng.nbt, flat_grads=ts.eng.flat_grads, logits=ts.logits,
                         loss_out=ts.loss_out, meters=ts.meters)
            state.update({"opt_state%d" % q: t for q, t in enumerate(ts.opt_state)})
            state.update({"aux%d" % q: t for q, t in enumerate(ts._aux_state())})
            state.update({"ema_arena%d" % q: t for q, t in enumerate(ts._ema_arenas())})
            put(name, **state)
            if fname == "eager_lanes" and ts.fused_update:
                # the square norm of the gradient scratch the last backward pass left
                nb = lib.nunet_plan_grad_sqnorm_ws_bytes(ts.pl.handle)
                ws = torch.full((nb // 8,), -1.0, dtype=torch.float64, device=dev)
                L.check(lib.nunet_plan_grad_sqnorm(ts.pl.handle, L.ptr(ts.pl.arena), L.nbytes(ts.pl.arena), L.ptr(ws), nb, L.stream()), "plan_grad_sqnorm")
                put(name + "/grad_sqnorm", ws=ws)
            if fname == "eager_lanes" and cname.startswith("nested_ds"):
                ev = EvalStep(m.eval(), shape, depth=2, use_graph=False)
                ev.step(*batches[0])
                put(cname + "/pruned_depth2_eval", logits=ev.main.logits)
                m.train()
                # one eager forward + backward under the list scheduler with its built-in costs: what it prints is the schedule
                L.check(lib.nunet_plan_set_schedule(ts.pl.handle, 2), "plan_set_schedule")
                torch.cuda.synchronize()
                with tempfile.TemporaryFile() as f:
                    sys.stderr.flush()
                    keep = os.dup(2)
                    os.dup2(f.fileno(), 2)
                    try:
                        ts._fwd_loss()
                        ts._bwd(3)
                        torch.cuda.synchronize()
                    finally:
                        os.dup2(keep, 2)
                        os.close(keep)
                    f.seek(0)
                    text = f.read()
                assert text.count(b"(built-in costs)") == 2 and text.count(b"\n") > 60, text[:400]
                out[cname + "/list_schedule_text/sha256_of_%d_lines" % text.count(b"\n")] = hashlib.sha256(text).hexdigest()
            del ts, m

    # the stand-alone weight pack (every dtype) and gradient unpack (overwrite, then accumulate)
    g = torch.Generator().manual_seed(11)
    for cout, cin, cinpad in ((40, 3, 32), (64, 96, 96)):
        w = torch.randn((cout, cin, 3, 3), generator=g).to(dev)
        for dn, dt in (("fp32", L.F32), ("bf16", L.BF16), ("fp16", L.F16)):
            es = 4 if dt == L.F32 else 2
            nwf = (9 * cout * cinpad * es + 255) // 256 * 256
            buf = torch.full((nwf + 9 * cout * cin * es,), 0xC3, dtype=torch.uint8, device=dev)
            L.check(lib.nunet_pack_weights(L.ptr(w), cout, cin, cinpad, dt, buf.data_ptr(), buf.data_ptr() + nwf, L.stream()), "pack_weights")
            put("pack_weights/%dx%d/%s" % (cout, cin, dn), packed=buf)
        dw = torch.randn((9, cout, cinpad), generator=g).to(dev)
        gr = torch.full((cout * cin * 9,), 0.5, device=dev)
        for acc in (0, 1):
            L.check(lib.nunet_unpack_wgrad(L.ptr(dw), cout, cin, cinpad, L.ptr(gr), acc, L.stream()), "unpack_wgrad")
            put("unpack_wgrad/%dx%d/acc%d" % (cout, cin, acc), grads=gr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: compare its digests with this commit's")
    ap.add_argument("--tree", default=None, help="(child) the checkout whose package is loaded")
    ap.add_argument("--out", default=os.path.join("profiles", "plan_split_parity.json"))
    a = ap.parse_args()
    if not a.parent:
        print(json.dumps(digests()))
        return
    runs = parent_compare.alternate(__file__, a.parent, [], 1)
    pa, th = runs["parent"][0], runs["this"][0]
    differ = sorted(k for k in set(pa) | set(th) if pa.get(k) != th.get(k))
    res = {"method": "tools/step_parity_digest.py --parent: SHA-256 of the training state after %d steps in every executor form, of a pruned eval "
                     "forward, of the stand-alone pack / unpack, of the square-norm workspace and of the list scheduler's debug text" % STEPS,
           "digests": len(th), "equal": len(th) - len([k for k in differ if k in th]), "differ": differ, "names": sorted(th)}
    print(json.dumps({k: v for k, v in res.items() if k != "names"}))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if differ or len(pa) != len(th):
        raise SystemExit("%d digests differ: %s" % (len(differ), ", ".join(differ[:20])))


if __name__ == "__main__":
    main()
