"""Weight EMA under data parallel, rehearsed on ONE MI355X (the pattern of test_clip_dist_gpu.py: two ranks share the GPU over
gloo). The ranks are built from different parameters (hence different initial averages) and with different decays: rank 0's
become everyone's at construction. After three steps on different batches the averaged parameters and n_averaged are
bit-identical across ranks without any collective - the average is a deterministic function of identical parameters - and within
the bound of tests/test_ema_gpu.py of the fp64 recurrence on the rank-common parameter trajectory. BatchNorm running statistics
are per replica in this project (rank 0's are the model's, sync_bn_buffers()), so each rank's averaged statistics are checked
against the recurrence on its own buffers, and are bit-identical across ranks once sync_bn_buffers() has run."""
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch

from dist_cases import run_ranks

pytestmark = pytest.mark.gpu

T = 3
EPS = 2.0 ** -24


def _worker(rank, world, port, q):
    os.environ.update(NUNET_DP_MODE="1", RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import nunet_amd
    from nunet_amd.trainer import TrainStep
    EMA = importlib.import_module("pytorch_nested-unet_amd.ema")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    synth = nunet_amd.synth
    st = synth.closed_form_state(1, 3, False, True, salt=rank)      # ranks start from different parameters
    m = nunet_amd.archs.NestedUNet(1, 3, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()

    def digest(t):
        """sha256 of a tensor's bytes: equal exactly when the tensors are bit-identical (36 MB arenas stay in the worker)"""
        return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
    own = digest(m.engine().flat_params)
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-2, use_graph=False, ema_decay=0.9 if rank == 0 else 0.5, ema_warmup=rank == 0)
    print("executor_choice", ts.executor_choice)
    torch.cuda.synchronize()
    built = dict(decay=ts.ema_decay, warmup=ts.ema_warmup, stats=ts.ema_stats(), own=own,
                 params=digest(ts.eng.flat_params), ema=digest(ts.ema_params), ema_bn=ts.ema_bnbuf.cpu().numpy().copy())
    rec = EMA.Recurrence(ts.ema_decay, ts.ema_warmup)
    big = [0.0, 0.0]
    sums = []
    for k in range(T):
        img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=900 + 10 * k + rank)      # every rank its own batch
        ts.step(torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda())
        torch.cuda.synchronize()
        rec.update([ts.eng.flat_params, ts.eng.bnbuf])
        big = [max(big[0], float(ts.eng.flat_params.abs().max())), max(big[1], float(ts.eng.bnbuf.abs().max()))]
        sums.append((float(ts.eng.flat_params.double().sum()), ts.ema_stats()))
    errs = []
    for dev, ref, b in ((ts.ema_params, rec.values[0], big[0]), (ts.ema_bnbuf, rec.values[1], big[1])):
        b = max(b, float(dev.abs().max()), float(ref.abs().max()))
        errs.append((float((dev.double().cpu() - ref).abs().max()), 5.0 * T * EPS * b))
    local_bn = ts.ema_bnbuf.cpu().numpy().copy()
    ts.sync_bn_buffers()
    torch.cuda.synchronize()
    done = dict(params=digest(ts.eng.flat_params), ema=digest(ts.ema_params), local_bn=local_bn,
                ema_bn=ts.ema_bnbuf.cpu().numpy().copy(), bn=ts.eng.bnbuf.cpu().numpy().copy(), stats=ts.ema_stats(), w=rec.w,
                errs=errs, sums=sums)
    q.put((rank, built, done))
    dist.destroy_process_group()


def test_two_ranks_keep_one_average():
    res = run_ranks(_worker, 2)
    (b0, d0), (b1, d1) = res[0], res[1]
    # construction: rank 0's decay, warm-up flag and averages are everyone's
    assert (b0["decay"], b0["warmup"]) == (b1["decay"], b1["warmup"]) == (0.9, True)
    assert b0["stats"] == b1["stats"] == dict(n_averaged=0, w=0.0)
    assert b0["own"] != b1["own"]                                    # they did start apart (digests of the arenas)
    assert b0["params"] == b1["params"] == b0["own"]
    assert b0["ema"] == b1["ema"] == b0["own"]
    assert np.array_equal(b0["ema_bn"], b1["ema_bn"])
    # three steps on different batches
    assert d0["sums"] == d1["sums"]                                  # one parameter trajectory, one n_averaged / w per step
    assert d0["params"] == d1["params"] != b0["params"]
    assert d0["ema"] == d1["ema"]                                    # bit-identical averages, no collective
    assert d0["stats"] == d1["stats"] and d0["stats"]["n_averaged"] == T and d0["stats"]["w"] == d0["w"] == d1["w"]
    for d in (d0, d1):
        for what, (err, bound) in zip(("ema_params", "ema_bnbuf"), d["errs"]):
            print("%s: max |ema - fp64 recurrence| %.3e, bound %.3e" % (what, err, bound))
            assert err <= bound, (what, err, bound)
    assert not np.array_equal(d0["local_bn"], d1["local_bn"])        # per-replica batch statistics, per-replica averages of them
    assert np.array_equal(d0["ema_bn"], d0["local_bn"])              # ... and rank 0's are the model's
    assert np.array_equal(d0["ema_bn"], d1["ema_bn"]) and np.array_equal(d0["bn"], d1["bn"])
    assert d0["ema"] != d0["params"]
