"""Data-parallel rehearsal on ONE MI355X: two ranks share the GPU, gradients are exchanged with
gloo (RCCL cannot put two ranks on one device). Checks the DP step (trainer.TrainStep, world=2):
replicas stay identical and the update equals SGD on the rank-averaged gradient."""
import os

import numpy as np
import pytest
import torch

from dist_cases import run_ranks

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, use_graph, dp_mode, q):
    os.environ.update(NUNET_DP_MODE=str(dp_mode), RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import nunet_amd
    from nunet_amd.trainer import TrainStep
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    synth = nunet_amd.synth
    # rank 0 holds the closed-form state, rank 1 a different one (salt) with non-trivial BN buffers: the TrainStep
    # broadcasts rank 0's parameters / momentum / BatchNorm buffers at construction, like DistributedDataParallel
    st = synth.closed_form_state(1, 3, False, True) if rank == 0 else synth.closed_form_state(1, 3, False, False, salt=7)
    m = nunet_amd.archs.NestedUNet(1, 3, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-2, momentum=0.9, weight_decay=1e-4, use_graph=use_graph)
    assert ts.world == 2
    ref0 = synth.closed_form_state(1, 3, False, True)
    sd0 = m.state_dict()
    for k in ("conv0_0.conv1.weight", "conv4_0.bn2.running_var", "conv2_1.bn1.num_batches_tracked", "final.bias"):
        assert np.array_equal(sd0[k].cpu().numpy(), np.asarray(ref0[k])), k
    img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=500 + rank)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    if use_graph:
        ts.capture(x, t)
    ts.step(x, t)
    torch.cuda.synchronize()
    w = m.conv0_4.conv2.weight.detach().cpu().clone()
    g = m.conv0_4.conv2.weight.grad.detach().cpu().clone() * world     # p.grad is the rank MEAN in every layout
    ts.step(x, t)
    torch.cuda.synchronize()
    # BatchNorm running statistics are per replica during training (different shards); the policy makes rank 0's the model's
    rv_local = m.conv0_0.bn1.running_var.detach().cpu().numpy().copy()
    ts.sync_bn_buffers()
    rv_synced = m.conv0_0.bn1.running_var.detach().cpu().numpy().copy()
    q.put((rank, w.numpy(), g.numpy(), m.conv3_1.conv1.weight.detach().cpu().numpy(), ts.epoch_stats(), rv_local, rv_synced))
    dist.destroy_process_group()


@pytest.mark.parametrize("use_graph,dp_mode", [(False, 1), (True, 1), (True, "auto")])
def test_two_rank_data_parallel_step(use_graph, dp_mode, synth):
    import nunet_amd
    res = run_ranks(_worker, 2, use_graph, dp_mode)
    # replicas identical after one and after two steps
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][1], res[1][1])
    # single-process evaluation of each shard's gradient -> SGD on their mean reproduces the DP update
    st = synth.closed_form_state(1, 3, False, True)
    grads = []
    for rank in range(2):
        m = nunet_amd.archs.NestedUNet(1, 3, False)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
        m = m.cuda().train()
        img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=500 + rank)
        loss = nunet_amd.losses.BCEDiceLoss()(m(torch.from_numpy(img).cuda()), torch.from_numpy(msk).cuda())
        loss.backward()
        grads.append(m.conv0_4.conv2.weight.grad.detach().cpu().numpy())
    gsum = grads[0] + grads[1]
    assert np.abs(res[0][1] - gsum).max() <= 2e-2 * np.abs(gsum).max()
    w0 = st["conv0_4.conv2.weight"]
    expect = w0 - 1e-2 * (gsum / 2 + 1e-4 * w0)
    assert np.abs(res[0][0] - expect).max() <= 2e-2 * 1e-2 * np.abs(gsum).max() + 1e-7
    assert np.isfinite(res[0][3][0]) and abs(res[0][3][0] - res[1][3][0]) < 0.5
    # BN buffer policy: local statistics differ between the replicas, after sync_bn_buffers() both hold rank 0's
    assert not np.array_equal(res[0][4], res[1][4])
    assert np.array_equal(res[0][5], res[0][4]) and np.array_equal(res[1][5], res[0][4])


def _rccl_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("NUNET_DP_MODE", None)                 # auto: layouts 1 and 3 are timed, the faster is kept
    import torch.distributed as dist
    import nunet_amd
    from nunet_amd.trainer import TrainStep
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    synth = nunet_amd.synth
    torch.manual_seed(100 + rank)                          # ranks initialise differently: the TrainStep broadcasts rank 0's state
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="bf16").cuda().train()
    ts = TrainStep(m, (16, 3, 96, 96), lr=1e-2)
    assert ts.world == world and ts.dp
    img, msk = synth.synth_batch(16, 96, 96, 3, 1, seed=700 + rank)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    ts.capture(x, t)
    for _ in range(3):
        ts.step(x, t)
    torch.cuda.synchronize()
    loss, _ = ts.epoch_stats()
    w = m.conv3_1.conv1.weight.detach().float().cpu().numpy()
    q.put((rank, w, loss, ts.dp_mode, ts.dp_choice))
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL cannot put two ranks on one device")
def test_rccl_two_gpus_replicas_stay_identical():
    """The real exchange: two ranks on two GPUs over RCCL, step layout chosen by measurement (NUNET_DP_MODE auto).
    Replicas that were initialised differently are identical after construction and stay identical through training."""
    res = run_ranks(_rccl_worker, 2)
    assert np.array_equal(res[0][0], res[1][0])
    assert np.isfinite(res[0][1]) and np.isfinite(res[1][1])
    assert res[0][2] == res[1][2] and res[0][2] in (1, 3)          # the same measured layout on both ranks
    print("layout chosen:", res[0][2], "ms per layout:", res[0][3])


def _in_graph_worker(rank, world, port, q):
    os.environ.update(NUNET_FORCE_DP="1", NUNET_DEBUG_SPIN_US="2000", RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ctypes as C
    import torch.distributed as dist
    import nunet_amd
    from nunet_amd import _lib as L
    from nunet_amd import trainer as TR
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    synth = nunet_amd.synth
    batches = []
    for k in range(3):
        img, msk = synth.synth_batch(16, 96, 96, 3, 1, seed=900 + k)
        batches.append((torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()))
    out = {}
    for mode in (1, 3):
        os.environ["NUNET_DP_MODE"] = str(mode)
        torch.manual_seed(0)
        m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="bf16").cuda().train()
        ts = TR.TrainStep(m, (16, 3, 96, 96), lr=1e-2)
        assert ts.dp and ts.dp_mode == mode
        stamps = torch.zeros(4, dtype=torch.int64, device="cuda")
        snap = torch.zeros_like(ts._buckets[0])
        calls = []
        real = dist.all_reduce
        if mode == 3:
            # every exchange the step issues also leaves a device timestamp (and, for bucket 0, a snapshot) on the stream it was
            # issued on: "when were this bucket's producers done" as seen from inside the graph
            def spy(t, *a, **kw):
                k = len(calls) % 2
                calls.append(torch.cuda.current_stream().cuda_stream)
                L.check(L.lib().nunet_debug_stamp(L.ptr(stamps, 8 * k), L.stream()), "stamp")
                if k == 0:
                    snap.copy_(t, non_blocking=True)
                return real(t, *a, **kw)
            TR.dist.all_reduce = spy
        ts.capture(*batches[0])
        if mode == 3:
            TR.dist.all_reduce = real
            assert ts.g_fb is not None and ts.g_opt is None           # the whole step, exchanges included, is ONE graph
            assert len(calls) >= 2 and calls[-2] != calls[-1]         # bucket 0 went to a side stream, bucket 1 to the caller's
        leads = []
        for x, t in batches:
            if mode == 3:
                snap.zero_()
            ts.step(x, t)
            if mode == 3:
                L.check(L.lib().nunet_debug_stamp(L.ptr(stamps, 16), L.stream()), "stamp")      # end of the step, caller's stream
                torch.cuda.synchronize()
                tk = stamps.tolist()
                leads.append(((tk[2] - tk[0]) / 100e3, (tk[2] - tk[1]) / 100e3))       # ms: bucket-0-ready -> end, bucket-1-ready -> end
                assert torch.equal(snap, ts._buckets[0]) and float(snap.abs().sum()) > 0   # world 1: the exchange is the identity
        torch.cuda.synchronize()
        out[mode] = (ts.eng.flat_params.clone().cpu(), ts.mom.clone().cpu(), ts.epoch_stats(), leads)
        del ts, m
    q.put((rank, bool(torch.equal(out[1][0], out[3][0]) and torch.equal(out[1][1], out[3][1])), out[1][2], out[3][2], out[3][3]))
    dist.destroy_process_group()


def test_exchange_inside_the_step_graph_overlaps_phase_two():
    """NUNET_DP_MODE=3: the data-parallel step is ONE graph that contains both gradient exchanges. Rehearsed with a single-rank
    RCCL group (the collectives are real calls into torch.distributed, captured into the graph):
      * it computes exactly what layout 1 computes (bit-identical parameters and momentum after three steps),
      * the first bucket's exchange sits on a side branch that is released by its producing kernels, not by the end of the pass:
        with a 2 ms spin kernel heading phase 2 (NUNET_DEBUG_SPIN_US) the bucket is ready - and bitwise final - more than 1 ms
        before the step ends, while the second bucket is ready only at the end of the pass."""
    same, s1, s3, leads = run_ranks(_in_graph_worker, 1, polls=200)[0]
    assert same, "layout 3 must compute what layout 1 computes"
    assert s1 == s3 and np.isfinite(s1[0])
    print("ms from bucket-ready to the end of the step (bucket 0, bucket 1):", leads)
    assert min(l[0] for l in leads) > 1.0, leads          # bucket 0 was ready > 1 ms before the end (phase 2 + its 2 ms spin ran beside it)
    assert max(l[1] for l in leads) < min(l[0] for l in leads)   # bucket 1 only after the whole pass
