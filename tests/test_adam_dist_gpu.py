"""Data-parallel Adam rehearsal on ONE MI355X (the pattern of test_dist_gpu.py: two ranks share the GPU over gloo): the
replicas stay identical (rank 1 starts from other parameters and BatchNorm buffers, replaced by rank 0's at construction), the
update is Adam on the rank-mean gradient, and broadcast_state carries the Adam state and step."""
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
    st = synth.closed_form_state(1, 3, False, True) if rank == 0 else synth.closed_form_state(1, 3, False, False, salt=7)
    m = nunet_amd.archs.NestedUNet(1, 3, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-3, weight_decay=1e-4, use_graph=use_graph, optimizer="Adam")
    if rank == 1:
        # a differing optimiser state on rank 1 (as after loading a checkpoint there): broadcast_state makes rank 0's - zero
        # moments, t = 0 - every rank's, the call the constructor makes for the parameters and BatchNorm buffers
        ts.exp_avg.fill_(0.25); ts.exp_avg_sq.fill_(0.5); ts.adam_step.fill_(7.0)
    ts.broadcast_state()
    assert ts.world == 2
    init = (float(ts.exp_avg.abs().max()), float(ts.exp_avg_sq.abs().max()), float(ts.adam_step))
    img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=500 + rank)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    if use_graph:
        ts.capture(x, t)
    ts.step(x, t)
    torch.cuda.synchronize()
    w = m.conv0_4.conv2.weight.detach().cpu().clone()
    g = m.conv0_4.conv2.weight.grad.detach().cpu().clone()      # rank MEAN
    ts.step(x, t)
    torch.cuda.synchronize()
    q.put((rank, w.numpy(), g.numpy(), ts.eng.flat_params.cpu().numpy(), ts.exp_avg.cpu().numpy(), float(ts.adam_step), init))
    dist.destroy_process_group()


@pytest.mark.parametrize("use_graph,dp_mode", [(False, 1), (True, 1), (True, "auto")])
def test_two_rank_data_parallel_adam_step(use_graph, dp_mode, synth):
    import nunet_amd
    res = run_ranks(_worker, 2, use_graph, dp_mode)
    # rank 0's optimiser state (zeros, t = 0) replaced rank 1's
    assert res[0][5] == (0.0, 0.0, 0.0) and res[1][5] == (0.0, 0.0, 0.0)
    # replicas identical after one and after two steps; two steps counted
    for k in range(4):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert res[0][4] == 2.0 and res[1][4] == 2.0
    # Adam's first step on the mean of the two shards' single-process gradients reproduces the DP update
    st = synth.closed_form_state(1, 3, False, True)
    grads = []
    for rank in range(2):
        m = nunet_amd.archs.NestedUNet(1, 3, False)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
        m = m.cuda().train()
        img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=500 + rank)
        loss = nunet_amd.losses.BCEDiceLoss()(m(torch.from_numpy(img).cuda()), torch.from_numpy(msk).cuda())
        loss.backward()
        grads.append(m.conv0_4.conv2.weight.grad.detach().cpu().double().numpy())
    gmean = (grads[0] + grads[1]) / 2
    assert np.abs(res[0][1] - gmean).max() <= 2e-2 * np.abs(gmean).max()
    w0 = np.asarray(st["conv0_4.conv2.weight"]).astype(np.float64)
    gd = gmean + 1e-4 * w0
    # t = 1: m = 0.1 g, v = 0.001 g^2, step = lr / 0.1 * m / (sqrt(v) / sqrt(0.001) + eps) = lr * g / (|g| + eps)
    expect = w0 - 1e-3 * gd / (np.abs(gd) + 1e-8)
    dw, dref = res[0][0] - w0, expect - w0
    # elements whose gradient is within the gradient error of zero may move the other way (see test_adam_gpu.py): bounded in norm
    assert np.linalg.norm(dw - dref) <= 0.05 * np.linalg.norm(dref), np.linalg.norm(dw - dref) / np.linalg.norm(dref)
