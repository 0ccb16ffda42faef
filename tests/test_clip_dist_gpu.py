"""Gradient-norm clipping under data parallel, rehearsed on ONE MI355X (the pattern of test_loss_scale_dist_gpu.py: two ranks share
the GPU over gloo): the norm is taken after the exchange, so both ranks report the same norm bit for bit - the fp64 norm of the
rank-mean p.grad / coef - from different batches, apply the same factor without any extra collective and stay identical; rank
0's max_norm replaces rank 1's at construction."""
import os

import numpy as np
import pytest
import torch

from dist_cases import run_ranks

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    os.environ.update(NUNET_DP_MODE="1", RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import nunet_amd
    from nunet_amd.trainer import TrainStep
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    synth = nunet_amd.synth
    st = synth.closed_form_state(1, 3, False, True)

    def module():
        m = nunet_amd.archs.NestedUNet(1, 3, False)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
        return m.cuda().train()
    img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=700 + rank)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    # the norm of the rank-mean gradient, measured beforehand (lr = 0, inf: nothing moves, nothing is clipped)
    m0 = module()
    probe = TrainStep(m0, (2, 3, 32, 32), lr=0.0, use_graph=False, clip_grad_norm=float("inf"))
    probe.step(x, t)
    n0 = probe.grad_norm_stats()["last"]
    del probe, m0
    m = module()
    # ranks built with different thresholds: rank 0's is broadcast with the rest of the replica state
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-2, use_graph=False, clip_grad_norm=0.25 * n0 if rank == 0 else 1e6)
    print("executor_choice", ts.executor_choice)
    torch.cuda.synchronize()
    max_norm = float(ts._clip.cpu()[0:1].view(torch.float32))
    out = []
    for k in range(2):
        ts.step(x, t)
        s = ts.grad_norm_stats()
        coef = float(ts._clip.cpu()[1:2].view(torch.float32))
        gn = float(torch.linalg.vector_norm(torch.cat([p.grad.detach().double().reshape(-1) for p in m.parameters()])))
        out.append((s, coef, gn, ts.eng.flat_params.cpu().numpy().copy()))
    q.put((rank, n0, max_norm, out))
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_norm():
    res = run_ranks(_worker, 2)
    n0 = res[0][0]
    assert res[1][0] == n0                                   # the probe already saw the exchanged gradient on both ranks
    want = float(torch.tensor(0.25 * n0, dtype=torch.float32))
    assert res[0][1] == res[1][1] == want                    # rank 0's max_norm won at construction
    for k in range(2):
        (s0, c0, g0, p0), (s1, c1, g1, p1) = res[0][2][k], res[1][2][k]
        print("step %d: norm %.9g coef %.9g, fp64 ||p.grad|| / coef %.17g" % (k, s0["last"], c0, g0 / c0))
        assert s0 == s1 and c0 == c1 and g0 == g1            # the same norm, bit for bit, from different batches
        assert c0 < 1.0 and s0["clipped"] == k + 1 and s0["steps"] == k + 1
        assert abs(s0["last"] - g0 / c0) <= 1e-6 * s0["last"]
        assert np.array_equal(p0, p1), k
    assert abs(res[0][2][0][0]["last"] - n0) <= 1e-6 * n0
    assert not np.array_equal(res[0][2][0][3], res[0][2][1][3])
