"""Dynamic loss scaling under data parallel, rehearsed on ONE MI355X (the pattern of test_dist_gpu.py: two ranks share the GPU
over gloo): rank 0's scaler state replaces rank 1's at construction, and an inf that only rank 1's gradient holds before the
exchange makes BOTH ranks skip the step (the exchange carries it; no extra collective) and back off identically."""
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
    m = nunet_amd.archs.NestedUNet(1, 3, False, dtype="fp16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.cuda().train()
    ts = TrainStep(m, (2, 3, 32, 32), lr=1e-2, use_graph=False, loss_scale=dict(init_scale=1024.0 if rank == 0 else 8.0))
    print("executor_choice", ts.executor_choice)
    init = ts.scaler_stats()
    img, msk = synth.synth_batch(2, 32, 32, 3, 1, seed=600 + rank)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    out = []
    ts.step(x, t)                                    # a clean step
    out.append((ts.scaler_stats(), ts.eng.flat_params.cpu().numpy().copy()))
    if rank == 1:                                    # one inf in rank 1's gradient scratch, after its backward, before the exchange
        bwd = ts._bwd
        def poisoned(phases):
            bwd(phases)
            ts._scratch[12345] = float("inf")
        ts._bwd = poisoned
    before = ts.eng.flat_params.clone()
    mom = ts.mom.clone()
    ts.step(x, t)
    torch.cuda.synchronize()
    skipped_ok = bool(torch.equal(before, ts.eng.flat_params)) and bool(torch.equal(mom, ts.mom))
    out.append((ts.scaler_stats(), ts.eng.flat_params.cpu().numpy().copy()))
    if rank == 1:
        ts._bwd = bwd
    ts.step(x, t)                                    # clean again
    out.append((ts.scaler_stats(), ts.eng.flat_params.cpu().numpy().copy()))
    q.put((rank, init, out, skipped_ok))
    dist.destroy_process_group()


def test_two_rank_skip_is_collective():
    res = run_ranks(_worker, 2)
    assert res[0][0] == res[1][0] == (1024.0, 0)            # rank 0's scaler state won at construction
    for k, want in enumerate([(1024.0, 0), (512.0, 1), (512.0, 1)]):
        assert res[0][1][k][0] == res[1][1][k][0] == want, (k, res[0][1][k][0], res[1][1][k][0])
        assert np.array_equal(res[0][1][k][1], res[1][1][k][1]), k
    assert res[0][2] and res[1][2]                          # the poisoned step changed no parameter and no momentum on either rank
    assert not np.array_equal(res[0][1][2][1], res[0][1][1][1])   # and the next clean step did
