"""What the multi-process rehearsals share: a free rendezvous port and the spawn-and-collect loop. The worker functions stay
top-level in their own test modules (spawn pickles them by module name)."""
import queue
import socket

import torch.multiprocessing as mp


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker, world, *args, polls=150):
    """Run worker(rank, world, port, *args, q) in `world` spawned processes; every worker puts (rank, *payload) on q. Returns
    {rank: payload} once every rank has answered and left with exit code 0. A worker that died must not hold the GPU box for
    the full timeout: the 2 s polls stop as soon as one has."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(polls):
        try:
            r = q.get(timeout=2)
            res[r[0]] = r[1:]
            if len(res) == world:
                break
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        if len(res) < world and p.exitcode is None:
            p.kill()                        # (a rank waiting in a collective for one that died)
        p.join(60)
    assert len(res) == world, "a rank failed: exit codes %s" % [p.exitcode for p in procs]
    for p in procs:
        assert p.exitcode == 0
    return res
