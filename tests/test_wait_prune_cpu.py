"""The lane scheduler's wait pruning (csrc/sched.h, WaitPruner) through its host-only entry nunet_wait_prune_host, on seeded
random DAGs: what it keeps is a subset of what was asked, and every requested cross-lane dependency is still enforced by
lane order plus the kept waits. No GPU."""
import ctypes as C
import random

import nunet_amd  # noqa: F401
from nunet_amd import _lib as L


def prune(nlanes, lane, edges):
    """edges[b] = producer ops of op b -> (flat edge list [(a, b)], keep flags)"""
    nops = len(lane)
    off, src = [0], []
    for b in range(nops):
        src += edges[b]
        off.append(len(src))
    keep = (C.c_uint8 * max(1, len(src)))(*([7] * max(1, len(src))))
    rc = L.lib().nunet_wait_prune_host(nlanes, nops, (C.c_int32 * max(1, nops))(*lane), (C.c_int32 * (nops + 1))(*off),
                                       (C.c_int32 * max(1, len(src)))(*src), keep)
    assert rc == 0, L.lib().nunet_last_error()
    flat = [(a, b) for b in range(nops) for a in edges[b]]
    return flat, [int(keep[e]) for e in range(len(flat))]


def ordered_before(nops, lane, flat, keep):
    """reach[b] = bit set of the ops that have ended before op b starts, by lane order and the kept waits alone"""
    kept_in = [[] for _ in range(nops)]
    for (a, b), k in zip(flat, keep):
        if k:
            kept_in[b].append(a)
    last, reach = {}, [0] * nops
    for b in range(nops):
        preds = list(kept_in[b])
        if lane[b] in last:
            preds.append(last[lane[b]])
        for a in preds:
            reach[b] |= reach[a] | (1 << a)
        last[lane[b]] = b
    return reach


def random_dag(rng):
    nops = rng.randint(1, 200)
    nlanes = rng.randint(3, 5)
    lane = [rng.randrange(nlanes) for _ in range(nops)]
    # ops in a topological issue order: producers are earlier ops; some asked for twice, as two resources of one producer are
    edges = []
    for b in range(nops):
        k = min(b, rng.choice((0, 1, 1, 2, 3, 6)))
        e = [rng.randrange(b) for _ in range(k)]
        if e and rng.random() < 0.2:
            e.append(e[0])
        edges.append(e)
    return nlanes, lane, edges


def test_kept_waits_are_a_subset_and_every_requested_edge_stays_ordered():
    rng = random.Random(20240607)
    asked = kept = 0
    for _ in range(200):
        nlanes, lane, edges = random_dag(rng)
        flat, keep = prune(nlanes, lane, edges)
        assert all(k in (0, 1) for k in keep)                      # every flag written, nothing but 0 / 1
        for (a, b), k in zip(flat, keep):
            assert not (k and lane[a] == lane[b]), "a wait on the op's own lane"
        reach = ordered_before(len(lane), lane, flat, keep)
        for a, b in flat:
            assert reach[b] >> a & 1, "op %d no longer waits for op %d (lanes %d, %d)" % (b, a, lane[b], lane[a])
        cross = [(a, b) for a, b in flat if lane[a] != lane[b]]
        asked += len(set(cross))
        kept += sum(keep)
    print("wait pruning on 200 random DAGs: %d distinct cross-lane waits asked, %d kept" % (asked, kept))
    assert kept < asked


def test_one_lane_keeps_no_wait():
    nops = 50
    for lane_id in (0, 3):
        lane = [lane_id] * nops
        edges = [[] if b == 0 else [b - 1] + ([0] if b > 1 else []) for b in range(nops)]
        flat, keep = prune(4, lane, edges)
        assert flat and sum(keep) == 0


def test_known_cases():
    # A (lane 0) -> B (lane 1) -> C (lane 2), and C also asks for A: implied through B
    flat, keep = prune(3, [0, 1, 2], [[], [0], [1, 0]])
    assert dict(zip(flat, keep)) == {(0, 1): 1, (1, 2): 1, (0, 2): 0}
    # ... whatever the order C names them in
    flat, keep = prune(3, [0, 1, 2], [[], [0], [0, 1]])
    assert dict(zip(flat, keep)) == {(0, 1): 1, (1, 2): 1, (0, 2): 0}
    # a later op of the producer lane was already waited for: the earlier one is implied
    flat, keep = prune(2, [0, 0, 1, 1], [[], [], [1], [0]])
    assert keep == [1, 0]
    # the same producer asked for twice: waited for once
    flat, keep = prune(2, [0, 1], [[], [0, 0]])
    assert keep == [1, 0]
    # independent producers on two lanes: both waits stay
    flat, keep = prune(3, [0, 1, 2], [[], [], [0, 1]])
    assert keep == [1, 1]


def test_refuses_bad_arguments():
    lib = L.lib()
    one = (C.c_int32 * 1)(0)
    off = (C.c_int32 * 2)(0, 0)
    keep = (C.c_uint8 * 1)(0)
    assert lib.nunet_wait_prune_host(17, 1, one, off, one, keep) == -1
    assert lib.nunet_wait_prune_host(2, 1, (C.c_int32 * 1)(2), off, one, keep) == -1            # lane out of range
    assert lib.nunet_wait_prune_host(2, 1, one, (C.c_int32 * 2)(0, 1), one, keep) == -1         # an op waiting for itself
