"""The lane scheduler's list schedule (csrc/sched.hip: hazard_dag + list_schedule, the two pure parts of Sched::run_list) through
its host-only entry nunet_list_schedule_host: on seeded random op lists the issue order is a permutation that keeps every
conflicting pair (read after write, write after write, write after read on some resource id) in program order, every lane is one
of the three, and the result is a function of the input; one case derived by hand from run_list; the refusals. No GPU."""
import ctypes as C
import random

import nunet_amd  # noqa: F401
from nunet_amd import _lib as L

NL = 3            # csrc/sched.hip list_schedule: lanes
NRES = 512        # csrc/sched.h: resource ids
MAX_RD, MAX_WR = 12, 8   # csrc/sched.h Sched::Op


def i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def call(ops, raw=None):
    """ops: [(cost, reads, writes)] -> (rc, order, lane); raw: replaces named arguments"""
    n = len(ops)
    rd_off, rd, wr_off, wr = [0], [], [0], []
    for _, r, w in ops:
        rd += r
        wr += w
        rd_off.append(len(rd))
        wr_off.append(len(wr))
    order, lane = i32([-7] * n), i32([-7] * n)
    a = dict(nops=n, cost=(C.c_float * max(1, n))(*[o[0] for o in ops]), rd_off=i32(rd_off), rd=i32(rd), wr_off=i32(wr_off), wr=i32(wr),
             order=order, lane=lane)
    a.update(raw or {})
    rc = L.lib().nunet_list_schedule_host(a["nops"], a["cost"], a["rd_off"], a["rd"], a["wr_off"], a["wr"], a["order"], a["lane"])
    return rc, [order[q] for q in range(n)], [lane[q] for q in range(n)]


def schedule(ops):
    rc, order, lane = call(ops)
    assert rc == 0, L.lib().nunet_last_error()
    return order, lane


def random_ops(rng):
    ids = rng.sample(range(NRES), 30)
    ops = []
    for _ in range(rng.randint(1, 200)):
        rd = [rng.choice(ids) for _ in range(rng.choice((0, 1, 2, 3, 3, 6, MAX_RD)))]
        wr = [rng.choice(ids) for _ in range(rng.choice((0, 1, 1, 2, 3, MAX_WR)))]
        ops.append((rng.uniform(1.0, 300.0), rd, wr))
    return ops


def test_random_lists_keep_every_hazard_in_program_order():
    rng = random.Random(20240611)
    pairs = 0
    for _ in range(60):
        ops = random_ops(rng)
        n = len(ops)
        order, lane = schedule(ops)
        assert sorted(order) == list(range(n)), "order is not a permutation"
        assert all(0 <= l < NL for l in lane)
        pos = [0] * n
        for q, p in enumerate(order):
            pos[p] = q
        sets = [(set(r), set(w)) for _, r, w in ops]
        for b in range(n):
            rb, wb = sets[b]
            for a in range(b):
                ra, wa = sets[a]
                if wa & rb or wa & wb or ra & wb:      # RAW, WAW, WAR
                    pairs += 1
                    assert pos[a] < pos[b], "ops %d and %d conflict and were reordered" % (a, b)
        assert schedule(ops) == (order, lane), "two calls on one input differ"
    print("list schedule on 60 random op lists: %d conflicting pairs kept in program order" % pairs)
    assert pairs > 0


def test_hand_derived_case():
    # a chain 0 -> 1 -> 2 through r0 and r1, and an independent op 3: derived by hand from Sched::run_list before its split
    order, lane = schedule([(10.0, [], [0]), (10.0, [0], [1]), (10.0, [1], []), (5.0, [], [])])
    assert order == [0, 3, 1, 2]
    assert lane == [0, 0, 0, 1]


def test_empty_list():
    assert call([])[0] == 0


def test_refuses_bad_arguments():
    lib = L.lib()
    ok = [(1.0, [3], [4]), (2.0, [4], [5])]
    assert call(ok)[0] == 0
    for bad in (-1, NRES):
        assert call([(1.0, [bad], [])])[0] == -1 and b"resource" in lib.nunet_last_error()
        assert call([(1.0, [], [bad])])[0] == -1 and b"resource" in lib.nunet_last_error()
    assert call([(1.0, list(range(MAX_RD)), list(range(MAX_WR)))])[0] == 0
    assert call([(1.0, list(range(MAX_RD + 1)), [])])[0] == -1 and b"12 / 8" in lib.nunet_last_error()
    assert call([(1.0, [], list(range(MAX_WR + 1)))])[0] == -1 and b"12 / 8" in lib.nunet_last_error()
    for name in ("cost", "rd_off", "wr_off", "order", "lane", "rd", "wr"):
        assert call(ok, {name: None})[0] == -1 and b"null" in lib.nunet_last_error(), name
    assert call(ok, {"nops": -1})[0] == -1
    assert call(ok, {"rd_off": i32([0, 1, 0])})[0] == -1 and b"monotonic" in lib.nunet_last_error()
    assert call(ok, {"wr_off": i32([1, 0, 2])})[0] == -1 and b"monotonic" in lib.nunet_last_error()
