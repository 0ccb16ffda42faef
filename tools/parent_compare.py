"""Shared by the *_overhead tools' --parent DIR mode: the same tool file measures a built checkout of the parent commit and this
one in alternating child processes (child: --tree DIR, the checkout whose package is imported), and every figure is judged by
one rule: the difference of the two medians must lie inside the parent's own spread - maximum minus minimum over all rounds of
all its processes, so round-to-round and process-to-process variation both count."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tree():
    """the checkout a tool imports from: --tree DIR of a child process, else the one the tool sits in"""
    return os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE


def alternate(script, parent, argv, procs, timeout=900):
    """[parent, this] * procs child processes of `script`; returns {'parent': [summary, ...], 'this': [...]}, a summary being the
    JSON object on a child's last output line"""
    out = {"parent": [], "this": []}
    for p in range(procs):
        for name, t in (("parent", os.path.abspath(parent)), ("this", HERE)):
            r = subprocess.run([sys.executable, os.path.abspath(script)] + list(argv) + ["--tree", t], capture_output=True, text=True, timeout=timeout)
            if r.returncode != 0:
                raise SystemExit("child on %s failed (%d):\n%s\n%s" % (t, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d %s done" % (p, name), flush=True)
    return out


def judge(parent_rounds, this_rounds):
    """two lists (one entry per process) of lists of rounds"""
    pa, th = [x for pr in parent_rounds for x in pr], [x for pr in this_rounds for x in pr]
    d = {"parent_by_process": parent_rounds, "this_by_process": this_rounds, "parent_median": statistics.median(pa), "this_median": statistics.median(th),
         "parent_spread": max(pa) - min(pa), "this_spread": max(th) - min(th)}
    d["median_minus_parent"] = d["this_median"] - d["parent_median"]
    d["inside_parent_spread"] = abs(d["median_minus_parent"]) <= d["parent_spread"]
    return d
