#!/usr/bin/env python3
"""The tile kernels before and after a change to their shared walk (DESIGN.md §4 "Segmented search", cid_segwalk.hpp): a parent build's
libcolorid_hip.so and this tree's alternate, five rounds, each run a fresh process of
    tools/exp_alleles.py kernels   cid_search_segments_dev and cid_search_perfect_segments_dev on 9.4 M k-mers
    tools/exp_cover.py kernels     k_cover_rows (the call with one empty segment: its k_cover_stats does nothing)
and every run's median of five timed calls is kept.  The bar is the parent's own spread: this tree's median of medians within the min..max
of the parent's five medians.  Run on the GPU box from the repo root:
    SEGWALK_PARENT_LIB=<a parent build's libcolorid_hip.so> python3 tools/exp_segwalk.py > profiles/segwalk_ab.txt"""
import os, re, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.environ["SEGWALK_PARENT_LIB"]
ROUNDS = 5
# (tool, the start of its line, what the line times)
LINES = (("exp_alleles.py", "cid_search_segments_dev", "cid_search_segments_dev (k_search_segments)"),
         ("exp_alleles.py", "cid_search_perfect_segments_dev", "cid_search_perfect_segments_dev (k_perfect_segments)"),
         ("exp_cover.py", "k_cover_rows (+", "cid_search_cover_dev, one empty segment (k_cover_rows)"))


def log(*a):
    print(*a, flush=True)


def main():
    med = {}
    for rnd in range(ROUNDS):      # the libraries alternate: whatever else runs on the box meets both alike
        for tool in ("exp_alleles.py", "exp_cover.py"):
            for who, lib in (("parent", PARENT), ("this tree", None)):
                env = {k: v for k, v in os.environ.items() if k != "COLORID_HIP_LIB"}
                if lib:
                    env["COLORID_HIP_LIB"] = lib
                t = time.time()
                p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "kernels"], capture_output=True, text=True, env=env, timeout=400)
                if p.returncode != 0:      # nothing more is started on the device
                    log("FAILED", tool, who, p.returncode, p.stdout[-1500:], p.stderr[-1500:]); sys.exit(1)
                for tl, start, what in LINES:
                    if tl != tool:
                        continue
                    line = next(l for l in p.stdout.splitlines() if l.startswith(start))
                    med.setdefault((what, who), []).append(float(re.search(r"median ([\d.]+) ms", line).group(1)))
                    log(f"round {rnd}: {who:9s}: {line}")
                checks = [l for l in p.stdout.splitlines() if "==" in l]
                log(f"round {rnd}: {who:9s}: {tool} kernels took {time.time() - t:.0f} s; " + " | ".join(checks))
    ok = True
    for _, _, what in LINES:
        a, b = med[(what, "parent")], med[(what, "this tree")]
        inside = min(a) <= statistics.median(b) <= max(a)
        ok = ok and inside
        log(f"{what}: parent's medians {a} ms, min {min(a)} max {max(a)} median {statistics.median(a)}; this tree's {b} ms, median {statistics.median(b)} "
            f"-> within the parent's min..max: {inside}")
    log("every kernel within the parent's spread:", ok)


if __name__ == "__main__":
    main()
