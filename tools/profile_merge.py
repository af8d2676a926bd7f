#!/usr/bin/env python3
"""rocprofv3 evidence for `colorid merge` at the metric's shape (two 128-colour halves, m = 50 M, n = 4, k = 31, colours interleaved by
name; tests/test_gpu_merge.py's full-size inputs): the process's phases (COLORID_TIMING), the deposit kernel's time and bytes/s, and
k_put_records loading the merged file for comparison.  Run on the GPU box:

  python3 tools/profile_merge.py OUT_DIR        # writes OUT_DIR/merge_summary.md, merge_kernel_stats.csv, load_kernel_stats.csv
"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")


def run(cmd, env=None, limit=600):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=env)
    if p.returncode != 0:
        sys.exit(f"{' '.join(cmd)}: exit {p.returncode}\n{p.stderr[-3000:]}")
    return p, time.perf_counter() - t0


def kernel_stats(out_dir, tag, cmd):
    d = os.path.join(out_dir, tag + "_stats")
    run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd])
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
    shutil.copy(f, os.path.join(out_dir, tag + "_kernel_stats.csv"))
    shutil.rmtree(d)
    with open(os.path.join(out_dir, tag + "_kernel_stats.csv")) as fh:
        return {r["Name"]: r for r in csv.DictReader(fh)}


def records_region(path):
    from test_gpu_merge import header_bytes
    start, n_rows, rec = header_bytes(path)
    return n_rows, rec


def find(stats, name):
    for k, v in stats.items():
        if name + "(" in k or k.endswith(name) or ("::" + name) in k:
            return int(v["Calls"]), float(v["TotalDurationNs"]) / 1e6
    raise KeyError(name)


def main():
    out_dir = os.path.abspath(sys.argv[1])
    os.makedirs(out_dir, exist_ok=True)
    from test_gpu_merge import full_size_inputs
    import pathlib
    work = pathlib.Path(tempfile.mkdtemp(prefix="merge_prof_"))
    try:
        paths, _, _, _ = full_size_inputs(work, np.random.default_rng(31))
        merged_prefix = str(work / "merged")
        cmd = [BIN, "merge", "-b", merged_prefix, "-i", *paths]
        env = dict(os.environ, COLORID_TIMING="1")
        walls, phases = [], []
        for _ in range(2):
            p, wall = run(cmd, env=env)
            walls.append(wall)
            phases.append([ln for ln in p.stderr.splitlines() if ln.startswith("timing:")])
        merge_stats = kernel_stats(out_dir, "merge", cmd)
        query = os.path.join(ROOT, "tests", "golden", "refs", "Listeria_phage_B021.fasta")
        load_stats = kernel_stats(out_dir, "load", [BIN, "search", "-b", merged_prefix + ".bxi", "-q", query, "-s"])
        in_recs = [records_region(pth) for pth in paths]
        out_rows, out_rec = records_region(merged_prefix + ".bxi")
        n_dep, t_dep = find(merge_stats, "k_put_records_mapped")
        n_put, t_put = find(load_stats, "k_put_records")
        rec_bytes_in = sum(n * r for n, r in in_recs)
        words_touched = sum(n for n, _ in in_recs) * 8          # each half's 128 colours reach all 8 output words of a row
        dep_bytes = rec_bytes_in + words_touched * 4 * 2        # records read + output words read and written
        put_bytes = out_rows * out_rec + out_rows * 8 * 4       # records read + words written
        lines = [
            "# `colorid merge` at the metric's shape: two 128-colour halves, m = 50 M, n = 4, k = 31",
            "",
            f"inputs: {in_recs[0][0]:,} + {in_recs[1][0]:,} row records of {in_recs[0][1]} B; merged: {out_rows:,} records of {out_rec} B",
            "",
            "| kernel | calls | total ms | bytes moved | GB/s | ns per record byte |",
            "|---|---|---|---|---|---|",
            f"| `k_put_records_mapped` (merge) | {n_dep} | {t_dep:.2f} | {dep_bytes / 1e9:.2f} GB | {dep_bytes / t_dep / 1e6:.0f} | "
            f"{t_dep * 1e6 / rec_bytes_in:.4f} |",
            f"| `k_put_records` (loading the merged file) | {n_put} | {t_put:.2f} | {put_bytes / 1e9:.2f} GB | {put_bytes / t_put / 1e6:.0f} | "
            f"{t_put * 1e6 / (out_rows * out_rec):.4f} |",
            "",
            f"process wall (COLORID_TIMING=1, two runs, inputs in the page cache): {walls[0]:.2f} s, {walls[1]:.2f} s",
            "",
            "```",
            *phases[0], "---", *phases[1],
            "```",
        ]
        with open(os.path.join(out_dir, "merge_summary.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
