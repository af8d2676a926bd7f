#!/usr/bin/env python3
"""rocprofv3 evidence for `colorid compare` at the metric's shape (a 256-colour input, m = 50 M, n = 4, k = 31, a fifth of the rows zero:
tests/test_gpu_subset.py's full-size input): k_pairs' time per upload chunk and in total from one `--kernel-trace --stats` run (no
counters in it), the process's phases (COLORID_TIMING=1; one warm run, then three), and for orientation `colorid subset`'s phase
"records streamed and extracted" on the same file in the same session — both stream the same bytes through the same chunks.
Run on the GPU box:

  python3 tools/profile_compare.py OUT_DIR        # writes OUT_DIR/compare_fullsize.txt and compare_kernel_stats.csv
"""
import csv
import glob
import os
import pathlib
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")

from profile_merge import records_region, run   # noqa: E402

REPS = 3


def timed(cmd, what):
    """one warm run, then REPS: the `timing:` lines of each and the milliseconds of the phase `what`"""
    env = dict(os.environ, COLORID_TIMING="1")
    run(cmd, env=env)
    lines, ms, walls = [], [], []
    for _ in range(REPS):
        p, wall = run(cmd, env=env)
        t = [ln for ln in p.stderr.splitlines() if ln.startswith("timing:")]
        lines.append(t)
        ms.append(next(float(ln.split(what)[1].split()[0]) for ln in t if what in ln))
        walls.append(wall)
        print(f"{cmd[1]}: {what} {ms[-1]:.0f} ms, wall {wall:.2f} s", flush=True)
    return lines, ms, walls


def base_name(kernel):
    return kernel.split("(")[0].split("::")[-1].split()[-1].removesuffix(".kd")


def find(stats, name):
    for k, v in stats.items():
        if base_name(k) == name:
            return int(v["Calls"]), float(v["TotalDurationNs"]) / 1e6
    raise KeyError(name)


def traced(out_dir, cmd):
    """one rocprofv3 --kernel-trace --stats run: ({kernel: stats row}, {kernel: [ms per launch, in launch order]})"""
    d = os.path.join(out_dir, "compare_trace")
    run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd])
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
    shutil.copy(f, os.path.join(out_dir, "compare_kernel_stats.csv"))
    with open(f) as fh:
        stats = {r["Name"]: r for r in csv.DictReader(fh)}
    per = {}
    with open(sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        per.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    shutil.rmtree(d)
    return stats, per


def main():
    out_dir = os.path.abspath(sys.argv[1])
    os.makedirs(out_dir, exist_ok=True)
    from test_gpu_subset import full_size_input
    work = pathlib.Path(tempfile.mkdtemp(prefix="compare_prof_"))
    try:
        src, _, names, kept = full_size_input(work, np.random.default_rng(41))
        print("input written", flush=True)
        lst = str(work / "keep.txt")
        with open(lst, "w") as fh:
            fh.write("".join(names[c] + "\n" for c in kept))
        cmp_cmd = [BIN, "compare", "-i", src, "-o", str(work / "cmp")]
        sub_cmd = [BIN, "subset", "-b", str(work / "sub"), "-i", src, "-a", lst]
        cmp_lines, cmp_ms, cmp_walls = timed(cmp_cmd, "records streamed and counted")
        sub_lines, sub_ms, sub_walls = timed(sub_cmd, "records streamed and extracted")
        stats, per = traced(out_dir, cmp_cmd)
        n_rows, rec = records_region(src)
        n_k, t_k = find(stats, "k_pairs")
        n_c, t_c = find(stats, "k_pairs_check")
        chunks = next(v for k, v in per.items() if base_name(k) == "k_pairs")
        rec_bytes = n_rows * rec
        tiles = (n_rows + 63) // 64
        lines = [
            "colorid compare at the metric's shape: 256 colours, m = 50 M, n = 4, k = 31, a fifth of the rows zero",
            "",
            f"input: {n_rows:,} row records of {rec} B ({rec_bytes / 1e9:.2f} GB), {tiles:,} tiles of 64 rows x 10 block pairs",
            "",
            "one rocprofv3 --kernel-trace --stats run (no counters):",
            f"  k_pairs        {n_k} launches (one per upload chunk), {t_k:.3f} ms in total; per chunk, in launch order: "
            + ", ".join(f"{c:.3f}" for c in chunks) + " ms",
            f"                 = {t_k * 1e6 / (tiles * 10):.1f} ns per (tile, block pair) over the whole chip; the records read once: {rec_bytes / t_k / 1e6:.0f} GB/s",
            f"  k_pairs_check  {n_c} launches, {t_c:.3f} ms in total",
            "",
            f"phase \"records streamed and counted\" of compare, {REPS} runs after a warm one (input in the page cache): "
            f"{min(cmp_ms):.0f}-{max(cmp_ms):.0f} ms; process wall {min(cmp_walls):.2f}-{max(cmp_walls):.2f} s",
            f"phase \"records streamed and extracted\" of subset (128 of the 256 colours) on the same file, same session, {REPS} runs after a warm one: "
            f"{min(sub_ms):.0f}-{max(sub_ms):.0f} ms; process wall {min(sub_walls):.2f}-{max(sub_walls):.2f} s",
            f"k_pairs' share of compare's streaming phase: {100 * t_k / max(cmp_ms):.1f}-{100 * t_k / min(cmp_ms):.1f} %",
            "",
            "compare, COLORID_TIMING=1:",
            *[ln for run_lines in cmp_lines for ln in run_lines + ["---"]],
            "subset, COLORID_TIMING=1:",
            *[ln for run_lines in sub_lines for ln in run_lines + ["---"]],
        ]
        with open(os.path.join(out_dir, "compare_fullsize.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
