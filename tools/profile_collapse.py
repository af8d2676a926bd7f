#!/usr/bin/env python3
"""rocprofv3 evidence for `colorid collapse` at the metric's shape (a 256-colour input, m = 50 M, n = 4, k = 31 — tests/test_gpu_subset.py's
full-size input — collapsed into 32 groups of 8 neighbours): the process's phases (COLORID_TIMING) of three runs after a warm one,
k_put_records_grouped's time per upload piece from one kernel trace (no counters in it), and the same file through `subset -a` with all
256 accessions kept, in the same session: the yardstick is stage_records' host-to-device copy, which both commands share.  Run on the
GPU box:

  python3 tools/profile_collapse.py OUT_DIR     # writes OUT_DIR/collapse_summary.md, collapse_kernel_stats.csv, collapse_subset_kernel_stats.csv
"""
import os
import pathlib
import re
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")

from profile_merge import find, kernel_stats, records_region, run   # noqa: E402


def timed_runs(cmd, n):
    """a warm run, then n runs: their wall times and `timing:` lines"""
    env = dict(os.environ, COLORID_TIMING="1")
    run(cmd, env=env)
    walls, phases = [], []
    for _ in range(n):
        p, wall = run(cmd, env=env)
        walls.append(wall)
        phases.append([ln for ln in p.stderr.splitlines() if ln.startswith("timing:")])
    return walls, phases


def phase_ms(phases, what):
    """the milliseconds of the phase whose line starts with `what`, one per run"""
    out = []
    for lines in phases:
        hit = [ln for ln in lines if ln.startswith("timing: " + what)]
        out.append(float(re.search(r"(\d+) ms \(at", hit[0]).group(1)))
    return out


def main():
    out_dir = os.path.abspath(sys.argv[1])
    os.makedirs(out_dir, exist_ok=True)
    from test_gpu_subset import full_size_input
    work = pathlib.Path(tempfile.mkdtemp(prefix="collapse_prof_"))
    try:
        src, _, names, _ = full_size_input(work, np.random.default_rng(41))
        groups = str(work / "groups.tsv")
        with open(groups, "w") as fh:
            fh.write("".join(f"{n}\tgroup_{c // 8:02d}\n" for c, n in enumerate(names)))
        keep = str(work / "keep.txt")
        with open(keep, "w") as fh:
            fh.write("".join(n + "\n" for n in names))
        col_cmd = [BIN, "collapse", "-b", str(work / "col"), "-i", src, "-g", groups]
        sub_cmd = [BIN, "subset", "-b", str(work / "sub"), "-i", src, "-a", keep]
        col_walls, col_phases = timed_runs(col_cmd, 3)
        sub_walls, sub_phases = timed_runs(sub_cmd, 3)
        col_stats = kernel_stats(out_dir, "collapse", col_cmd)
        sub_stats = kernel_stats(out_dir, "collapse_subset", sub_cmd)
        in_rows, in_rec = records_region(src)
        out_rows, out_rec = records_region(str(work / "col.bxi"))
        n_col, t_col = find(col_stats, "k_put_records_grouped")
        n_chk, t_chk = find(col_stats, "k_pairs_check")
        n_sub, t_sub = find(sub_stats, "k_put_records_subset")
        rec_bytes = in_rows * in_rec
        col_stream, sub_stream = phase_ms(col_phases, "records streamed"), phase_ms(sub_phases, "records streamed")
        inside = min(sub_stream) <= min(col_stream) and max(col_stream) <= max(sub_stream)
        extra = sum(col_stream) / 3 - sum(sub_stream) / 3
        lines = [
            "# `colorid collapse` at the metric's shape: 256 colours into 32 groups of 8 neighbours, m = 50 M, n = 4, k = 31",
            "",
            f"input: {in_rows:,} row records of {in_rec} B ({rec_bytes / 1e9:.2f} GB); output: {out_rows:,} records of {out_rec} B",
            "",
            "| kernel | calls (upload pieces) | total ms | ms per piece | GB/s of records read |",
            "|---|---|---|---|---|",
            f"| `k_put_records_grouped` (collapse: rows and both sets of column counts) | {n_col} | {t_col:.2f} | {t_col / n_col:.2f} | {rec_bytes / t_col / 1e6:.0f} |",
            f"| `k_pairs_check` (collapse: the piece's check before it is applied) | {n_chk} | {t_chk:.2f} | {t_chk / n_chk:.2f} | {rec_bytes / t_chk / 1e6:.0f} |",
            f"| `k_put_records_subset` (`subset -a`, all 256 kept, the same file) | {n_sub} | {t_sub:.2f} | {t_sub / n_sub:.2f} | {rec_bytes / t_sub / 1e6:.0f} |",
            "",
            f"\"records streamed\" phase, three runs after a warm one (ms): collapse {col_stream}, subset {sub_stream}",
            "",
            ("collapse's phase lies within the spread of subset's three runs." if inside else
             f"collapse's phase does not lie within the spread of subset's three runs: its mean differs by {extra:+.0f} ms; the kernels' totals "
             f"differ by {t_col + t_chk - t_sub:+.0f} ms (k_put_records_grouped + k_pairs_check against k_put_records_subset, whose check is "
             f"inside it); what remains lies outside the kernels, where collapse adds to subset's piece loop the counters' memset and "
             f"read-back and a second stream synchronisation."),
            "",
            f"process wall, the same runs (s): collapse {', '.join(f'{w:.2f}' for w in col_walls)}; subset {', '.join(f'{w:.2f}' for w in sub_walls)} "
            f"(subset writes all 256 colours back: {in_rec} B records against collapse's {out_rec} B)",
            "",
            "collapse:",
            "```",
            *[ln for run_lines in col_phases for ln in run_lines + ["---"]][:-1],
            "```",
            "subset -a (all 256 kept):",
            "```",
            *[ln for run_lines in sub_phases for ln in run_lines + ["---"]][:-1],
            "```",
        ]
        with open(os.path.join(out_dir, "collapse_summary.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
