#!/usr/bin/env python3
"""rocprofv3 evidence for `colorid fold` at the metric's shape (a 256-colour input, m = 50 M, n = 4, k = 31: tests/test_gpu_subset.py's
full-size input): for `fold -f 2` and `fold -f 10` the whole-process wall time over REPS runs (COLORID_TIMING phases of the first), and
from one traced run each (rocprofv3 --kernel-trace --stats, a run of its own) the OR kernel's time per 256 MiB piece and its bytes per
second; beside them `subset -a` keeping every accession of the same file — the existing streaming command with the same input
traffic — from SUBSET_BIN (default: this tree's binary; give the parent commit's for a comparison across trees).  Run on the GPU box:

  python3 tools/profile_fold.py OUT_DIR [SUBSET_BIN]   # writes OUT_DIR/fold_summary.md, fold_f2_kernel_stats.csv, fold_f10_kernel_stats.csv,
                                                       # fold_subset_kernel_stats.csv
"""
import os
import pathlib
import shutil
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
REPS = 5
PIECE = 256 << 20

from profile_merge import find, kernel_stats, records_region, run   # noqa: E402


def spread(xs):
    return f"median {statistics.median(xs):.2f} s, {min(xs):.2f}–{max(xs):.2f} s over {len(xs)} runs"


def main():
    out_dir = os.path.abspath(sys.argv[1])
    subset_bin = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else BIN
    os.makedirs(out_dir, exist_ok=True)
    from test_gpu_subset import full_size_input
    work = pathlib.Path(tempfile.mkdtemp(prefix="fold_prof_"))
    try:
        src, _, names, _ = full_size_input(work, np.random.default_rng(41))
        lst = str(work / "all.txt")
        with open(lst, "w") as fh:
            fh.write("".join(n + "\n" for n in names))
        in_rows, in_rec = records_region(src)
        rec_bytes = in_rows * in_rec
        pieces = -(-rec_bytes // (PIECE // in_rec * in_rec))
        env = dict(os.environ, COLORID_TIMING="1")
        cmds = {"fold_f2": [BIN, "fold", "-b", str(work / "f2"), "-i", src, "-f", "2"],
                "fold_f10": [BIN, "fold", "-b", str(work / "f10"), "-i", src, "-f", "10"],
                "fold_subset": [subset_bin, "subset", "-b", str(work / "sub"), "-i", src, "-a", lst]}
        run(cmds["fold_f2"], env=env)                          # a warm-up nobody counts: the input comes into the page cache
        walls, phases = {k: [] for k in cmds}, {}
        for rep in range(REPS):                                # the three commands alternate, so a drift of the box hits them alike
            for tag, cmd in cmds.items():
                p, wall = run(cmd, env=env)
                walls[tag].append(wall)
                if rep == 0:
                    phases[tag] = [ln for ln in p.stderr.splitlines() if ln.startswith("timing:")]
        stats = {tag: kernel_stats(out_dir, tag, cmd) for tag, cmd in cmds.items()}
        label = {"fold_f2": "fold -f 2", "fold_f10": "fold -f 10", "fold_subset": "subset -a (all 256)"}
        kern = {"fold_f2": "k_put_records_folded", "fold_f10": "k_put_records_folded", "fold_subset": "k_put_records_subset"}
        lines = [
            "# `colorid fold` at the metric's shape: 256 colours, m = 50 M, n = 4, k = 31, folded by 2 and by 10",
            "",
            f"input: {in_rows:,} row records of {in_rec} B ({rec_bytes / 1e9:.2f} GB, {pieces} pieces of at most 256 MiB), rows ascending, "
            "a quarter of the bits set; `subset -a` keeps all 256 accessions of the same file"
            + ("" if subset_bin == BIN else f" and runs from `{os.path.relpath(subset_bin, ROOT)}`"),
            "",
            "| command | wall | kernel | calls | total ms | ms per piece | record bytes per second (GB/s) |",
            "|---|---|---|---|---|---|---|",
        ]
        for tag in cmds:
            n, t = find(stats[tag], kern[tag])
            lines.append(f"| `{label[tag]}` | {spread(walls[tag])} | "
                         f"`{kern[tag]}` | {n} | {t:.2f} | {t / n:.3f} | {rec_bytes / t / 1e6:.0f} |")
            if tag != "fold_subset":
                n_c, t_c = find(stats[tag], "k_pairs_check")
                lines.append(f"| | | `k_pairs_check` (the piece's check, before the OR) | {n_c} | {t_c:.2f} | {t_c / n_c:.3f} | {rec_bytes / t_c / 1e6:.0f} |")
        lines += ["", "Kernel times are from one `rocprofv3 --kernel-trace --stats` run per command, made after the wall-time runs; bytes are the "
                  "record bytes read, counted, not measured with counters.", ""]
        for tag in cmds:
            lines += [f"`{tag}` phases (first run):", "", "```", *phases[tag], "```", ""]
        with open(os.path.join(out_dir, "fold_summary.md"), "w") as fh:
            fh.write("\n".join(lines))
        print("\n".join(lines))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
