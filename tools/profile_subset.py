#!/usr/bin/env python3
"""rocprofv3 evidence for `colorid subset` at the metric's shape (a 256-colour input, m = 50 M, n = 4, k = 31; 128 colours kept,
interleaved; tests/test_gpu_subset.py's full-size input): the process's phases (COLORID_TIMING), the extract kernel's time and bytes/s,
and k_put_records loading the same INPUT file (`search -s`) in the same session for comparison.  Run on the GPU box:

  python3 tools/profile_subset.py OUT_DIR        # writes OUT_DIR/subset_summary.md, subset_kernel_stats.csv, subset_load_kernel_stats.csv
"""
import os
import pathlib
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")

from profile_merge import find, kernel_stats, records_region, run   # noqa: E402


def main():
    out_dir = os.path.abspath(sys.argv[1])
    os.makedirs(out_dir, exist_ok=True)
    from test_gpu_subset import full_size_input
    work = pathlib.Path(tempfile.mkdtemp(prefix="subset_prof_"))
    try:
        src, _, names, kept = full_size_input(work, np.random.default_rng(41))
        lst = str(work / "keep.txt")
        with open(lst, "w") as fh:
            fh.write("".join(names[c] + "\n" for c in kept))
        prefix = str(work / "sub")
        cmd = [BIN, "subset", "-b", prefix, "-i", src, "-a", lst]
        env = dict(os.environ, COLORID_TIMING="1")
        walls, phases = [], []
        for _ in range(2):
            p, wall = run(cmd, env=env)
            walls.append(wall)
            phases.append([ln for ln in p.stderr.splitlines() if ln.startswith("timing:")])
        sub_stats = kernel_stats(out_dir, "subset", cmd)
        query = os.path.join(ROOT, "tests", "golden", "refs", "Listeria_phage_B021.fasta")
        load_stats = kernel_stats(out_dir, "subset_load", [BIN, "search", "-b", src, "-q", query, "-s"])
        in_rows, in_rec = records_region(src)
        out_rows, out_rec = records_region(prefix + ".bxi")
        w_in, w_out = (in_rec - 24) // 4, (out_rec - 24) // 4
        n_sub, t_sub = find(sub_stats, "k_put_records_subset")
        n_put, t_put = find(load_stats, "k_put_records")
        rec_bytes = in_rows * in_rec
        sub_bytes = rec_bytes + in_rows * w_out * 4          # each input record read once + 4 bytes stored per output word
        put_bytes = rec_bytes + in_rows * w_in * 4           # the loader: the same records read + every word stored
        ns_sub, ns_put = t_sub * 1e6 / rec_bytes, t_put * 1e6 / rec_bytes
        share = [t_sub / 1e3 / w for w in walls]
        lines = [
            "# `colorid subset` at the metric's shape: 128 of 256 colours (interleaved), m = 50 M, n = 4, k = 31",
            "",
            f"input: {in_rows:,} row records of {in_rec} B ({rec_bytes / 1e9:.2f} GB); output: {out_rows:,} records of {out_rec} B",
            "",
            "| kernel | calls | total ms | counted bytes | GB/s | ns per record byte |",
            "|---|---|---|---|---|---|",
            f"| `k_put_records_subset` (subset) | {n_sub} | {t_sub:.2f} | {sub_bytes / 1e9:.2f} GB | {sub_bytes / t_sub / 1e6:.0f} | {ns_sub:.4f} |",
            f"| `k_put_records` (`search -s` loading the same input file) | {n_put} | {t_put:.2f} | {put_bytes / 1e9:.2f} GB | "
            f"{put_bytes / t_put / 1e6:.0f} | {ns_put:.4f} |",
            "",
            f"ratio, ns per record byte, extract / loader: {ns_sub / ns_put:.2f}",
            "",
            f"process wall (COLORID_TIMING=1, two runs, input in the page cache): {walls[0]:.2f} s, {walls[1]:.2f} s; "
            f"the extract kernel's share of it (kernel time from the traced run): {100 * share[0]:.1f} %, {100 * share[1]:.1f} %",
            "",
            "```",
            *phases[0], "---", *phases[1],
            "```",
        ]
        with open(os.path.join(out_dir, "subset_summary.md"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
