#!/usr/bin/env python3
"""Evidence for `read_id --split` on tools/profile_filter.py's sample — 1 M x 150 bp reads with Illumina-style headers as
block gzip — and an index of 256 random genomes of 62 500 bases (m = 5 M, n = 4, k = 31), the reads drawn from them with 1 % errors
and classified with -Q 0 (no quality masking: nearly every read then carries one accession's label):

  (a) COLORID_TIMING's `--split` line (cid_fastq_split + writing, 256 + 4 bins) against PARENT_BIN's `--taxon genome` line (a substring
      of every accession: nearly all reads kept, the same text volume through the same coder into ONE file);
  (b) the whole-process wall clock of `--split` against PARENT_BIN's `read_id` without any filter;
  REPS runs each, alternating, after one warm-up; then one traced run of either command of (a) for the kernels behind the two lines, and
  the number of bins, members and short members, the host counting sort's share (CID_FASTQ_TIMING) and the outputs' sizes.

Run on the GPU box:   python3 tools/profile_split.py OUT_DIR PARENT_BIN
writes OUT_DIR/split_summary.md, split_kernel_stats.csv, split_parent_taxon_kernel_stats.csv"""
import glob
import os
import pathlib
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
REPS = int(os.environ.get("EXP_REPS", 3))

import profile_filter as pf   # noqa: E402
from profile_merge import kernel_stats, run   # noqa: E402

pf.G, pf.LG = 256, 62_500


def line_ms(stderr, flag):
    m = re.search(r"timing: %s: (\d+) ms" % flag, stderr)
    return int(m.group(1)) if m else None


def main():
    out_dir, parent_bin = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    os.makedirs(out_dir, exist_ok=True)
    work = pathlib.Path(tempfile.mkdtemp(prefix="split_prof_"))
    lines = [f"# `read_id --split`: every label's reads to a file of its own, {pf.R:,} x 150 bp reads, {pf.G} colours", ""]
    try:
        text_bytes = pf.make_sample(work)
        print("sample and index made", file=sys.stderr, flush=True)
        env = dict(os.environ, COLORID_TIMING="1", CID_FASTQ_TIMING="1")
        # -Q 0: at the default -Q 15 a fifth of this sample's bases are masked, hardly a 31-mer is left whole and 96 % of the reads are no_hits
        q = ["-b", str(work / "idx.bxi"), "-q", str(work / "reads.fastq.gz"), "-Q", "0"]
        cmds = {"split": [BIN, "read_id", *q, "-n", str(work / "split"), "--split"],
                "parent_taxon": [parent_bin, "read_id", *q, "-n", str(work / "ptaxon"), "--taxon", "genome"],
                "taxon": [BIN, "read_id", *q, "-n", str(work / "taxon"), "--taxon", "genome"],
                "parent_plain": [parent_bin, "read_id", *q, "-n", str(work / "pplain")]}
        flag = {"split": "--split", "parent_taxon": "--taxon", "taxon": "--taxon", "parent_plain": None}
        run(cmds["parent_plain"], env=env)                       # a warm-up nobody counts: index and reads come into the page cache
        walls, part, first = {k: [] for k in cmds}, {k: [] for k in cmds}, {}
        for rep in range(REPS):                                  # alternating, so a drift of the box hits them alike
            for tag, cmd in cmds.items():
                p, wall = run(cmd, env=env)
                walls[tag].append(wall)
                part[tag].append(line_ms(p.stderr, flag[tag]) if flag[tag] else None)
                print(f"{tag}: {wall:.2f} s, its line {part[tag][-1]} ms", file=sys.stderr, flush=True)
                first.setdefault(tag, [ln.split("\r")[-1].replace(str(work) + "/", "WORK/") for ln in p.stderr.splitlines()
                                       if "timing:" in ln or "Wrote " in ln or "cid_fastq" in ln])
        same = all(open(work / f"split_{s}.txt", "rb").read() == open(work / f"pplain_{s}.txt", "rb").read() for s in ("reads", "counts"))
        files = glob.glob(str(work / "split_*.fq.gz"))
        split_bytes, one_bytes = sum(os.path.getsize(f) for f in files), os.path.getsize(work / "ptaxon_genome.fq.gz")
        manifest = [ln.split("\t") for ln in open(work / "split_split.tsv").read().splitlines()]
        split_line = next(ln for ln in first["split"] if "timing: --split" in ln)
        members, short = (int(x) for x in re.search(r"(\d+) members \((\d+) of them", split_line).groups())
        split_parts = re.search(r"creating the files (\d+) ms and writing to them (\d+) ms", split_line).groups()
        kept = int(re.search(r"Wrote (\d+) read-pairs", "\n".join(first["parent_taxon"])).group(1))
        sort_ms = float(re.search(r"counting sort\) ([\d.]+)", "\n".join(first["split"])).group(1))
        steps = int(re.search(r"cid_fastq: (\d+) steps", "\n".join(first["split"])).group(1))
        stats = kernel_stats(out_dir, "split", cmds["split"])
        pstats = kernel_stats(out_dir, "split_parent_taxon", cmds["parent_taxon"])
        label = {"split": "`read_id --split`", "parent_taxon": "`read_id --taxon genome`, the parent commit's binary",
                 "taxon": "`read_id --taxon genome`, this commit", "parent_plain": "`read_id`, the parent commit's binary"}
        lines += [f"index: {pf.G} genomes of {pf.LG:,} bases, m = 5 M, n = 4, k = 31; `-Q 0`; reads: {text_bytes / 1e6:.1f} MB of FASTQ text as block gzip "
                  f"({os.path.getsize(work / 'reads.fastq.gz') / 1e6:.1f} MB), classified in {steps} steps; `_reads.txt` and `_counts.txt` of `--split` equal "
                  f"to the parent's run without a filter: {same}", "",
                  f"`--split`: {pf.G + 4} bins, {len(manifest)} of them non-empty ({sum(int(m[1]) for m in manifest):,} reads in the manifest), {len(files)} files, "
                  f"{members:,} members, {short:,} of them the last of a bin in its step (short: under 65 280 bytes of text — the price of cutting per bin per step); "
                  f"output {split_bytes / 1e6:.1f} MB against {one_bytes / 1e6:.1f} MB for the single file of `--taxon genome` "
                  f"({100.0 * (split_bytes - one_bytes) / one_bytes:+.1f} %).", "",
                  f"Per read: {split_bytes / sum(int(m[1]) for m in manifest):.1f} bytes in the {len(files)} files, {one_bytes / kept:.1f} in the single file "
                  f"({kept:,} reads carry an accession's label, which `--taxon genome` keeps).", "",
                  f"Where the `--split` line's time goes, by the line itself (first counted run): creating the files {split_parts[0]} ms, writing to them "
                  f"{split_parts[1]} ms; the parts of `cid_fastq_split` are in the `cid_fastq:` line below.", "",
                  f"Host counting sort inside `cid_fastq_split` (CID_FASTQ_TIMING, first counted run): {sort_ms:.1f} ms of the line's {part['split'][0]} ms.", "",
                  f"| command | (a) its COLORID_TIMING line: the call + writing, {REPS} alternating runs | (b) process wall |", "|---|---|---|"]
        for tag in cmds:
            xs = part[tag]
            lines.append(f"| {label[tag]} | {pf.rng_of(xs, 'ms', '{:.0f}') if flag[tag] else '—'} | {pf.rng_of(walls[tag], 's')} |")
        for title, st in (("`--split`", stats), ("the parent's `--taxon genome`", pstats)):
            lines += ["", f"Kernels behind the line, one traced run of {title} (`rocprofv3 --kernel-trace --stats`, on its own):", "",
                      "| kernel | calls | total ms |", "|---|---|---|"]
            for name, r in st.items():
                if any(k in name for k in ("k_bgzf_deflate", "k_bgzf_gather", "k_bgzf_piece", "k_bgzf_seg", "k_fq_filter", "k_fq_split")):
                    lines.append(f"| `{name.split('(')[0][-70:]}` | {int(r['Calls'])} | {float(r['TotalDurationNs']) / 1e6:.2f} |")
        for tag in cmds:
            lines += ["", f"{label[tag]}, first counted run:", "", "```", *first[tag], "```"]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(os.path.join(out_dir, "split_summary.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
