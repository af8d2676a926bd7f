#!/usr/bin/env python3
"""Evidence for `read_id --taxon` on 1 M x 150 bp reads with Illumina-style headers and 41 skewed quality letters:

  (a) the compressor alone: tools/exp_deflate.py (HIP events around cid_bgzf_deflate_dev and cid_bgzf_deflate_lz_dev, the members' size,
      zlib level 1 and level 6 over the same 65 280-byte pieces on 16 host threads; the same once more with 4 binned quality letters) and,
      from a run of its own under rocprofv3 --kernel-trace --stats, the time per kernel;
  (b) the command line: an index of 16 random 1 Mb genomes (m = 5 M, n = 4, k = 31), the reads drawn from them with 1 % errors and
      written as block gzip; `read_id` without the flags, `read_id --taxon genomeA` (8 of the 16 genomes: about half the reads kept), the
      same with `--gz-matches` and
      the same three commands from PARENT_BIN (the parent commit's binary), alternating, REPS (EXP_REPS, default 3) times each after one
      warm-up: the whole-process wall clock, the classification phase and the `timing: --taxon:` line (COLORID_TIMING), whether either
      binary's .fq.gz files are the same bytes, then one traced --taxon run of either binary for the filter step's kernels.

Run on the GPU box:   python3 tools/profile_filter.py OUT_DIR [PARENT_BIN [cli]]      (cli: section (b) alone)
writes OUT_DIR/filter_summary.md, filter_deflate.json, filter_deflate_kernel_stats.csv, filter_cli_kernel_stats.csv,
filter_cli_parent_kernel_stats.csv"""
import json
import os
import pathlib
import re
import shutil
import struct
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
REPS = int(os.environ.get("EXP_REPS", 3))
G, LG, R = 16, 1_000_000, int(os.environ.get("EXP_READS", 1_000_000))

from profile_merge import kernel_stats, run   # noqa: E402


def make_sample(work):
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genomes = []
    with open(work / "refs.tsv", "w") as tsv:
        for g in range(G):
            s = acgt[rng.integers(0, 4, LG)]
            genomes.append(s)
            body = s.tobytes()
            (work / f"g{g:02d}.fasta").write_bytes(f">g{g}\n".encode() + b"\n".join(body[i:i + 80] for i in range(0, LG, 80)) + b"\n")
            tsv.write(f"genome{'A' if g < G // 2 else 'B'}{g:02d}\t{work}/g{g:02d}.fasta\n")
    src, pos = rng.integers(0, G, R), rng.integers(0, LG - 150, R)
    reads = np.stack([genomes[src[i]][pos[i]:pos[i] + 150] for i in range(R)])
    err = rng.random(reads.shape) < 0.01
    reads[err] = acgt[rng.integers(0, 4, int(err.sum()))]
    p = np.linspace(1, 8, 41)
    qual = rng.choice(np.arange(33, 74, dtype=np.uint8), size=(R, 150), p=p / p.sum())
    text = b"".join(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n" % (1101 + i // 5000, 1000 + (i * 37) % 30000, 1000 + (i * 101) % 30000) +
                    reads[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n" for i in range(R))
    with open(work / "reads.fastq.gz", "wb") as f:
        for i in range(0, len(text), 65280):
            c = text[i:i + 65280]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = co.compress(c) + co.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(body) + 8 - 1))
            f.write(body + struct.pack("<II", zlib.crc32(c) & 0xFFFFFFFF, len(c)))
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    run([BIN, "build", "-s", "5000000", "-n", "4", "-k", "31", "-b", str(work / "idx"), "-r", str(work / "refs.tsv")])
    return len(text)


def phases(stderr):
    return [ln.split("\r")[-1] for ln in stderr.splitlines() if "timing:" in ln or "Wrote " in ln]


def classification_ms(stderr):
    for name, ms in re.findall(r"timing: ([A-Za-z_ ,]+?) (\d+) ms", stderr.replace("\r", "\n")):
        if "lassif" in name:
            return int(ms)
    return None


def rng_of(xs, unit, fmt="{:.2f}"):
    xs = [x for x in xs if x is not None]
    return (fmt.format(min(xs)) + "–" + fmt.format(max(xs)) + " " + unit + " (" + ", ".join(fmt.format(x) for x in xs) + ")") if xs else "n/a"


def taxon_line_ms(stderr):
    m = re.search(r"timing: --taxon: (\d+) ms", stderr)
    return int(m.group(1)) if m else None


# every kernel the filter step launches, either binary's: the copy, the coder, the gather and the scans that size and lay them out
FILTER_STEP_KERNELS = ("k_bgzf_deflate", "k_bgzf_gather", "k_bgzf_piece", "k_bgzf_seg", "k_fq_filter", "k_fq_split",
                       "FqKeepIn", "FqOrderIn", "DefLenIn", "DefSegRoomIn", "DefSegPiecesIn")


def compressor_alone(out_dir, lines):
    exp = [sys.executable, os.path.join(ROOT, "tools", "exp_deflate.py")]
    p, _ = run(exp, env=dict(os.environ, EXP_READS=str(R)), limit=900)
    djs = [json.loads(ln) for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    with open(os.path.join(out_dir, "filter_deflate.json"), "w") as fh:
        for dj in djs:
            print(json.dumps(dj), file=sys.stderr, flush=True)
            fh.write(json.dumps(dj) + "\n")
    os.environ["EXP_READS"] = str(R)
    stats = kernel_stats(out_dir, "filter_deflate", exp)
    lines += ["## (a) the compressor on the reads' text: literals only, with matches, zlib level 1 and level 6", ""]
    for dj in djs:
        lines += [f"Qualities: {dj['qualities']}; text {dj['text_MB']} MB in {dj['members']} members; HIP events around the call, text and members resident.", "",
                  "| coder | time | output | ratio |", "|---|---|---|---|"]
        for key, label in (("literals", "`cid_bgzf_deflate_dev` (literals only)"), ("matches", "`cid_bgzf_deflate_lz_dev` (LZ77 matches)")):
            later = dj[f"{key}_ms_later"]
            lines.append(f"| {label} | first call {dj[f'{key}_ms_first']} ms, then {min(later)}–{max(later)} ms "
                         f"({dj['text_MB'] / 1e3 / (min(later) / 1e3):.0f} GB/s of text at the best) | {dj[f'{key}_out_MB']} MB | {dj[f'{key}_ratio']} x |")
        for level in (1, 6):
            lines.append(f"| zlib level {level}, {dj[f'zlib{level}_threads']} host threads | {dj[f'zlib{level}_ms']} ms | {dj[f'zlib{level}_out_MB']} MB | "
                         f"{dj[f'zlib{level}_ratio']} x |")
        lines += ["", f"The matches achieve {100 * dj['share_of_zlib1_saving']:.0f} % of zlib level 1's saving over the literal-only members and "
                      f"{100 * dj['share_of_zlib6_saving']:.0f} % of level 6's.", ""]
    lines += ["Per kernel (one `rocprofv3 --kernel-trace --stats` run of the same script: six calls of either coder per text):", "",
              "| kernel | calls | total ms | ms per call |", "|---|---|---|---|"]
    for name, r in stats.items():
        if any(k in name for k in ("k_bgzf_deflate", "k_bgzf_gather", "scan")):
            n, t = int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6
            lines.append(f"| `{name.split('(')[0][-60:]}` | {n} | {t:.2f} | {t / n:.3f} |")


def main():
    out_dir = os.path.abspath(sys.argv[1])
    parent_bin = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] else None
    os.makedirs(out_dir, exist_ok=True)
    lines = [f"# `read_id --taxon`: the device compressor and the fused filter, {R:,} x 150 bp reads", ""]
    if sys.argv[3:] != ["cli"]:
        compressor_alone(out_dir, lines)
    # ---- (b) the command line
    work = pathlib.Path(tempfile.mkdtemp(prefix="filter_prof_"))
    try:
        text_bytes = make_sample(work)
        print("sample and index made", file=sys.stderr, flush=True)
        env = dict(os.environ, COLORID_TIMING="1")
        q = ["-b", str(work / "idx.bxi"), "-q", str(work / "reads.fastq.gz")]
        cmds = {"plain": [BIN, "read_id", *q, "-n", str(work / "plain")],
                "taxon": [BIN, "read_id", *q, "-n", str(work / "taxon"), "--taxon", "genomeA"],
                "taxon_lz": [BIN, "read_id", *q, "-n", str(work / "taxon_lz"), "--taxon", "genomeA", "--gz-matches"]}
        if parent_bin:                                           # (the parent's --taxon runs follow this commit's directly: alternating)
            cmds["parent"] = [parent_bin, "read_id", *q, "-n", str(work / "parent")]
            cmds["parent_taxon"] = [parent_bin, *cmds["taxon"][1:-3], str(work / "ptaxon"), "--taxon", "genomeA"]
            cmds["parent_taxon_lz"] = [*cmds["parent_taxon"][:-3], str(work / "ptaxon_lz"), "--taxon", "genomeA", "--gz-matches"]
        run(cmds["plain"], env=env)                              # a warm-up nobody counts: index and reads come into the page cache
        walls, cls, flt, first = {k: [] for k in cmds}, {k: [] for k in cmds}, {k: [] for k in cmds}, {}
        for rep in range(REPS):                                  # alternating, so a drift of the box hits them alike
            for tag, cmd in cmds.items():
                p, wall = run(cmd, env=env)
                walls[tag].append(wall)
                print(f"{tag}: {wall:.2f} s", file=sys.stderr, flush=True)
                cls[tag].append(classification_ms(p.stderr))
                flt[tag].append(taxon_line_ms(p.stderr))
                first.setdefault(tag, phases(p.stderr))
        same = all(open(work / f"taxon_{s}.txt", "rb").read() == open(work / f"plain_{s}.txt", "rb").read() for s in ("reads", "counts"))
        out_gz = os.path.getsize(work / "taxon_genomeA.fq.gz")
        out_gz_lz = os.path.getsize(work / "taxon_lz_genomeA.fq.gz")
        if parent_bin:
            same_files = all(open(work / f"taxon{s}_genomeA.fq.gz", "rb").read() == open(work / f"ptaxon{s}_genomeA.fq.gz", "rb").read() for s in ("", "_lz"))
        traced = {"taxon": kernel_stats(out_dir, "filter_cli", cmds["taxon"])}
        if parent_bin:
            traced["parent_taxon"] = kernel_stats(out_dir, "filter_cli_parent", cmds["parent_taxon"])
        label = {"plain": "`read_id`", "taxon": "`read_id --taxon genomeA`", "taxon_lz": "`read_id --taxon genomeA --gz-matches`",
                 "parent": "`read_id`, the parent commit's binary", "parent_taxon": "`read_id --taxon genomeA`, the parent commit's binary",
                 "parent_taxon_lz": "`read_id --taxon genomeA --gz-matches`, the parent commit's binary"}
        lines += ["", "## (b) the command line", "",
                  f"index: {G} genomes of {LG:,} bases, m = 5 M, n = 4, k = 31; reads: {text_bytes / 1e6:.1f} MB of FASTQ text as block gzip "
                  f"({os.path.getsize(work / 'reads.fastq.gz') / 1e6:.1f} MB); `--taxon genomeA` names {G // 2} of the {G} accessions; its output: "
                  f"{out_gz / 1e6:.1f} MB, with `--gz-matches` {out_gz_lz / 1e6:.1f} MB; `_reads.txt` and `_counts.txt` equal to the run without the flags: {same}", "",
                  f"| command | process wall, {REPS} alternating runs | classification phase (COLORID_TIMING) | its `timing: --taxon:` line, median |",
                  "|---|---|---|---|"]
        for tag in cmds:
            ms = sorted(x for x in flt[tag] if x is not None)
            lines.append(f"| {label[tag]} | {rng_of(walls[tag], 's')} | {rng_of(cls[tag], 'ms', '{:.0f}')} | "
                         f"{rng_of(flt[tag], 'ms', '{:.0f}')}, {ms[len(ms) // 2] if ms else '—'} |")
        if parent_bin:
            lines += ["", f"`.fq.gz` outputs of this commit equal to the parent's byte for byte, both coders: {same_files}"]
        for tag, stats in traced.items():
            lines += ["", f"Kernels of the filter step, one traced run of {label[tag]}:", "", "| kernel | calls | total ms |", "|---|---|---|"]
            rows = [(name, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6) for name, r in stats.items() if any(k in name for k in FILTER_STEP_KERNELS)]
            lines += [f"| `{name.split('(')[0][-70:]}` | {calls} | {ms:.2f} |" for name, calls, ms in rows]
            lines.append(f"| all of them | {sum(r[1] for r in rows)} | {sum(r[2] for r in rows):.2f} |")
        for tag in cmds:
            lines += ["", f"{label[tag]}, first counted run:", "", "```", *first[tag], "```"]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(os.path.join(out_dir, "filter_summary.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
