#!/usr/bin/env python3
"""`colorid search --gather` through the whole command line against the run without the flag, and the greedy cover's kernels at the
benchmark's index shape — 256 colours, m = 50 M, n = 4, k = 31 (DESIGN.md §4 "Greedy cover", §5).  The sample: 1 M reads of 150 bases
from a mixture of three indexed genomes (1 Mbp each), 1 % substitutions.  Run on the GPU box from the repo root:
    python3 tools/exp_gather.py cli     > profiles/gather_cli.txt      (GATHER_PARENT_BIN=<a parent build's bin/colorid> alternates with it)
    rocprofv3 --kernel-trace --stats -d DIR -o gather --output-format csv -- python3 tools/exp_gather.py kernels > profiles/gather_kernels.txt
    python3 tools/exp_gather.py rounds DIR/gather_kernel_trace.csv >> profiles/gather_kernels.txt
`cli` prints, per case and repetition, the wall clock and the CLI's phase lines (COLORID_TIMING=1); `kernels` makes the index and the
k-mer set in the process and calls cid_search_gather_set a few times on all of the reads' k-mers, sequencing errors included (no cut-off:
the matrix at its largest); `rounds` reads the profiler's kernel trace and prints each kernel's time in the first and in the median round."""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
W = os.environ.get("GATHER_WORK", "/tmp/cid_gather"); os.makedirs(W, exist_ok=True)
G, LG, READS, RL, K = 256, 1_000_000, 1_000_000, 150, 31
MIX = (10, 100, 200)          # the sample's genomes, half, a third and a sixth of the reads
acgt = np.frombuffer(b"ACGT", np.uint8)


def log(*a):
    print(*a, flush=True)


def sample_reads(genomes, rng):
    """READS x RL bases drawn from the three genomes, 1 % substitutions"""
    which = rng.choice(3, READS, p=[1 / 2, 1 / 3, 1 / 6])
    start = rng.integers(0, LG - RL, READS)
    reads = np.empty((READS, RL), np.uint8)
    for j in range(3):
        sel = np.flatnonzero(which == j)
        reads[sel] = genomes[j][start[sel, None] + np.arange(RL)[None, :]]
    err = rng.random(reads.shape) < 0.01
    reads[err] = acgt[rng.integers(0, 4, int(err.sum()))]
    return reads


def run(label, binary, args, rep):
    t = time.time()
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=dict(os.environ, COLORID_TIMING="1"), timeout=600)
    dt = time.time() - t
    if p.returncode != 0:
        log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
    ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
    extra = [ln for ln in p.stderr.splitlines() if "--gather" in ln]
    log(f"{label} rep {rep}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph) + (" | " + extra[0] if extra else ""))
    return p


def cli():
    import gzip
    rng = np.random.default_rng(5)
    genomes = {}
    with open(f"{W}/refs.tsv", "w") as tsv:
        for g in range(G):
            s = acgt[rng.integers(0, 4, LG)]
            if g in MIX:
                genomes[g] = s
            with open(f"{W}/g{g:03d}.fasta", "wb") as f:
                f.write(f">genome{g}\n".encode() + s.tobytes() + b"\n")
            tsv.write(f"genome{g:03d}\t{W}/g{g:03d}.fasta\n")
    run("build -k 31 -s 50000000 -n 4 (256 x 1 Mbp)", BIN, ["build", "-s", "50000000", "-n", "4", "-k", str(K), "-b", f"{W}/idx", "-r", f"{W}/refs.tsv"], 0)
    reads = sample_reads([genomes[g] for g in MIX], rng)
    qual = b"I" * RL
    with gzip.open(f"{W}/reads.fastq.gz", "wb", compresslevel=1) as f:
        f.write(b"".join(b"@r%d\n" % i + reads[i].tobytes() + b"\n+\n" + qual + b"\n" for i in range(READS)))
    q = ["search", "-b", f"{W}/idx.bxi", "-q", f"{W}/reads.fastq.gz"]
    parent = os.environ.get("GATHER_PARENT_BIN")
    cases = ([("search (parent build)        ", parent, q)] if parent else []) + [("search (this tree)           ", BIN, q),
                                                                                  ("search --gather              ", BIN, q + ["--gather", f"{W}/out"])]
    last = {}
    for rep in range(3):        # the cases alternate, and each rep starts with another one: the first run after a pause is the fastest
        for label, binary, args in cases[rep % len(cases):] + cases[:rep % len(cases)]:
            last[label] = run(label, binary, args, rep)
    a, b, c = last.get(cases[0][0]) if parent else None, last["search (this tree)           "], last["search --gather              "]
    if a:
        log("parent's stdout == this tree's:", a.stdout == b.stdout)
    log("stdout with --gather == without:", c.stdout == b.stdout)
    log(open(f"{W}/out.gather.tsv").read())


def kernels():
    import math
    import torch
    import bench
    import colorid_amd
    from colorid_amd.hip import check
    dev = torch.device("cuda:0")
    ctx = colorid_amd.Context(0)
    m, n = 50_000_000, 4
    hx = colorid_amd.Index(ctx, m, n, K, G)
    ptr, rs = hx.device_matrix()
    p = bench.fill_background_fast(dev, ptr, m, rs, G, 1.0 - math.exp(-n * LG / m), seed=7)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    genomes = [acgt[rng.integers(0, 4, LG)] for _ in MIX]
    for g, s in zip(MIX, genomes):          # the three genomes on top of a background of the other accessions' density
        ks = colorid_amd.KmerSet(ctx, K)
        ks.add_seqs([s.tobytes()])
        ks.finalize()
        check(hx.lib.cid_index_insert_kmerset(hx.h, ks.h, g))
        ks.close()
    hx.finalize()
    reads = sample_reads(genomes, rng)
    ks = colorid_amd.KmerSet(ctx, K)
    ks.add_seqs([r.tobytes() for r in reads])
    nk = ks.finalize()
    log(f"index: {G} colours, m = {m}, n = {n}, k = {K}, background density {p:.4f}, row stride {rs} words; {READS} reads, {nk} distinct k-mers "
        f"(no cut-off), matrix {nk * rs * 8 / 1e9:.2f} GB")
    for min_new in (1000, 1000, 1000, 100_000, 1):       # the last one: every accession, most of them for their chance hits alone
        t = time.time()
        rows, n_hit = ks.search_gather(hx, min_new)
        dt = time.time() - t
        log(f"cid_search_gather_set min_new {min_new}: {len(rows)} rounds, n_hit {n_hit}, wall {dt * 1e3:.1f} ms; first rows "
            f"{[(int(r['colour']), int(r['new_kmers']), int(r['total_kmers'])) for r in rows[:4]]}; last new_kmers {int(rows[-1]['new_kmers']) if len(rows) else 0}")
    ks.close(); hx.close(); ctx.close()


def rounds():
    """per call of the trace (a call begins at its k_cover_rows) and kernel of the cover: launches, total, and the first, the median and the last launch"""
    import csv
    ev = [(int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in csv.DictReader(open(sys.argv[2]))]
    ev.sort()
    names = ("k_cover_rows", "k_gather_init", "k_gather_fold<true>", "k_gather_fold<false>", "k_gather_mark", "k_gather_pick")
    calls, cur = [], None
    for _, name, ms in ev:
        key = next((nm for nm in names if nm.split("<")[0] in name and (("<" not in nm) or nm.split("<")[1].rstrip(">") in name)), None)
        if key is None:
            continue
        if key == "k_cover_rows":
            cur = {nm: [] for nm in names}
            calls.append(cur)
        if cur is not None:
            cur[key].append(ms)
    for i, c in enumerate(calls):
        log(f"call {i}: " + "; ".join(f"{nm} x{len(v)} total {sum(v):.3f} ms" + (f" (first {v[0]:.3f}, median {sorted(v)[len(v) // 2]:.3f}, last {v[-1]:.3f})" if len(v) > 1 else "")
                                       for nm, v in c.items() if v))


if __name__ == "__main__":
    {"cli": cli, "kernels": kernels, "rounds": rounds}[sys.argv[1]]()
