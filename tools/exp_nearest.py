#!/usr/bin/env python3
"""`colorid search -s -m --alleles --nearest` on the scheme-sized input of tools/exp_alleles.py (20 000 records x 500 bp, 256 colours,
m = 50 M, n = 4, k = 31): what the flag costs when it is off and when it is on, and k_nearest_groups beside k_search_segments and
k_perfect_segments on the same k-mers and offsets (DESIGN.md §4 "Nearest allele per locus", profiles/nearest_summary.md).
Run on the GPU box from the repo root:
    python3 tools/exp_nearest.py cli     > profiles/nearest_cli.txt      (NEAREST_PARENT_BIN=<a parent build's bin/colorid> adds its --alleles)
    python3 tools/exp_nearest.py kernels > profiles/nearest_kernels.txt  (under rocprofv3 --kernel-trace --stats for the kernel times)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exp_alleles as ea
from exp_alleles import BIN, G, K, RECORDS, RL, W, log, run


def cli():
    genomes = ea.genomes_of_one_species(G)
    with open(f"{W}/refs.tsv", "w") as tsv:
        for g, s in enumerate(genomes):
            with open(f"{W}/g{g:03d}.fasta", "wb") as f:
                f.write(f">genome{g}\n".encode() + s.tobytes() + b"\n")
            tsv.write(f"genome{g:03d}\t{W}/g{g:03d}.fasta\n")
    run("build -k 31 -s 50000000 -n 4 (256 x 1 Mbp)", BIN, ["build", "-s", "50000000", "-n", "4", "-k", str(K), "-b", f"{W}/idx", "-r", f"{W}/refs.tsv"], reps=1)
    with open(f"{W}/scheme.fasta", "wb") as f:
        for label, s in ea.scheme(genomes):
            f.write(b">" + label.encode() + b"\n" + s.tobytes() + b"\n")
    q = ["search", "-b", f"{W}/idx.bxi", "-q", f"{W}/scheme.fasta", "-s", "-m"]
    parent = os.environ.get("NEAREST_PARENT_BIN")
    a = b = c = None
    for rnd in range(3):      # the three cases alternate: whatever else runs on the host meets all of them alike
        if parent:
            a = run(f"round {rnd}: -s -m --alleles (parent build)                ", parent, q + ["--alleles", f"{W}/p"], reps=1)
        b = run(f"round {rnd}: -s -m --alleles (this tree)                   ", BIN, q + ["--alleles", f"{W}/t"], reps=1)
        c = run(f"round {rnd}: -s -m --alleles --nearest -p 0.9 (this tree)  ", BIN, q + ["--alleles", f"{W}/n", "--nearest", "-p", "0.9"], reps=1)
    if a:
        log("parent's stdout == this tree's:", a.stdout == b.stdout, "; tables the same files:",
            all(open(f"{W}/p.{e}").read() == open(f"{W}/t.{e}").read() for e in ("raw.tsv", "detailed.tsv", "report.out")))
    log("stdout with --nearest == without:", c.stdout == b.stdout, "; tables the same files:",
        all(open(f"{W}/n.{e}").read() == open(f"{W}/t.{e}").read() for e in ("raw.tsv", "detailed.tsv", "report.out")))
    log("\n".join(l for l in c.stderr.splitlines() if l.startswith("alleles:") or l.startswith("timing: -s -m")))
    shares = np.array([float(l.split("\t")[5]) for l in open(f"{W}/n.nearest.tsv").read().splitlines()[1:]])
    log(f"nearest.tsv: {len(shares)} lines, shares {shares.min():.3f} .. {shares.max():.3f}" if len(shares) else "nearest.tsv: no lines")


def kernels():
    import math
    import torch
    import bench
    import colorid_amd
    dev = torch.device("cuda:0")
    ctx = colorid_amd.Context(0)
    m, n = 50_000_000, 4
    hx = colorid_amd.Index(ctx, m, n, K, G)
    ptr, rs = hx.device_matrix()
    bench.fill_background_fast(dev, ptr, m, rs, G, 1.0 - math.exp(-n * ea.LG / m), seed=7)
    torch.cuda.synchronize()
    recs = [s for _, s in ea.scheme(ea.genomes_of_one_species(8))]
    wins = np.concatenate([np.lib.stride_tricks.sliding_window_view(s, K) for s in recs])
    nw, per = len(wins), RL - K + 1
    dk = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1)).to(dev)
    do = torch.from_numpy(np.arange(RECORDS + 1, dtype=np.int64) * per).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    for _ in range(G):       # the one-species planting of exp_alleles.py kernels
        colour = torch.randint(0, G, (nw,), device=dev, dtype=torch.int32, generator=gen)
        torch.cuda.synchronize()
        hx.insert_kmers_dev(dk.data_ptr(), colour.data_ptr(), nw)
        ctx.synchronize()
    colour = torch.zeros(per, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for s in range(0, RECORDS, 8):
        hx.insert_kmers_dev(dk.data_ptr() + s * per * K, colour.data_ptr(), per)
    ctx.synchronize()
    hx.finalize()
    groupings = {"2 000 loci x 10 alleles": np.arange(0, RECORDS + 1, 10, dtype=np.int64), "20 000 loci x 1 allele": np.arange(RECORDS + 1, dtype=np.int64),
                 "2 loci x 10 000 alleles": np.array([0, RECORDS // 2, RECORDS], np.int64)}
    d_hits = torch.zeros(RECORDS * G, dtype=torch.int32, device=dev)
    d_words = torch.zeros(RECORDS * rs, dtype=torch.int64, device=dev)
    d_miss = torch.zeros(RECORDS, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(RECORDS * G * 4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    log(f"index: {G} colours, m = {m}, n = {n}, k = {K}, row stride {rs} words; {RECORDS} segments x {per} k-mers = {nw} k-mers; counters {RECORDS * G * 4 / 1e6:.1f} MB")

    def timed(label, call):
        call(); ctx.synchronize()
        ms = []
        for _ in range(5):
            ctx.timer_start(); call(); ms.append(ctx.timer_stop_ms())
        log(f"{label}: best {min(ms):.3f} ms, median {sorted(ms)[2]:.3f} ms")
        return min(ms)

    seg = timed("cid_search_segments_dev (memsets + k_search_segments)                  ",
                lambda: hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, d_hits.data_ptr(), d_miss.data_ptr()))
    timed("cid_search_perfect_segments_dev (memsets + k_perfect_segments + finish)",
          lambda: hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, d_words.data_ptr(), d_miss.data_ptr()))
    hits = d_hits.cpu().numpy().view(np.uint32).reshape(RECORDS, G)
    for name, go in groupings.items():
        dg = torch.from_numpy(go).to(dev)
        torch.cuda.synchronize()
        t = timed(f"cid_search_nearest_segments_dev, {name:24s} (the above + preset + k_nearest_groups)",
                  lambda: hx.search_nearest_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, dg.data_ptr(), len(go) - 1, d_out.data_ptr()))
        cells = d_out.cpu().numpy().view(np.uint32).reshape(-1, 4)[:(len(go) - 1) * G].reshape(len(go) - 1, G, 4)
        # equal lengths: the best share is the largest counter, the first segment that has it
        want = np.stack([go[g] + hits[go[g]:go[g + 1]].argmax(axis=0) for g in range(len(go) - 1)])
        top = np.stack([hits[go[g]:go[g + 1]].max(axis=0) for g in range(len(go) - 1)])
        ok = np.array_equal(cells[..., 1], top) and np.array_equal(cells[..., 0][top > 0], want[top > 0].astype(np.uint32))
        log(f"    nearest - counters = {t - seg:.3f} ms; cells equal the counters' argmax: {bool(ok)}; {int((cells[..., 3] > 0).sum())} cells with a perfect segment")
    hx.close(); ctx.close()


if __name__ == "__main__":
    {"cli": cli, "kernels": kernels}[sys.argv[1]]()
