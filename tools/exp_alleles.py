#!/usr/bin/env python3
"""`colorid search -s -m` on a scheme-sized input: the batched route (one cid_search_perfect_segments call per batch of records)
against one cid_search_perfect call per record (a parent build; this tree's group path on one rank), through the whole command line, and k_perfect_segments beside
k_search_segments on the same k-mers and offsets (DESIGN.md §4 "Segmented perfect search", §5; profiles/alleles_summary.md).
Index: the benchmark's shape — 256 colours, m = 50 M, n = 4, k = 31 — built by `colorid build` over 256 genomes of 1 Mbp that are one
ancestor with 1 % substitutions each (one species: most k-mers of an allele are in most accessions); scheme: 20 000 records x 500 bp
named locN_A, cut from the genomes, every fifth with 1 % substitutions of its own.  Run on the GPU box from the repo root:
    python3 tools/exp_alleles.py cli     > profiles/alleles_cli.txt      (ALLELES_PARENT_BIN=<a parent build's bin/colorid> adds its -s -m)
    python3 tools/exp_alleles.py kernels > profiles/alleles_kernels.txt  (under rocprofv3 --kernel-trace --stats for the kernel times)
`cli` prints, per case and repetition, the wall clock and the CLI's phase lines (COLORID_TIMING=1), and the host's share of the `search`
phase: reading and k-merising the records alone (`colorid debug-kmers --mode mf`, no GPU)."""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
W = os.environ.get("ALLELES_WORK", "/tmp/cid_alleles"); os.makedirs(W, exist_ok=True)
G, LG, RECORDS, RL, K = 256, 1_000_000, 20_000, 500, 31
acgt = np.frombuffer(b"ACGT", np.uint8)


def log(*a):
    print(*a, flush=True)


def substitute(rng, s, rate):
    s = s.copy()
    e = rng.integers(0, len(s), int(len(s) * rate))
    s[e] = acgt[rng.integers(0, 4, e.size)]
    return s


def genomes_of_one_species(n):
    rng = np.random.default_rng(5)
    ancestor = acgt[rng.integers(0, 4, LG)]
    return [substitute(rng, ancestor, 0.01) for _ in range(n)]


def scheme(genomes):
    """RECORDS alleles of RECORDS / 10 loci: locus l is the stretch [l * RL, (l + 1) * RL) of the genomes"""
    rng = np.random.default_rng(11)
    recs = []
    for i in range(RECORDS):
        locus = i // 10
        s = genomes[int(rng.integers(0, len(genomes)))][locus * RL:(locus + 1) * RL]
        recs.append((f"loc{locus}_{i % 10 + 1}", substitute(rng, s, 0.01) if i % 5 == 4 else s))
    return recs


def run(label, binary, args, reps=3, env=None):
    for rep in range(reps):
        t = time.time()
        p = subprocess.run([binary, *args], capture_output=True, text=True, env=dict(os.environ, COLORID_TIMING="1", **(env or {})), timeout=600)
        dt = time.time() - t
        if p.returncode != 0:
            log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
        ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
        log(f"{label} rep {rep}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph) + f" | {p.stdout.count(chr(10)) - 3} stdout lines")
    return p


def cli():
    genomes = genomes_of_one_species(G)
    with open(f"{W}/refs.tsv", "w") as tsv:
        for g, s in enumerate(genomes):
            with open(f"{W}/g{g:03d}.fasta", "wb") as f:
                f.write(f">genome{g}\n".encode() + s.tobytes() + b"\n")
            tsv.write(f"genome{g:03d}\t{W}/g{g:03d}.fasta\n")
    run("build -k 31 -s 50000000 -n 4 (256 x 1 Mbp)", BIN, ["build", "-s", "50000000", "-n", "4", "-k", str(K), "-b", f"{W}/idx", "-r", f"{W}/refs.tsv"], reps=1)
    log(f"index: {os.path.getsize(f'{W}/idx.bxi') / 1e9:.2f} GB")
    with open(f"{W}/scheme.fasta", "wb") as f:
        for label, s in scheme(genomes):
            f.write(b">" + label.encode() + b"\n" + s.tobytes() + b"\n")
    q = ["search", "-b", f"{W}/idx.bxi", "-q", f"{W}/scheme.fasta", "-s", "-m"]
    parent = os.environ.get("ALLELES_PARENT_BIN")
    a = run("-s -m (parent build: per record)      ", parent, q) if parent else None
    b = run("-s -m (this tree: batched)            ", BIN, q)
    c = run("-s -m --alleles (this tree: batched)  ", BIN, q + ["--alleles", f"{W}/t"])
    d = run("-s -m --alleles (per record: 1 rank)  ", BIN, q + ["--alleles", f"{W}/u", "--gpus", "1"], env={"COLORID_REDUCE": "host"})
    if a:
        log("parent's -s -m stdout == this tree's:", a.stdout == b.stdout)
    log("stdout of --alleles == -s -m:", c.stdout == b.stdout, "; per-record --alleles:", d.stdout == b.stdout)
    log("tables of the two routes are the same files:", all(open(f"{W}/t.{e}").read() == open(f"{W}/u.{e}").read() for e in ("raw.tsv", "detailed.tsv", "report.out")))
    log("\n".join(l for l in c.stderr.splitlines() if l.startswith("alleles:") or l.startswith("timing: -s -m")))
    t = time.time()
    p = subprocess.run([BIN, "debug-kmers", "--mode", "mf", "-k", str(K), "-q", f"{W}/scheme.fasta"], capture_output=True, text=True, timeout=600)
    log(f"host alone, reading and k-merising the {p.stdout.count('>')} records (debug-kmers --mode mf, whole process): {1e3 * (time.time() - t):.0f} ms")


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
    p_row = bench.fill_background_fast(dev, ptr, m, rs, G, 1.0 - math.exp(-n * LG / m), seed=7)
    torch.cuda.synchronize()
    recs = [s for _, s in scheme(genomes_of_one_species(8))]
    wins = np.concatenate([np.lib.stride_tricks.sliding_window_view(s, K) for s in recs])
    nw, per = len(wins), RL - K + 1
    seg_off = np.arange(RECORDS + 1, dtype=np.int64) * per
    dk = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1)).to(dev)
    do = torch.from_numpy(seg_off).to(dev)
    # one species: an allele's k-mers are in most accessions.  G rounds of "every k-mer into one random colour" leave a (k-mer, colour) pair
    # present with probability 1 - (1 - 1/G)^G = 0.63; one allele in every eight goes into colour 0 whole, so that perfect hits exist
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    for _ in range(G):
        colour = torch.randint(0, G, (nw,), device=dev, dtype=torch.int32, generator=gen)
        torch.cuda.synchronize()
        hx.insert_kmers_dev(dk.data_ptr(), colour.data_ptr(), nw)
        ctx.synchronize()
    colour = torch.zeros(per, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for s in range(0, RECORDS, 8):
        hx.insert_kmers_dev(dk.data_ptr() + s * per * K, colour.data_ptr(), per)   # (8 * per * K bytes: a multiple of 16)
    ctx.synchronize()
    hx.finalize()
    d_hits = torch.zeros(RECORDS * G, dtype=torch.int32, device=dev)
    d_words = torch.zeros(RECORDS * rs, dtype=torch.int64, device=dev)
    d_miss = torch.zeros(RECORDS, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    log(f"index: {G} colours, m = {m}, n = {n}, k = {K}, background density {p_row:.4f}, row stride {rs} words; {RECORDS} segments x {per} k-mers = {nw} k-mers")

    def timed(label, call):
        call(); ctx.synchronize()
        ms = []
        for _ in range(5):
            ctx.timer_start(); call(); ms.append(ctx.timer_stop_ms())
        log(f"{label}: best {min(ms):.3f} ms, median {sorted(ms)[2]:.3f} ms  ({nw / min(ms) / 1e6:.2f} G k-mers/s)")
        return min(ms)

    seg = timed("cid_search_segments_dev (memsets + k_search_segments)                 ",
                lambda: hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, d_hits.data_ptr(), d_miss.data_ptr()))
    per_ = timed("cid_search_perfect_segments_dev (memsets + k_perfect_segments + finish)",
                 lambda: hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, d_words.data_ptr(), d_miss.data_ptr()))
    log(f"perfect / counters = {per_ / seg:.2f}")
    hits = d_hits.cpu().numpy().view(np.uint32).reshape(RECORDS, G)
    words = d_words.cpu().numpy().view("<u4").reshape(RECORDS, 2 * rs)[:, :G // 32]
    flagged = d_miss.cpu().numpy().astype(bool)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)
    log("AND words == (counters == segment length) where no row is absent:", bool(np.array_equal(bits[~flagged], (hits == per)[~flagged])),
        f"; {int(flagged.sum())} segments flagged, {int(bits.any(axis=1).sum())} with a perfect hit")
    hx.close(); ctx.close()


if __name__ == "__main__":
    {"cli": cli, "kernels": kernels}[sys.argv[1]]()
