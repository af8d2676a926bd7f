#!/usr/bin/env python3
"""`colorid search -g -m --coverage` against `-g -m` through the whole command line, and the coverage kernels beside k_search_segments
on the same k-mers (DESIGN.md §4 "Coverage search", §5).  Index: the benchmark's shape — 256 colours, m = 50 M, n = 4, k = 31 — built by
`colorid build` over 256 synthetic 1 Mbp genomes; panel: 5 000 records x 1 kb cut from the genomes with 2 % substitutions.  Run on the
GPU box from the repo root:
    python3 tools/exp_cover.py cli     > profiles/cover_cli.txt       (COVER_PARENT_BIN=<a parent build's bin/colorid> adds its -g -m)
    python3 tools/exp_cover.py kernels > profiles/cover_kernels.txt
`cli` prints, per case and repetition, the wall clock and the CLI's phase lines (COLORID_TIMING=1); `kernels` prints ctx-timer
milliseconds (cid_timer_start / _stop_ms around the device-pointer calls, best and median of 5)."""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
W = os.environ.get("COVER_WORK", "/tmp/cid_cover"); os.makedirs(W, exist_ok=True)
G, LG, RECORDS, RL, K = 256, 1_000_000, 5_000, 1_000, 31
acgt = np.frombuffer(b"ACGT", np.uint8)


def log(*a):
    print(*a, flush=True)


def panel(genomes):
    rng = np.random.default_rng(11)
    recs = []
    for i in range(RECORDS):
        g = genomes[int(rng.integers(0, len(genomes)))]
        st = int(rng.integers(0, len(g) - RL))
        s = g[st:st + RL].copy()
        e = rng.integers(0, RL, RL // 50)
        s[e] = acgt[rng.integers(0, 4, e.size)]
        recs.append(s)
    return recs


def run(label, binary, args, reps=3):
    for rep in range(reps):
        t = time.time()
        p = subprocess.run([binary, *args], capture_output=True, text=True, env=dict(os.environ, COLORID_TIMING="1"), timeout=300)
        dt = time.time() - t
        if p.returncode != 0:
            log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
        ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
        log(f"{label} rep {rep}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph) + f" | {p.stdout.count(chr(10)) - 3} rows")
    return p


def cli():
    rng = np.random.default_rng(5)
    genomes = []
    with open(f"{W}/refs.tsv", "w") as tsv:
        for g in range(G):
            s = acgt[rng.integers(0, 4, LG)]
            genomes.append(s)
            with open(f"{W}/g{g:03d}.fasta", "wb") as f:
                f.write(f">genome{g}\n".encode() + s.tobytes() + b"\n")
            tsv.write(f"genome{g:03d}\t{W}/g{g:03d}.fasta\n")
    run("build -k 31 -s 50000000 -n 4 (256 x 1 Mbp)", BIN, ["build", "-s", "50000000", "-n", "4", "-k", str(K), "-b", f"{W}/idx", "-r", f"{W}/refs.tsv"], reps=1)
    log(f"index: {os.path.getsize(f'{W}/idx.bxi') / 1e9:.2f} GB")
    with open(f"{W}/panel.fasta", "wb") as f:
        for i, s in enumerate(panel(genomes)):
            f.write(b">gene%d\n" % i + s.tobytes() + b"\n")
    q = ["search", "-b", f"{W}/idx.bxi", "-q", f"{W}/panel.fasta", "-g", "-m"]
    parent = os.environ.get("COVER_PARENT_BIN")
    a = run("-g -m (parent build)      ", parent, q) if parent else None
    b = run("-g -m (this tree)         ", BIN, q)
    c = run("-g -m --coverage          ", BIN, q + ["--coverage"])
    if a:
        log("parent's -g -m stdout == this tree's:", a.stdout == b.stdout)
    log("columns 1-4 of --coverage == -g -m:", ["\t".join(l.split("\t")[:4]) for l in c.stdout.splitlines()[3:]] == b.stdout.splitlines()[3:])
    tails = np.array([l.split("\t")[4:] for l in c.stdout.splitlines()[3:]], float)
    log(f"--coverage rows: {len(tails)}; mean breadth {tails[:, 0].mean():.3f}, mean stretches {tails[:, 2].mean():.2f}, mean longest stretch {tails[:, 1].mean():.0f} bases")


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
    p = bench.fill_background_fast(dev, ptr, m, rs, G, 1.0 - math.exp(-n * LG / m), seed=7)
    torch.cuda.synchronize()
    hx.finalize()
    rng = np.random.default_rng(5)
    recs = panel([acgt[rng.integers(0, 4, LG)] for _ in range(8)])
    wins = np.concatenate([np.lib.stride_tricks.sliding_window_view(s, K) for s in recs])     # every window's k bytes, in order
    nw, per = len(wins), RL - K + 1
    seg_off = np.arange(RECORDS + 1, dtype=np.int64) * per
    dk = torch.from_numpy(np.ascontiguousarray(wins).reshape(-1)).to(dev)
    do = torch.from_numpy(seg_off).to(dev)
    d_none = torch.zeros(2, dtype=torch.int64, device=dev)                                     # one empty segment: the statistics launch does nothing
    d_hits = torch.zeros(RECORDS * G, dtype=torch.int32, device=dev)
    d_cells = torch.zeros(RECORDS * G * 8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    log(f"index: {G} colours, m = {m}, n = {n}, k = {K}, background density {p:.4f}, row stride {rs} words; {RECORDS} segments x {per} windows = {nw} windows")

    def timed(label, call):
        call(); ctx.synchronize()
        ms = []
        for _ in range(5):
            ctx.timer_start(); call(); ms.append(ctx.timer_stop_ms())
        log(f"{label}: best {min(ms):.3f} ms, median {sorted(ms)[2]:.3f} ms  ({nw / min(ms) / 1e6:.2f} G windows/s)")
        return min(ms)

    seg = timed("k_search_segments                      ", lambda: hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), RECORDS, nw, d_hits.data_ptr()))
    rows = timed("k_cover_rows (+ an empty k_cover_stats) ", lambda: hx.search_cover_dev(dk.data_ptr(), d_none.data_ptr(), None, 1, nw, d_cells.data_ptr()))
    both = timed("k_cover_rows + k_cover_stats            ", lambda: hx.search_cover_dev(dk.data_ptr(), do.data_ptr(), None, RECORDS, nw, d_cells.data_ptr()))
    log(f"k_cover_stats by difference: {both - rows:.3f} ms; coverage / segments = {both / seg:.2f}")
    cells = d_cells.cpu().numpy().view(np.uint32).reshape(RECORDS, G, 8)
    log("kmers_hit == k_search_segments' counters:", bool(np.array_equal(cells[:, :, 0], d_hits.cpu().numpy().view(np.uint32).reshape(RECORDS, G))))
    hx.close(); ctx.close()


if __name__ == "__main__":
    {"cli": cli, "kernels": kernels}[sys.argv[1]]()
