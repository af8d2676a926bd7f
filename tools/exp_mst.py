#!/usr/bin/env python3
"""`dists --mst` on a scheme-sized table WITH population structure (profiles/mst_summary.md): 8 192 accessions x 3 000 loci descended from
48 founders (20 alleles a locus, uniform) by a handful of allele changes each — every accession copies an earlier one of its lineage
and changes 0 .. 6 loci — and 5 % of the cells NA: zero distances and ties are frequent, lineages are far apart.  (The uniform table of
tools/exp_dists.py has neither.)  Run on the GPU box from the repository root:
    python3 tools/exp_mst.py table       writes the table (MST_WORK, default /tmp/cid_mst)
    python3 tools/exp_mst.py lib         cid_dists_forest through colorid_amd.Dists, five calls timed on the host clock (the call ends in a
                                         stream synchronise), its rounds; then the honest baseline: both matrices fetched with
                                         cid_dists_rows in blocks of 1 024 rows into two held A x A arrays and Prim's algorithm over them
                                         on the host (numpy), transfer included; the two forests must be equal edge for edge
    python3 tools/exp_mst.py kernels     what a `rocprofv3 --kernel-trace --stats -- python3 tools/exp_mst.py kernels` run should trace:
                                         three passes of cid_dists_rows over the whole table in blocks of 1 024 rows (k_dists_tile) and,
                                         where the library has it, one cid_dists_forest (k_dists_best).  COLORID_HIP_LIB chooses the library:
                                         the same mode on the parent commit's library gives k_dists_tile's time before this change
    python3 tools/exp_mst.py cli         three runs each of `colorid dists --mst` and `colorid dists --mst --no-matrices`, COLORID_TIMING=1"""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
W = os.environ.get("MST_WORK", "/tmp/cid_mst"); os.makedirs(W, exist_ok=True)
A, L, ALLELES, MISSING, FOUNDERS = int(os.environ.get("MST_A", 8192)), int(os.environ.get("MST_L", 3000)), 20, 0.05, 48
TABLE, OUT = os.path.join(W, "table.tsv"), os.path.join(W, "out")


def log(*a, **kw):
    print(*a, flush=True, **kw)


def codes():
    kept = os.path.join(W, f"codes_{A}x{L}.npy")     # (the modes of one session share it)
    if os.path.exists(kept):
        return np.load(kept)
    c = make_codes()
    np.save(kept, c)
    return c


def make_codes():
    rng = np.random.default_rng(11)
    c = np.zeros((A, L), np.uint32)
    n_f = min(FOUNDERS, A)
    c[:n_f] = rng.integers(1, ALLELES + 1, size=(n_f, L), dtype=np.uint32)
    lineage = np.arange(A) % n_f
    for a in range(n_f, A):
        earlier = np.flatnonzero(lineage[:a] == lineage[a])
        c[a] = c[int(rng.choice(earlier))]
        loci = rng.choice(L, size=int(rng.integers(0, 7)), replace=False)
        c[a, loci] = rng.integers(1, ALLELES + 1, size=len(loci), dtype=np.uint32)
    c[rng.random((A, L)) < MISSING] = 0
    return c


def write_table():
    c = codes()
    text = np.array([b"NA"] + [str(i).encode() for i in range(1, ALLELES + 1)], dtype=object)
    with open(TABLE, "wb") as f:
        f.write(b"\t" + b"\t".join(b"loc%04d" % l for l in range(L)) + b"\n")
        for a in range(A):
            f.write(b"iso%05d\t" % a + b"\t".join(text[c[a]]) + b"\n")
    log(f"table: {A} accessions x {L} loci from {min(FOUNDERS, A)} founders, {os.path.getsize(TABLE) / 1e6:.1f} MB, "
        f"{float((c == 0).mean()):.4f} of the cells NA -> {TABLE}")


def prim(differ, compared, M=1):
    """the minimum spanning forest under the edge key (differ, -compared, lo, hi) by Prim's algorithm over the two held matrices"""
    n = len(differ)
    idx = np.arange(n, dtype=np.int64)
    INF = np.iinfo(np.int64).max

    def keys(i):     # the key of {i, j} for every j as one integer; no edge: INF
        k = ((differ[i].astype(np.int64) * (L + 1) + (L - compared[i].astype(np.int64))) * n + np.minimum(idx, i)) * n + np.maximum(idx, i)
        k[compared[i] < M] = INF
        k[i] = INF
        return k
    in_tree = np.zeros(n, bool)
    best = np.full(n, INF)
    via = np.full(n, -1, np.int64)
    edges = []
    for _ in range(n):
        cand = np.where(in_tree, INF, best)
        j = int(cand.argmin())
        if cand[j] == INF:                      # nothing reaches the trees so far: a new tree at the first accession left
            j = int(np.flatnonzero(~in_tree)[0])
        else:
            i = int(via[j])
            edges.append((int(cand[j]), min(i, j), max(i, j), int(differ[i, j]), int(compared[i, j])))
        in_tree[j] = True
        k = keys(j)
        better = k < best
        best[better] = k[better]
        via[better] = j
    return [e[1:] for e in sorted(edges)]


def mode_lib():
    import colorid_amd
    c = codes()
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, c)
    d.forest()                                  # warm-up: code objects, scratch blocks
    for rep in range(5):
        t = time.perf_counter()
        edges, rounds = d.forest()
        log(f"cid_dists_forest, call {rep}: {(time.perf_counter() - t) * 1e3:.2f} ms, {rounds} rounds, {len(edges)} edges, "
            f"{A - len(edges)} trees, total length {int(edges[:, 2].sum())}")
    t = time.perf_counter()
    differ, compared = np.zeros((A, A), np.uint32), np.zeros((A, A), np.uint32)
    for r0 in range(0, A, 1024):
        differ[r0:r0 + 1024], compared[r0:r0 + 1024] = d.rows(r0, min(1024, A - r0))
    t_rows = time.perf_counter() - t
    t = time.perf_counter()
    want = prim(differ, compared)
    t_prim = time.perf_counter() - t
    log(f"host baseline: {differ.nbytes + compared.nbytes} bytes held (two {A} x {A} u32 matrices); cid_dists_rows in blocks of 1 024 rows "
        f"{t_rows * 1e3:.1f} ms, Prim (numpy) {t_prim * 1e3:.1f} ms, together {(t_rows + t_prim) * 1e3:.1f} ms")
    got = [tuple(int(v) for v in e) for e in edges]
    assert got == want, "the device's forest is not Prim's"
    log(f"the two forests are equal edge for edge; differ = 0 on {sum(1 for e in got if e[2] == 0)} edges")
    d.close(); ctx.close()


def mode_kernels():
    import colorid_amd
    c = codes()
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, c)
    for _ in range(3):
        for r0 in range(0, A, 1024):
            d.rows(r0, min(1024, A - r0))
    if hasattr(d.lib, "cid_dists_forest"):
        edges, rounds = d.forest()
        log(f"forest: {rounds} rounds, {len(edges)} edges")
    log(f"library: {colorid_amd._lib.LIB_PATH}")
    d.close(); ctx.close()


def run_cli(label, *flags):
    t = time.time()
    p = subprocess.run([BIN, "dists", "-t", TABLE, "-o", OUT, *flags], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_TIMING="1"), timeout=900)
    dt = time.time() - t
    if p.returncode != 0:
        log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
    ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
    log(f"{label}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph))
    return p


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "lib"
    if mode == "table" or (mode == "cli" and not os.path.exists(TABLE)):
        write_table()
    if mode == "lib":
        mode_lib()
    elif mode == "kernels":
        mode_kernels()
    elif mode == "cli":
        for rep in range(3):                    # alternating, so that both see the same box
            p = run_cli(f"dists --mst, run {rep}", "--mst")
            q = run_cli(f"dists --mst --no-matrices, run {rep}", "--mst", "--no-matrices")
        log("".join(l + "\n" for l in (p.stderr + q.stderr).splitlines() if l.startswith("dists: ")), end="")
