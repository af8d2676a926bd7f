#!/usr/bin/env python3
"""`colorid dists` on a scheme-sized table (profiles/dists_summary.md): 8 192 accessions x 3 000 loci, 5 % of the cells NA, 20 alleles a
locus, drawn uniformly (a table without population structure: about 95 % of the compared loci of a pair differ; the kernel's work does not
depend on the values).  Run on the GPU box from the repository root:
    python3 tools/exp_dists.py table                 writes the table (DISTS_WORK, default /tmp/cid_dists)
    python3 tools/exp_dists.py cli                   three runs of `colorid dists --cluster 7` with COLORID_TIMING=1: wall clock and phase lines,
                                                     and 32 rows of both matrices checked against numpy
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- colorid_amd/bin/colorid dists -t $DISTS_WORK/table.tsv -o $DISTS_WORK/out --cluster 7
                                                     one run of the command line on its own, for the kernels' times
    python3 tools/exp_dists.py cpu                   tools/bin/dists_cpu_loop (make -C tools bin/dists_cpu_loop) on the same table, 16 threads"""
import os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "colorid_amd", "bin", "colorid")
W = os.environ.get("DISTS_WORK", "/tmp/cid_dists"); os.makedirs(W, exist_ok=True)
A, L, ALLELES, MISSING = int(os.environ.get("DISTS_A", 8192)), int(os.environ.get("DISTS_L", 3000)), 20, 0.05
TABLE, OUT = os.path.join(W, "table.tsv"), os.path.join(W, "out")


def log(*a, **kw):
    print(*a, flush=True, **kw)


def codes():
    rng = np.random.default_rng(7)
    c = rng.integers(1, ALLELES + 1, size=(A, L), dtype=np.uint32)
    c[rng.random((A, L)) < MISSING] = 0
    return c


def write_table():
    c = codes()
    text = np.array([b"NA"] + [str(i).encode() for i in range(1, ALLELES + 1)], dtype=object)
    with open(TABLE, "wb") as f:
        f.write(b"\t" + b"\t".join(b"loc%04d" % l for l in range(L)) + b"\n")
        for a in range(A):
            f.write(b"iso%05d\t" % a + b"\t".join(text[c[a]]) + b"\n")
    log(f"table: {A} accessions x {L} loci, {os.path.getsize(TABLE) / 1e6:.1f} MB, {float((c == 0).mean()):.4f} of the cells NA -> {TABLE}")


def run_cli(label):
    t = time.time()
    p = subprocess.run([BIN, "dists", "-t", TABLE, "-o", OUT, "--cluster", "7"], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_TIMING="1"), timeout=900)
    dt = time.time() - t
    if p.returncode != 0:
        log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
    ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
    log(f"{label}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph))
    return p


def check_rows():
    c = codes()
    called = c != 0
    rows = sorted(set(int(r) for r in np.random.default_rng(1).integers(0, A, 30)) | {0, A - 1})
    want_d, want_c = {}, {}
    for i in rows:
        both = called[i][None, :] & called
        want_c[i] = both.sum(1)
        want_d[i] = (both & (c != c[i][None, :])).sum(1)
    for name, want in (("dists", want_d), ("compared", want_c)):
        with open(f"{OUT}.{name}.tsv") as f:
            f.readline()
            for i, line in enumerate(f):
                if i in want:
                    got = np.array(line.rstrip("\n").split("\t")[1:], dtype=np.int64)
                    assert np.array_equal(got, want[i]), (name, i)
    log(f"{len(rows)} rows of dists.tsv and compared.tsv equal numpy; clusters.tsv: {sum(1 for _ in open(OUT + '.clusters.tsv')) - 1} lines")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "cli"
    if mode == "table" or not os.path.exists(TABLE):
        write_table()
    if mode == "cli":
        for rep in range(3):
            p = run_cli(f"dists --cluster 7, run {rep}")
        log("".join(l + "\n" for l in p.stderr.splitlines() if l.startswith("dists: ")), end="")
        check_rows()
    elif mode == "cpu":
        p = subprocess.run([os.path.join(ROOT, "tools", "bin", "dists_cpu_loop"), TABLE, "16"], capture_output=True, text=True, timeout=900)
        log(p.stdout.strip() or p.stderr[-500:])
