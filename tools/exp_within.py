#!/usr/bin/env python3
"""`dists --within T` and `dists --query` on the table of tools/exp_mst.py (profiles/within_summary.md): 8 192 accessions x 3 000 loci from
48 founders, 5 % NA — it has population structure, so `--within 7` finds pairs.  Run on the GPU box from the repository root:
    python3 tools/exp_within.py table      writes the table and the --query pair: the table without 16 of its accessions, and those 16
                                           (WITHIN_WORK, default /tmp/cid_within)
    python3 tools/exp_within.py lib        cid_dists_within through colorid_amd.Dists, T = 7: upper and full mode, five calls each timed on
                                           the host clock (a call ends in a stream synchronise and a host sort), the pairs found and the
                                           bytes that crossed the bus; then the same lists from both matrices fetched with cid_dists_rows
                                           in blocks of 1 024 rows and filtered with numpy, transfer included; they must be equal
    python3 tools/exp_within.py kernels    what a `rocprofv3 --kernel-trace --stats -- python3 tools/exp_within.py kernels` run should
                                           trace: three passes of cid_dists_rows over the whole table in blocks of 1 024 rows (k_dists_tile),
                                           one cid_dists_forest (k_dists_best) and, where the library has it, three counts and three lists
                                           in upper and in full mode (k_dists_within: one launch a call unless the list overflowed).
                                           COLORID_HIP_LIB chooses the library: the parent commit's gives the two older kernels before
    python3 tools/exp_within.py cli        three runs each of `colorid dists --within 7 --no-matrices`, `colorid dists --cluster 7
                                           --no-matrices` and `colorid dists --query ... --within 7`, alternating, COLORID_TIMING=1"""
import ctypes as C
import os, re, subprocess, sys, time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MST_WORK", os.environ.get("WITHIN_WORK", "/tmp/cid_within"))
import exp_mst                                                     # the table, its codes and the timed CLI run are that script's
from exp_mst import A, TABLE, W, codes, log, run_cli

T = int(os.environ.get("WITHIN_T", 7))
ASKED = np.arange(16) * (A // 16) + 5                              # the 16 query accessions: spread over the table
DB, NEW = os.path.join(W, "db.tsv"), os.path.join(W, "new.tsv")


def write_tables():
    exp_mst.write_table()
    lines = open(TABLE, "rb").read().split(b"\n")
    asked = set(int(a) + 1 for a in ASKED)
    with open(DB, "wb") as f:
        f.write(b"\n".join(l for k, l in enumerate(lines) if k not in asked))
    with open(NEW, "wb") as f:
        f.write(b"\n".join([lines[0]] + [lines[k] for k in sorted(asked)]) + b"\n")
    log(f"query pair: {A - len(asked)} accessions -> {DB}, {len(asked)} -> {NEW}")


def run_query(label):
    """exp_mst.run_cli with the two tables of the --query pair"""
    t = time.time()
    p = subprocess.run([exp_mst.BIN, "dists", "-t", DB, "--query", NEW, "-o", exp_mst.OUT, "--within", str(T)], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_TIMING="1"), timeout=900)
    dt = time.time() - t
    if p.returncode != 0:
        log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
    ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
    log(f"{label}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph))
    return p


def listed(d, upper):
    """one count and one list with exactly that room: two calls, each one walk"""
    n = d.within_count(T, 1, upper=upper)
    out = np.zeros((max(n, 1), 4), np.uint32)
    m = C.c_uint64(0)
    rc = d.lib.cid_dists_within(d.h, 0, A, T, 1, 1 if upper else 0, out.ctypes.data, n, C.byref(m))
    assert rc == 0 and m.value == n
    return out[:n]


def mode_lib():
    import colorid_amd
    c = codes()
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, c)
    got = {}
    for upper in (True, False):
        listed(d, upper)                                           # warm-up: code objects, scratch blocks
        for rep in range(5):
            t = time.perf_counter()
            n = d.within_count(T, 1, upper=upper)
            t_count = time.perf_counter() - t
            t = time.perf_counter()
            got[upper] = listed(d, upper)
            log(f"cid_dists_within, T = {T}, {'upper' if upper else 'full'}, call {rep}: count {t_count * 1e3:.2f} ms, count + list "
                f"{(time.perf_counter() - t) * 1e3:.2f} ms, {n} pairs, {16 * n} bytes of entries and 16 bytes of cursor over the bus")
    t = time.perf_counter()
    differ, compared = np.zeros((A, A), np.uint32), np.zeros((A, A), np.uint32)
    for r0 in range(0, A, 1024):
        differ[r0:r0 + 1024], compared[r0:r0 + 1024] = d.rows(r0, min(1024, A - r0))
    t_rows = time.perf_counter() - t
    t = time.perf_counter()
    ok = (compared >= 1) & (differ <= T)
    np.fill_diagonal(ok, False)
    a, b = np.nonzero(ok)
    full = np.stack([a, b, differ[a, b], compared[a, b]], 1).astype(np.uint32)
    t_np = time.perf_counter() - t
    log(f"host baseline: {differ.nbytes + compared.nbytes} bytes over the bus and held (two {A} x {A} u32 matrices); cid_dists_rows in blocks of "
        f"1 024 rows {t_rows * 1e3:.1f} ms, numpy filter {t_np * 1e3:.1f} ms")
    assert np.array_equal(got[False], full) and np.array_equal(got[True], full[full[:, 1] > full[:, 0]])
    log(f"both lists equal the matrices' cells with differ <= {T} and compared >= 1, order included: {len(got[True])} upper, {len(got[False])} full; "
        f"differ = 0 on {int((got[True][:, 2] == 0).sum())} of the upper pairs")
    d.close(); ctx.close()


def mode_kernels():
    import colorid_amd
    c = codes()
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, c)
    for _ in range(3):
        for r0 in range(0, A, 1024):
            d.rows(r0, min(1024, A - r0))
    edges, rounds = d.forest()
    log(f"forest: {rounds} rounds, {len(edges)} edges")
    if hasattr(d.lib, "cid_dists_within"):
        for upper in (True, False):
            for _ in range(3):
                n = len(listed(d, upper))
            log(f"within {T}, {'upper' if upper else 'full'}: {n} pairs, 3 counts and 3 lists: 6 launches of k_dists_within unless a list overflowed")
    log(f"library: {colorid_amd._lib.LIB_PATH}")
    d.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "lib"
    if mode == "table" or (mode == "cli" and not os.path.exists(NEW)):
        write_tables()
    if mode == "lib":
        mode_lib()
    elif mode == "kernels":
        mode_kernels()
    elif mode == "cli":
        for rep in range(3):                                       # alternating, so that all see the same box
            p = run_cli(f"dists --within {T} --no-matrices, run {rep}", "--within", str(T), "--no-matrices")
            q = run_cli(f"dists --cluster {T} --no-matrices, run {rep}", "--cluster", str(T), "--no-matrices")
            r = run_query(f"dists -t db --query new --within {T}, run {rep}")
        log("".join(l + "\n" for l in (p.stderr + q.stderr + r.stderr).splitlines() if l.startswith("dists: ")), end="")
