#!/usr/bin/env python3
"""`dists --closest K` on the table of tools/exp_mst.py (profiles/closest_summary.md): 8 192 accessions x 3 000 loci from 48 founders, 5 %
NA, and the --query pair of tools/exp_within.py (16 of its accessions against the other 8 176).  Run on the GPU box from the repository root:
    python3 tools/exp_closest.py table        writes the table and the --query pair (CLOSEST_WORK, default /tmp/cid_closest)
    python3 tools/exp_closest.py lib          cid_dists_closest through colorid_amd.Dists over all rows, K = 1, 10 and 64: five calls each
                                              on the host clock (a call ends in a stream synchronise and the unpacking), the bytes of
                                              scratch and the bytes that crossed the bus; K = 1 must equal cid_dists_best with every
                                              accession its own component, K = 10 and 64 within 7 must equal cid_dists_within sorted and cut
    python3 tools/exp_closest.py kernels K    what a `rocprofv3 --kernel-trace --stats -- python3 tools/exp_closest.py kernels K` run
                                              should trace: three cid_dists_closest calls over all rows at that K (k_dists_closest, one
                                              launch a call, and k_dists_closest_merge, two levels a call at 128 column tiles), and beside
                                              them the yardsticks of the same run: three rounds of cid_dists_best (k_dists_best) and three
                                              full-mode counts of cid_dists_within at T = 7 (k_dists_within) — the same walk, other epilogues
    python3 tools/exp_closest.py cli          three runs each of `colorid dists --closest 10 --no-matrices`, `colorid dists --cluster 7
                                              --no-matrices` and `colorid dists --query ... --closest 10`, alternating, COLORID_TIMING=1"""
import os, re, subprocess, sys, time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("WITHIN_WORK", os.environ.get("CLOSEST_WORK", "/tmp/cid_closest"))
import exp_within                                                  # the --query pair is that script's, the table exp_mst's
import exp_mst
from exp_mst import A, L, codes, log, run_cli
from exp_within import DB, NEW, T

KS = (1, 10, 64)
UNBOUNDED = 0xFFFFFFFF


def run_query(label, k):
    t = time.time()
    p = subprocess.run([exp_mst.BIN, "dists", "-t", DB, "--query", NEW, "-o", exp_mst.OUT, "--closest", str(k)], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_TIMING="1"), timeout=900)
    dt = time.time() - t
    if p.returncode != 0:
        log(label, "FAILED", p.stderr[-1500:]); sys.exit(1)
    ph = re.findall(r"timing: ([A-Za-z ]+?) (\d+) ms \(at (\d+) ms\)", p.stderr)
    log(f"{label}: wall {dt:.3f} s | " + ", ".join(f"{n} {ms}" for n, ms, _ in ph))
    return p


def mode_lib():
    import colorid_amd
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, codes())
    tiles = (A + 63) // 64
    got = {}
    for k in KS:
        d.closest(k)                                               # warm-up: code objects, scratch blocks
        for rep in range(5):
            t = time.perf_counter()
            got[k] = d.closest(k)
            log(f"cid_dists_closest, K = {k}, all {A} rows, call {rep}: {(time.perf_counter() - t) * 1e3:.2f} ms; scratch {A * tiles * k * 8} bytes "
                f"of per-tile keys + {A * ((tiles + 63) // 64) * k * 8} + {A * k * 8} of the merge's two levels; {A * k * 8} bytes over the bus")
    b, bd, bc = d.best(np.arange(A, dtype=np.uint32), 1)
    assert np.array_equal(got[1][:, 0, 1], b) and np.array_equal(got[1][:, 0, 2], bd) and np.array_equal(got[1][:, 0, 3], bc)
    log(f"K = 1 equals cid_dists_best with every accession its own component: {int((b != UNBOUNDED).sum())} accessions have a nearest")
    for k in KS[1:]:                                               # the prefix property: the K nearest are the first K of the 64 nearest
        assert np.array_equal(got[k], got[64][:, :k])
    pairs = d.within(T, 1, upper=False)
    start = np.searchsorted(pairs[:, 0], np.arange(A + 1))
    for k in KS[1:]:
        t = time.perf_counter()
        near = d.closest(k, T, 1)
        dt = time.perf_counter() - t
        for a in range(A):
            mine = pairs[start[a]:start[a + 1]].astype(np.int64)
            mine = mine[np.lexsort((mine[:, 1], -mine[:, 3], mine[:, 2]))][:k]
            assert np.array_equal(near[a, :len(mine)], mine) and (near[a, len(mine):, 1] == UNBOUNDED).all()
        log(f"K = {k} within {T} equals cid_dists_within's {len(pairs)} ordered pairs sorted and cut, order included: {dt * 1e3:.2f} ms, "
            f"{int((near[:, :, 1] != UNBOUNDED).sum())} neighbours")
    d.close(); ctx.close()


def mode_kernels(k):
    import colorid_amd
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, codes())
    for _ in range(3):
        near = d.closest(k)
    log(f"closest {k}: {int((near[:, :, 1] != UNBOUNDED).sum())} neighbours of {A} accessions, 3 calls: 3 launches of k_dists_closest, 6 of "
        f"k_dists_closest_merge")
    own = np.arange(A, dtype=np.uint32)
    for _ in range(3):
        d.best(own, 1)
        n = d.within_count(T, 1, upper=False)
    log(f"yardsticks: 3 launches of k_dists_best, 3 of k_dists_within (full mode, T = {T}: {n} ordered pairs counted)")
    log(f"library: {colorid_amd._lib.LIB_PATH}; {A} x {L}")
    d.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "lib"
    if mode == "table" or (mode == "cli" and not os.path.exists(NEW)):
        exp_within.write_tables()
    if mode == "lib":
        mode_lib()
    elif mode == "kernels":
        mode_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 10)
    elif mode == "cli":
        for rep in range(3):                                       # alternating, so that all see the same box
            p = run_cli(f"dists --closest 10 --no-matrices, run {rep}", "--closest", "10", "--no-matrices")
            q = run_cli(f"dists --cluster {T} --no-matrices, run {rep}", "--cluster", str(T), "--no-matrices")
            r = run_query(f"dists -t db --query new --closest 10, run {rep}", 10)
        log("".join(l + "\n" for l in (p.stderr + q.stderr + r.stderr).splitlines() if l.startswith("dists: ")), end="")
