#!/usr/bin/env python3
"""`dists --hist` and `dists --levels` on the table of tools/exp_mst.py (profiles/hist_summary.md): 8 192 accessions x 3 000 loci from 48
founders, 5 % NA.  Run on the GPU box from the repository root:
    python3 tools/exp_hist.py table        writes the table (HIST_WORK, default /tmp/cid_hist)
    python3 tools/exp_hist.py lib          cid_dists_hist through colorid_amd.Dists over all rows, upper and full mode: five calls each on
                                           the host clock (a call ends in a stream synchronise), the bytes that crossed the bus; the
                                           histograms must equal those of both matrices fetched with cid_dists_rows and counted with
                                           numpy, and their running sum at T = 7 the count of cid_dists_within
    python3 tools/exp_hist.py kernels      what a `rocprofv3 --kernel-trace --stats -- python3 tools/exp_hist.py kernels` run should
                                           trace, three times over and alternating: cid_dists_hist upper, cid_dists_within (a count)
                                           upper, cid_dists_hist full, cid_dists_within full, one round of cid_dists_best — five
                                           launches a round in that order, the same walk under three epilogues
    python3 tools/exp_hist.py cli          three runs each of `colorid dists --hist --no-matrices`, `colorid dists --levels 0,2,7,20
                                           --no-matrices` and `colorid dists --cluster 7 --no-matrices`, alternating, COLORID_TIMING=1"""
import os, sys, time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MST_WORK", os.environ.get("HIST_WORK", "/tmp/cid_hist"))
import exp_mst
from exp_mst import A, L, codes, log, run_cli

T = 7
LEVELS = "0,2,7,20"


def mode_lib():
    import colorid_amd
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, codes())
    got = {}
    for upper in (True, False):
        d.hist(1, upper=upper)                                     # warm-up: code objects, scratch blocks
        for rep in range(5):
            t = time.perf_counter()
            got[upper] = d.hist(1, upper=upper)
            log(f"cid_dists_hist, {'upper' if upper else 'full'}, all {A} rows, call {rep}: {(time.perf_counter() - t) * 1e3:.2f} ms; "
                f"{2 * (L + 1) * 8} bytes over the bus")
    differ, compared = np.zeros((A, A), np.uint32), np.zeros((A, A), np.uint32)
    for r0 in range(0, A, 1024):
        differ[r0:r0 + 1024], compared[r0:r0 + 1024] = d.rows(r0, min(1024, A - r0))
    off = ~np.eye(A, dtype=bool)
    want_c = np.bincount(compared[off], minlength=L + 1).astype(np.uint64)
    want_d = np.bincount(differ[off & (compared >= 1)], minlength=L + 1).astype(np.uint64)
    assert np.array_equal(got[False][0], want_d) and np.array_equal(got[False][1], want_c)
    assert np.array_equal(got[True][0] * 2, want_d) and np.array_equal(got[True][1] * 2, want_c)
    for upper in (True, False):
        assert int(np.cumsum(got[upper][0])[T]) == d.within_count(T, 1, upper=upper)
    dh, ch = got[True]
    busy_d, busy_c = np.flatnonzero(dh), np.flatnonzero(ch)
    log(f"both histograms equal numpy over the two matrices; upper: {int(ch.sum())} pairs, {int(ch[0])} without a common locus; differ in "
        f"{len(busy_d)} bins from {busy_d[0]} to {busy_d[-1]}, the fullest bin {int(dh.argmax())} with {int(dh.max())} pairs; compared in "
        f"{len(busy_c)} bins from {busy_c[0]} to {busy_c[-1]}; {int(np.cumsum(dh)[T])} pairs within {T}")
    d.close(); ctx.close()


def mode_kernels():
    import colorid_amd
    ctx = colorid_amd.Context(0)
    d = colorid_amd.Dists(ctx, codes())
    own = np.arange(A, dtype=np.uint32)
    for _ in range(3):
        for upper in (True, False):
            dh, ch = d.hist(1, upper=upper)
            n = d.within_count(T, 1, upper=upper)
        d.best(own, 1)
    log(f"3 rounds of: k_dists_hist upper, k_dists_within upper, k_dists_hist full, k_dists_within full, k_dists_best; "
        f"{int(ch.sum())} ordered pairs counted, {n} within {T}")
    log(f"library: {colorid_amd._lib.LIB_PATH}; {A} x {L}")
    d.close(); ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "lib"
    if mode == "table" or (mode == "cli" and not os.path.exists(exp_mst.TABLE)):
        exp_mst.write_table()
    if mode == "lib":
        mode_lib()
    elif mode == "kernels":
        mode_kernels()
    elif mode == "cli":
        for rep in range(3):                                       # alternating, so that all see the same box
            p = run_cli(f"dists --hist --no-matrices, run {rep}", "--hist", "--no-matrices")
            q = run_cli(f"dists --levels {LEVELS} --no-matrices, run {rep}", "--levels", LEVELS, "--no-matrices")
            r = run_cli(f"dists --cluster {T} --no-matrices, run {rep}", "--cluster", str(T), "--no-matrices")
        log("".join(l + "\n" for l in (p.stderr + q.stderr + r.stderr).splitlines() if l.startswith("dists: ")), end="")
