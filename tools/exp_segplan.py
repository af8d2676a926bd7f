#!/usr/bin/env python3
"""The host forms of the segmented searches before and after a change to their walk (DESIGN.md §4 "Segmented search", Host form): a parent
build's bin/colorid and this tree's alternate on the scheme-sized input of tools/exp_alleles.py (20 000 records x 500 bp, 256 colours,
m = 50 M, n = 4, k = 31), and every run's library-call lines are kept — `search -s -m` for cid_search_perfect_segments,
`search -s -m --alleles P --nearest` for cid_search_nearest_segments.  The bar is the parent's own spread: this tree's median within the
parent's min..max.  Run on the GPU box from the repo root:
    SEGPLAN_PARENT_BIN=<a parent build's bin/colorid> python3 tools/exp_segplan.py > profiles/segplan_ab.txt"""
import os, re, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exp_alleles as ea
from exp_alleles import BIN, G, K, W, log

PARENT = os.environ["SEGPLAN_PARENT_BIN"]
ROUNDS = 5


def once(binary, args):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=dict(os.environ, COLORID_TIMING="1"), timeout=300)
    if p.returncode != 0:
        log("FAILED", binary, args, p.returncode, p.stderr[-1500:]); sys.exit(1)
    calls = {m[0]: (int(m[1]), int(m[2])) for m in re.findall(r"timing: -s -m (batched|--nearest): (\d+) \w+ calls (\d+) ms", p.stderr)}
    search = re.findall(r"timing: search (\d+) ms", p.stderr)
    return p, calls, int(search[0]) if search else -1


def main():
    genomes = ea.genomes_of_one_species(G)
    with open(f"{W}/refs.tsv", "w") as tsv:
        for g, s in enumerate(genomes):
            with open(f"{W}/g{g:03d}.fasta", "wb") as f:
                f.write(f">genome{g}\n".encode() + s.tobytes() + b"\n")
            tsv.write(f"genome{g:03d}\t{W}/g{g:03d}.fasta\n")
    ea.run("build -k 31 -s 50000000 -n 4 (256 x 1 Mbp)", BIN, ["build", "-s", "50000000", "-n", "4", "-k", str(K), "-b", f"{W}/idx", "-r", f"{W}/refs.tsv"], reps=1)
    with open(f"{W}/scheme.fasta", "wb") as f:
        for label, s in ea.scheme(genomes):
            f.write(b">" + label.encode() + b"\n" + s.tobytes() + b"\n")
    q = ["search", "-b", f"{W}/idx.bxi", "-q", f"{W}/scheme.fasta", "-s", "-m"]
    log("per run: the library-call line(s) of the CLI (COLORID_TIMING=1; whole ms, as it prints them), and its `search` phase")
    cases = (("-s -m", [], "batched"), ("-s -m --alleles P --nearest", ["--alleles", None, "--nearest"], "--nearest"))
    ms, last = {}, {}
    for rnd in range(ROUNDS):      # the binaries alternate: whatever else runs on the host meets both alike
        for case, extra, key in cases:
            for who, binary in (("parent", PARENT), ("this tree", BIN)):
                p, calls, search = once(binary, q + [f"{W}/{who[0]}" if a is None else a for a in extra])
                last[(case, who)] = p
                ms.setdefault((case, who), []).append(calls[key][1])
                log(f"round {rnd}: {case:28s} {who:9s}: " + ", ".join(f"{k} {n} calls {t} ms" for k, (n, t) in sorted(calls.items())) + f" | search {search} ms")
    for case, _, key in cases:
        a, b = ms[(case, "parent")], ms[(case, "this tree")]
        log(f"{case} ({'cid_search_nearest_segments' if key == '--nearest' else 'cid_search_perfect_segments'} calls): parent {a} ms, min {min(a)} max {max(a)} "
            f"median {statistics.median(a)}; this tree {b} ms, median {statistics.median(b)} -> within the parent's min..max: {min(a) <= statistics.median(b) <= max(a)}")
        log(f"    stdout the same bytes: {last[(case, 'parent')].stdout == last[(case, 'this tree')].stdout}")
    log("tables of --nearest the same files:", all(open(f"{W}/p.{e}").read() == open(f"{W}/t.{e}").read() for e in ("raw.tsv", "detailed.tsv", "report.out", "nearest.tsv")))


if __name__ == "__main__":
    main()
