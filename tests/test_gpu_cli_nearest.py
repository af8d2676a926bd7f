"""`colorid search -s -m --alleles PREFIX --nearest -p MIN_SHARE` end to end on the four-phage index of test_gpu_cli_alleles.py:
PREFIX.nearest.tsv equals a file computed here from the oracle's counters (search_count per record), and stdout, stderr and the tables
are those of the run without --nearest, plus one closing line on stderr.

The rule.  Locus = the label up to its first '_', allele = the text between the first and the second '_'.  Per (locus, accession) the
records of the locus that have k-mers and hit at least once are candidates, in input order over all query files; the best is the one with
the largest share kmers_hit / kmers, compared exactly (hit_a * len_b against hit_b * len_a), the earlier record on a tie.  A line is
written for every accession (colour order) and locus (byte order) where the accession holds no record of the locus completely and the
best share is at least MIN_SHARE.

The scheme, cut from the genomes, over two query files:
  locA  a perfect allele for two accessions, and a 1 %-mutated copy of another accession's sequence: that accession's nearest allele is
        the locus's second record
  locD  two mutated alleles (1 % and 3 %): no column in the tables, nearest lines
  locE  shorter than k: a warning, an empty segment, no locus
  locT  the same mutated record twice: equal shares, the earlier record wins
  locR  3 % mutated in the first file, 1 % mutated in the second: the locus recurs, the better allele comes later
  locP  150 genuine bases and 350 random ones: a share near 0.26, which -p 0.5 removes and -p 0 keeps
  locF  an N inside
With COLORID_MF_BATCH_RECORDS=3 the batch boundaries fall inside the runs of locD and of locT."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli_alleles import TABLES, read_tables
from test_gpu_cli_segments import ACGT, BANNER, K, PHAGES, REFS, WARNING, mutate, write_fasta

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
HEADER = "accession\tlocus\tallele\tkmers_hit\tkmers\tshare\n"
P = 0.5


def run(*args, env=None, ok=True):
    clean = {k: v for k, v in os.environ.items() if k not in ("COLORID_REDUCE", "COLORID_MF_BATCH_RECORDS", "COLORID_TIMING")}
    p = subprocess.run([BIN, *args], capture_output=True, text=True, env=dict(clean, **(env or {})))
    assert (p.returncode == 0) == ok, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout, p.stderr


def scheme(genomes):
    rng = np.random.default_rng(41)
    g = genomes
    twice = mutate(rng, g[2][2000:2500], 0.01)
    recurs = g[1][9000:9500]
    a = [("locA_1", g[0][3700:4200]),
         ("locA_2", mutate(rng, g[1][5000:5500], 0.01)),
         ("locD_1", mutate(rng, g[3][15500:16100], 0.01)), ("locD_2", mutate(rng, g[3][15500:16100], 0.03)),
         ("locE_1", g[0][3700:3700 + K - 1]),
         ("locT_1", twice), ("locT_2", twice),
         ("locR_1", mutate(rng, recurs, 0.03)),
         ("locP_1", g[0][10000:10150] + ACGT[rng.integers(0, 4, 350)].tobytes())]
    b = [("locF_3", g[1][3400:3800] + b"N" + g[1][3801:4200]),
         ("locR_2_later", mutate(rng, recurs, 0.01)),
         ("locD_5", mutate(rng, g[3][15500:16100], 0.05))]
    return a, b


def nearest_lines(cells, loci, accessions, p):
    out = []
    for c, acc in enumerate(accessions):
        for locus in loci:
            best, n_perfect = cells[(locus, c)]
            if n_perfect == 0 and best is not None and best[1] / best[2] >= p:
                out.append("%s\t%s\t%s\t%d\t%d\t%.3f\n" % (acc, locus, best[0].split("_")[1], best[1], best[2], best[1] / best[2]))
    return out


@pytest.fixture(scope="module")
def env(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_nearest")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in reversed(PHAGES)))
    run("build", "-s", "750000", "-n", "4", "-k", str(K), "-b", str(d / "phage"), "-r", str(tsv))
    oix = orc.Index.build_single(str(tsv), 750000, 4, K)
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    a, b = scheme(genomes)
    fa, fb = d / "scheme_a.fasta", d / "scheme_b.fasta"
    write_fasta(fa, a)
    write_fasta(fb, b)
    # per (locus, accession): the best record so far as (label, hits, k-mers), in input order, and the number of perfect records
    accessions = oix.colors()
    cells, loci, first_of = {}, set(), {}
    for f in (fa, fb):
        labels, seqs = orc.read_fasta_mf(str(f))
        for lab, s in zip(labels, seqs):
            lab = lab.decode()
            locus = lab.split("_")[0]
            first_of.setdefault(locus, lab)
            km = orc.Kmers(K)
            if km.kmerize_string(s) != 0 or len(km) == 0:
                continue
            loci.add(locus)
            hits = oix.search_count(km.keys(), None, want_unique=False)[0]
            n = len(km)
            for c in range(len(accessions)):
                best, n_perfect = cells.get((locus, c), (None, 0))
                h = int(hits[c])
                if h > 0 and (best is None or h * best[2] > best[1] * n):
                    best = (lab, h, n)
                cells[(locus, c)] = (best, n_perfect + (h == n))
    loci = [l.decode() for l in sorted(l.encode() for l in loci)]
    return d, str(d / "phage.bxi"), [str(fa), str(fb)], cells, loci, accessions, first_of


def test_nearest_file_from_one_search(env):
    d, bxi, files, cells, loci, accessions, first_of = env
    want = nearest_lines(cells, loci, accessions, P)
    everything = nearest_lines(cells, loci, accessions, 0.0)
    # the expected file shows what the scheme was cut for
    assert loci == ["locA", "locD", "locF", "locP", "locR", "locT"]                          # locE has no k-mers
    rows = [l.rstrip("\n").split("\t") for l in want]
    assert any(r[1] == "locD" for r in rows)                                                  # a locus without a column
    assert any(0 < float(r[5]) < 1 and f"{r[1]}_{r[2]}" != "_".join(first_of[r[1]].split("_")[:2]) for r in rows)     # not its locus's first record
    assert any(r[1] == "locA" and r[2] == "2" for r in rows)                                  # the mutated copy, not the locus's first record
    assert any(r[1] == "locR" and r[2] == "2" for r in rows)                                  # the better allele came with the second file
    assert any(r[1] == "locT" and r[2] == "1" for r in rows) and not any(r[1] == "locT" and r[2] == "2" for r in rows)   # equal shares: the earlier
    removed = [l for l in everything if l not in want]
    assert removed and any(l.split("\t")[1] == "locP" for l in removed)                       # what -p removes
    assert all(cells[(r[1], accessions.index(r[0]))][1] == 0 for r in rows)
    assert any(n_perfect > 0 for _, n_perfect in cells.values())                              # locA's perfect cells: no line
    plain_out, plain_err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "plain"))
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "t"), "--nearest", "-p", str(P))
    assert out == plain_out and WARNING % "locE_1" in out
    closing = err.splitlines()[-1]
    assert closing == f"alleles: {len(want)} nearest-allele calls (share >= {P:g}) written to {d / 't'}.nearest.tsv"
    assert err.replace(str(d / "t"), "PREFIX") == plain_err.replace(str(d / "plain"), "PREFIX") + closing.replace(str(d / "t"), "PREFIX") + "\n"
    assert read_tables(d / "t") == read_tables(d / "plain")
    assert "locD" not in read_tables(d / "t")["raw.tsv"].splitlines()[0].split("\t")
    assert not os.path.exists(d / "plain.nearest.tsv")
    assert open(d / "t.nearest.tsv").read() == HEADER + "".join(want)
    # -p 0: every cell with a candidate and no perfect record
    run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "p0"), "--nearest", "-p", "0")
    assert open(d / "p0.nearest.tsv").read() == HEADER + "".join(everything)
    assert read_tables(d / "p0") == read_tables(d / "plain")


def test_batch_boundaries_inside_a_locus_change_nothing(env):
    d, bxi, files, cells, loci, accessions, _ = env
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "whole"), "--nearest", "-p", str(P))
    for n in ("3", "1"):
        out_n, err_n = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / f"cut{n}"), "--nearest", "-p", str(P),
                           env={"COLORID_MF_BATCH_RECORDS": n})
        assert out_n == out and err_n.replace(str(d / f"cut{n}"), "PREFIX") == err.replace(str(d / "whole"), "PREFIX")
        assert read_tables(d / f"cut{n}") == read_tables(d / "whole")
        assert open(d / f"cut{n}.nearest.tsv").read() == open(d / "whole.nearest.tsv").read() == HEADER + "".join(nearest_lines(cells, loci, accessions, P))
    # the switch alone, without --nearest: the rows and the tables of the plain run
    out_s, _ = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "sw"), env={"COLORID_MF_BATCH_RECORDS": "3"})
    assert out_s == out and read_tables(d / "sw") == read_tables(d / "whole")


def test_a_label_without_underscore_ends_the_run_without_a_nearest_file(env, orc):
    d, bxi, files, *_ = env
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    bad = d / "bad.fasta"
    write_fasta(bad, [("locA_1", genomes[0][3700:4200]), ("nounderscore", genomes[2][2000:2500])])
    _, err = run("search", "-b", bxi, "-q", str(bad), "-s", "-m", "--alleles", str(d / "bad"), "--nearest", ok=False)
    assert "the label 'nounderscore' has no '_'" in err
    assert not os.path.exists(d / "bad.nearest.tsv") and not os.path.exists(d / "bad.raw.tsv")
