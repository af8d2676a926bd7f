"""`colorid dists --hist`, `--levels T1,T2,..` and `search -s -m --alleles PREFIX --dists --hist --levels ..` end to end, on the generated
70 x 40 table of test_gpu_cli_dists.py (missing cells, two pairs without a common locus, near copies) with three accessions made
identical: PREFIX.hist.tsv against numpy over the PREFIX.dists.tsv and PREFIX.compared.tsv of the same run and against
tests/hist_ref.py, the same bytes without the matrices, its running sum against the lines of PREFIX.within.tsv; PREFIX.levels.tsv
against the `cluster` column of --cluster t runs, with and without --mst beside it; the search entrance; a table of one accession."""
import os

import numpy as np
import pytest

import hist_ref
from test_gpu_cli_alleles import run
from test_gpu_cli_alleles import env  # noqa: F401  (the module-scoped fixture: the four-phage index and its scheme)
from test_gpu_cli_dists import generated_table, matrices, parse_table
from test_gpu_cli_mst import clusters_of

pytestmark = pytest.mark.gpu

EXTS = ("dists.tsv", "compared.tsv", "clusters.tsv", "mst.tsv", "mst.nwk", "within.tsv", "closest.tsv", "hist.tsv", "levels.tsv")
HEADER = "loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n"


def read_files(prefix):
    return {ext: open(f"{prefix}.{ext}").read() for ext in EXTS if os.path.exists(f"{prefix}.{ext}")}


def dists_lines(err):
    return [l for l in err.splitlines() if l.startswith("dists: ")]


def the_table():
    """the generated table with accessions 21 and 22 given the cells of accession 20: three identical accessions"""
    text, accs = generated_table()
    lines = text.split("\n")
    for a in (21, 22):
        lines[1 + a] = accs[a] + "\t" + lines[1 + 20].split("\t", 1)[1]
    return "\n".join(lines), accs


def read_matrix(text):
    return np.array([[int(v) for v in l.split("\t")[1:]] for l in text.splitlines()[1:]], np.int64)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """per M the files and the stderr of `dists --hist --levels 7,0,2` with the matrices"""
    d = tmp_path_factory.mktemp("cli_hist")
    text, accs = the_table()
    (d / "t.tsv").write_text(text)
    out = {}
    for M in (1, 20):
        extra = ["--min-compared", str(M)] if M != 1 else []
        _, err = run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"full{M}"), "--hist", "--levels", "7,0,2", *extra)
        out[M] = (read_files(d / f"full{M}"), err)
    return d, text, accs, out


@pytest.mark.parametrize("M", [1, 20])
def test_hist_file_against_the_matrices_of_the_same_run(runs, M):
    d, text, accs, out = runs
    got, err = out[M]
    assert sorted(got) == ["compared.tsv", "dists.tsv", "hist.tsv", "levels.tsv"]
    differ, compared = read_matrix(got["dists.tsv"]), read_matrix(got["compared.tsv"])
    assert differ.shape == compared.shape == (70, 70)
    above = np.triu(np.ones((70, 70), bool), 1)
    ch = np.bincount(compared[above], minlength=41)
    dh = np.bincount(differ[above & (compared >= M)], minlength=41)
    want = HEADER + "".join(f"{n}\t{dh[n]}\t{dh[:n + 1].sum()}\t{ch[n]}\n" for n in range(41))
    assert got["hist.tsv"] == want
    _, loci, cells = parse_table(text)
    assert got["hist.tsv"] == hist_ref.hist_tsv(*matrices(cells, len(loci)), 40, M)            # ... and from the table's text
    assert ch[0] >= 2 and ch.sum() == 70 * 69 // 2 and dh[0] >= 3                               # no common locus; the identical three
    prefix = str(d / f"full{M}")
    left_out = int(ch[:M].sum())
    assert f"dists: 2415 pairs counted, {left_out} of them left out of the differ columns for sharing fewer than {M} loci, written to {prefix}.hist.tsv" \
        in dists_lines(err)
    assert left_out >= ch[0] and (M == 1 or left_out > ch[0])


@pytest.mark.parametrize("M", [1, 20])
def test_without_the_matrices_the_same_bytes(runs, M):
    d, text, accs, out = runs
    extra = ["--min-compared", str(M)] if M != 1 else []
    _, err = run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"bare{M}"), "--hist", "--no-matrices", *extra)
    got = read_files(d / f"bare{M}")
    assert got == {"hist.tsv": out[M][0]["hist.tsv"]}
    assert dists_lines(err)[0] == "dists: 70 accessions x 40 loci, matrices not written (--no-matrices)" and len(dists_lines(err)) == 2


@pytest.mark.parametrize("T,M", [(0, 1), (3, 1), (3, 20), (40, 1)])
def test_the_running_sum_is_the_number_of_lines_of_within(runs, T, M):
    d, text, accs, out = runs
    extra = ["--min-compared", str(M)] if M != 1 else []
    run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"w{T}_{M}"), "--within", str(T), "--no-matrices", *extra)
    n_lines = len(open(d / f"w{T}_{M}.within.tsv").read().splitlines()) - 1
    row = out[M][0]["hist.tsv"].splitlines()[1 + T].split("\t")
    assert int(row[0]) == T and int(row[2]) == n_lines and n_lines > 0


@pytest.mark.parametrize("M", [1, 20])
def test_levels_are_the_clusters_at_each_threshold(runs, M):
    d, text, accs, out = runs
    extra = ["--min-compared", str(M)] if M != 1 else []
    got = out[M][0]["levels.tsv"]
    lines = [l.split("\t") for l in got.splitlines()]
    assert lines[0] == ["accession", "T7", "T2", "T0", "address"] and [l[0] for l in lines[1:]] == accs   # descending t, table order
    for col, t in ((1, 7), (2, 2), (3, 0)):
        run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"c{t}_{M}"), "--cluster", str(t), "--no-matrices", *extra)
        assert [int(l[col]) for l in lines[1:]] == clusters_of(open(d / f"c{t}_{M}.clusters.tsv").read()), t
    assert all(l[4] == ".".join(l[1:4]) for l in lines[1:])
    assert lines[1 + 20][3] == lines[1 + 21][3] == lines[1 + 22][3]                            # the identical three: one cluster at 0
    assert lines[1][1:] == ["1", "1", "1", "1.1.1"]
    _, loci, cells = parse_table(text)
    assert got == hist_ref.levels_tsv(accs, *matrices(cells, len(loci)), [7, 0, 2], M)
    n = [max(int(l[c]) for l in lines[1:]) for c in (1, 2, 3)]
    assert n[0] <= n[1] <= n[2] and n[0] < n[2]
    assert (f"dists: cluster addresses of 70 accessions (at least {M} shared): {n[0]} at <= 7, {n[1]} at <= 2, {n[2]} at <= 0 differing loci, "
            f"written to {d / f'full{M}'}.levels.tsv") in dists_lines(out[M][1])
    # with --mst beside it: the same file, and the forest's files as a run without --levels writes them
    run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"lm{M}"), "--levels", "7,0,2", "--mst", "--no-matrices", *extra)
    run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"m{M}"), "--mst", "--no-matrices", *extra)
    both, mst = read_files(d / f"lm{M}"), read_files(d / f"m{M}")
    assert sorted(both) == ["levels.tsv", "mst.nwk", "mst.tsv"] and both["levels.tsv"] == got
    assert sorted(mst) == ["mst.nwk", "mst.tsv"] and all(both[k] == mst[k] for k in mst)
    # the order the thresholds are given in does not matter
    run("dists", "-t", str(d / "t.tsv"), "-o", str(d / f"lo{M}"), "--levels", "0,2,7", "--no-matrices", *extra)
    assert read_files(d / f"lo{M}") == {"levels.tsv": got}


def test_search_dists_writes_what_dists_writes_from_the_raw_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "sh"), "--dists", "--hist", "--levels", "0,2,7")
    run("dists", "-t", str(d / "sh.raw.tsv"), "-o", str(d / "sh_again"), "--hist", "--levels", "0,2,7")
    got = read_files(d / "sh")
    assert sorted(got) == ["compared.tsv", "dists.tsv", "hist.tsv", "levels.tsv"] and got == read_files(d / "sh_again")
    # four accessions x four loci; Listeria_phage_B051 and Listeria_phage_B545 share locB_4: the one pair with a common call
    assert got["hist.tsv"] == HEADER + "0\t1\t1\t5\n1\t0\t1\t1\n2\t0\t1\t0\n3\t0\t1\t0\n4\t0\t1\t0\n"
    assert got["levels.tsv"] == ("accession\tT7\tT2\tT0\taddress\nListeria_phage_B021\t1\t1\t1\t1.1.1\nListeria_phage_B056\t2\t2\t2\t2.2.2\n"
                                 "Listeria_phage_B051\t3\t3\t3\t3.3.3\nListeria_phage_B545\t3\t3\t3\t3.3.3\n")


def test_a_table_of_one_accession(tmp_path):
    (tmp_path / "one.tsv").write_text("\tl1\tl2\tl3\nonly\t4\tNA\t7\n")
    _, err = run("dists", "-t", str(tmp_path / "one.tsv"), "-o", str(tmp_path / "o"), "--hist", "--levels", "1", "--no-matrices")
    assert read_files(tmp_path / "o") == {"hist.tsv": HEADER + "0\t0\t0\t0\n1\t0\t0\t0\n2\t0\t0\t0\n3\t0\t0\t0\n",
                                          "levels.tsv": "accession\tT1\taddress\nonly\t1\t1\n"}
    assert "dists: 0 pairs counted, 0 of them left out" in err
