"""`colorid dists -t TABLE -o PREFIX [--cluster T [--min-compared M]]` and `search -s -m --alleles PREFIX --dists` end to end.  The expected
PREFIX.dists.tsv, PREFIX.compared.tsv and PREFIX.clusters.tsv are derived here from the table's text: numpy for the two matrices
(compared = called @ called.T, differ = both called and another allele text), a plain union-find for the clusters.  The table of
tests/golden/alleles, a generated 70 x 40 table (string alleles, NA and empty cells, pairs of accessions without a common locus), the
four-phage scheme of test_gpu_cli_alleles.py through the search's own context, and an empty table."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli_alleles import BIN, ROOT, read_tables, run
from test_gpu_cli_alleles import env  # noqa: F401  (the module-scoped fixture: the four-phage index and its scheme)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "alleles", "expected.raw.tsv")
FILES = ("dists.tsv", "compared.tsv", "clusters.tsv")


def parse_table(text):
    """-> (accessions, loci, cells): cells[a][l] is the allele text, None where the table says NA or nothing"""
    lines = text.split("\n")
    head = lines[0].split("\t")
    assert head[0] == ""
    loci = [] if head[1:] == [""] else head[1:]
    accs, cells = [], []
    for line in lines[1:]:
        if line == "":
            continue
        f = line.split("\t")
        assert len(f) == len(loci) + 1
        accs.append(f[0])
        cells.append([None if c in ("NA", "") else c for c in f[1:]])
    return accs, loci, cells


def matrices(cells, n_loci):
    """(differ, compared) by the issue's numpy formulas over codes numbered per locus in order of first appearance"""
    A = len(cells)
    codes = np.zeros((A, n_loci), np.int64)
    for l in range(n_loci):
        seen = {}
        for a in range(A):
            if cells[a][l] is not None:
                codes[a, l] = seen.setdefault(cells[a][l], len(seen) + 1)
    called = codes != 0
    compared = called.astype(np.int64) @ called.astype(np.int64).T
    differ = ((codes[:, None, :] != codes[None, :, :]) & called[:, None, :] & called[None, :, :]).sum(-1)
    return differ.reshape(A, A), compared.reshape(A, A)


def matrix_text(accs, m):
    head = "\t" + "\t".join(accs) + "\n" if accs else "\t\n"
    return head + "".join(accs[i] + "".join(f"\t{int(v)}" for v in m[i]) + "\n" for i in range(len(accs)))


def clusters_text(accs, differ, compared, T, M=1):
    A = len(accs)
    M = max(M, 1)
    parent = list(range(A))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for i in range(A):
        for j in range(i + 1, A):
            if compared[i][j] >= M and differ[i][j] <= T:
                a, b = find(i), find(j)
                if a != b:
                    parent[b] = a
    roots = [find(i) for i in range(A)]
    number = {}
    for r in roots:                                    # numbered from 1 in order of their first member
        number.setdefault(r, len(number) + 1)
    out = "accession\tcluster\tsize\tnearest\tdiffer\tcompared\n"
    for i in range(A):
        cand = [(differ[i][j], -compared[i][j], j) for j in range(A) if j != i and compared[i][j] >= M]
        if cand:
            d, c, j = min(cand)
            near = f"{accs[j]}\t{int(d)}\t{int(-c)}"
        else:
            near = "-\t-\t-"
        out += f"{accs[i]}\t{number[roots[i]]}\t{roots.count(roots[i])}\t{near}\n"
    return out, number, roots


def expected(text, T=None, M=1):
    accs, loci, cells = parse_table(text)
    differ, compared = matrices(cells, len(loci))
    want = {"dists.tsv": matrix_text(accs, differ), "compared.tsv": matrix_text(accs, compared)}
    if T is not None:
        want["clusters.tsv"] = clusters_text(accs, differ, compared, T, M)[0]
    return want


def read_files(prefix):
    return {ext: open(f"{prefix}.{ext}").read() for ext in FILES if os.path.exists(f"{prefix}.{ext}")}


def closing(err, prefix, A, L, T=None):
    lines = [l for l in err.splitlines() if l.startswith("dists: ")]
    assert lines[0] == f"dists: {A} accessions x {L} loci written to {prefix}.dists.tsv, {prefix}.compared.tsv"
    assert len(lines) == (1 if T is None else 2)
    if T is not None:
        assert lines[1].startswith("dists: ") and f" clusters of 2 or more at <= {T} differing loci hold " in lines[1]
        assert lines[1].endswith(f" accessions, written to {prefix}.clusters.tsv")
    return lines


def test_the_golden_table(tmp_path):
    text = open(GOLD).read()
    out, err = run("dists", "-t", GOLD, "-o", str(tmp_path / "g"), "--cluster", "1")
    got = read_files(tmp_path / "g")
    assert got == expected(text, 1)
    # by hand: acc_A and acc_C share abcZ (12 / 12) and lmo0001 (1 / 2); acc_B and acc_C share lmo0001 (1 / 2) only
    rows = {l.split("\t")[0]: l.split("\t")[1:] for l in got["dists.tsv"].splitlines()[1:]}
    comp = {l.split("\t")[0]: l.split("\t")[1:] for l in got["compared.tsv"].splitlines()[1:]}
    names = got["dists.tsv"].splitlines()[0].split("\t")[1:]
    assert names == ["acc_A", "acc_B", "acc_C", "acc_late", "sample 4"]
    assert rows["acc_A"][2] == "1" and comp["acc_A"][2] == "2" and rows["acc_C"][0] == "1" and comp["acc_C"][0] == "2"
    assert comp["acc_A"][0] == "3" and rows["acc_A"][0] == "0"              # the diagonal: acc_A's called loci, no difference
    assert comp["acc_C"][3] == "0" and rows["acc_C"][3] == "0"              # acc_C and acc_late: no locus in common
    last = closing(err, str(tmp_path / "g"), 5, 6, 1)[1]
    assert "dists: 1 clusters of 2 or more at <= 1 differing loci hold 5 accessions" in last
    # without --cluster: two files
    run("dists", "-t", GOLD, "-o", str(tmp_path / "n"))
    assert sorted(read_files(tmp_path / "n")) == ["compared.tsv", "dists.tsv"]


def generated_table():
    """70 accessions x 40 loci: alleles are strings (numbers, hashes, INF- calls), 15 % NA and 5 % empty cells; accessions 0 / 1 and 2 / 3
    have no called locus in common (0 and 2 call the first 20 loci only, 1 and 3 the last 20); 10 .. 14 are near copies of 9"""
    rng = np.random.default_rng(40)
    A, L = 70, 40
    pool = ["1", "2", "3", "17", "INF-4", "a3f9", "novel*", "0"]
    cells = [[pool[int(rng.integers(0, len(pool)))] for _ in range(L)] for _ in range(A)]
    for a in range(9, 15):
        cells[a] = list(cells[9])
        for l in rng.choice(L, size=a - 9, replace=False):
            cells[a][int(l)] = "x%d" % a
    for a in range(A):
        for l in range(L):
            u = rng.random()
            if a >= 4 and u < 0.15:
                cells[a][l] = "NA"
            elif a >= 4 and u < 0.20:
                cells[a][l] = ""
    for a, half in ((0, 0), (1, 1), (2, 0), (3, 1)):
        for l in range(L):
            if (l >= L // 2) != bool(half):
                cells[a][l] = "NA" if l % 2 else ""
    cells[3][L - 1] = "NA"                      # (a line may end in an empty cell, but not every line: acc3 ends in NA)
    loci = ["loc%03d" % l for l in range(L)]
    accs = ["iso %d" % a if a % 7 == 0 else "iso_%d" % a for a in range(A)]
    return "\t" + "\t".join(loci) + "\n" + "".join(accs[a] + "\t" + "\t".join(cells[a]) + "\n" for a in range(A)), accs


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_dists")
    text, accs = generated_table()
    (d / "table.tsv").write_text(text + "\n")   # (a trailing empty line is skipped)
    return d, text, accs


@pytest.mark.parametrize("T,M", [(0, None), (3, None), (3, 20)], ids=["T0", "T3", "T3M20"])
def test_a_generated_table(generated, T, M):
    d, text, accs = generated
    prefix = str(d / f"t{T}m{M}")
    args = ["--cluster", str(T)] + (["--min-compared", str(M)] if M is not None else [])
    out, err = run("dists", "-t", str(d / "table.tsv"), "-o", prefix, *args)
    want = expected(text, T, M or 1)
    got = read_files(prefix)
    assert got == want
    closing(err, prefix, 70, 40, T)
    _, _, cells = parse_table(text)
    differ, compared = matrices(cells, 40)
    _, number, roots = clusters_text(accs, differ, compared, T, M or 1)
    assert compared[0][1] == 0 and compared[2][3] == 0 and differ[0][1] == 0      # no locus in common: distance 0 ...
    assert roots[0] != roots[1] and roots[2] != roots[3]                          # ... and never linked
    comp_rows = got["compared.tsv"].splitlines()
    assert comp_rows[1].split("\t")[2] == "0" and comp_rows[3].split("\t")[4] == "0"
    clus = [l.split("\t") for l in got["clusters.tsv"].splitlines()[1:]]
    assert clus[0][1] != clus[1][1] and clus[2][1] != clus[3][1]
    assert [c[0] for c in clus] == accs and clus[0][1] == "1"
    if T == 3 and M is None:
        assert len({c[1] for c in clus[9:13]}) == 1 and int(clus[9][2]) >= 4      # the near copies of accession 9 within 3 loci
    if M == 20:
        assert all(c[3] == "-" or int(c[5]) >= 20 for c in clus)


def test_search_dists_writes_what_dists_writes_from_the_raw_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    plain_out, plain_err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "plain"))
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "sd"), "--dists", "--cluster", "0")
    assert out == plain_out
    assert read_tables(d / "sd") == read_tables(d / "plain")
    assert err.replace(str(d / "sd"), "P").startswith(plain_err.replace(str(d / "plain"), "P"))
    closing(err, str(d / "sd"), 4, 4, 0)
    run("dists", "-t", str(d / "sd.raw.tsv"), "-o", str(d / "again"), "--cluster", "0")
    got = read_files(d / "sd")
    assert sorted(got) == sorted(FILES) and got == read_files(d / "again")
    assert got == expected(open(d / "sd.raw.tsv").read(), 0)
    # Listeria_phage_B051 and Listeria_phage_B545 share locB_4: the one pair with a common call
    clus = [l.split("\t") for l in got["clusters.tsv"].splitlines()[1:]]
    assert [c[0] for c in clus] == ["Listeria_phage_B021", "Listeria_phage_B056", "Listeria_phage_B051", "Listeria_phage_B545"]
    assert [c[1] for c in clus] == ["1", "2", "3", "3"] and clus[2][3:] == ["Listeria_phage_B545", "0", "1"] and clus[1][3:] == ["-", "-", "-"]


def test_search_dists_with_max_missing_takes_the_clean_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "mm"), "--max-missing", "2", "--dists", "--cluster", "0")
    clean = open(d / "mm.clean.tsv").read()
    assert [l.split("\t")[0] for l in clean.splitlines()[1:]] == ["Listeria_phage_B021", "Listeria_phage_B545"]
    run("dists", "-t", str(d / "mm.clean.tsv"), "-o", str(d / "mm_again"), "--cluster", "0")
    got = read_files(d / "mm")
    assert sorted(got) == sorted(FILES) and got == read_files(d / "mm_again") == expected(clean, 0)


def test_an_empty_table_gives_header_only_files(tmp_path):
    (tmp_path / "empty.tsv").write_text("\t\n")
    p = subprocess.run([BIN, "dists", "-t", str(tmp_path / "empty.tsv"), "-o", str(tmp_path / "e"), "--cluster", "2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert read_files(tmp_path / "e") == {"dists.tsv": "\t\n", "compared.tsv": "\t\n",
                                          "clusters.tsv": "accession\tcluster\tsize\tnearest\tdiffer\tcompared\n"}
    closing(p.stderr, str(tmp_path / "e"), 0, 0, 2)
