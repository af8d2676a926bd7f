"""`colorid search -s -m --alleles PREFIX` end to end on the four-phage index of test_gpu_cli_segments.py: stdout and stderr are those of
`-s -m` (plus one closing line on stderr), and the accessions x loci tables equal tables computed here from the oracle's perfect search,
equal what `colorid alleles -r` makes from the run's saved stdout, and are the same files on the per-record route (the group path on
one rank).  The scheme's records are cut from the genomes: a locus with one allele in one accession, an allele shared by two accessions,
two identical records of one locus (MULTI / NA), a locus whose alleles are all mutated (no column), a record shorter than k, a record
with an N, a label with a second '_', over two query files."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli_segments import BANNER, K, PHAGES, REFS, WARNING, mutate, write_fasta

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
TABLES = ("raw.tsv", "detailed.tsv", "report.out")


def run(*args, env=None):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout, p.stderr


def scheme(genomes):
    rng = np.random.default_rng(23)
    g = genomes
    shared = g[1][2450:2850]
    assert shared in g[3] and shared not in g[0] and shared not in g[2]
    # (the genome files hold 38 to 61 records each and `genomes` joins them: every cut lies inside one record)
    a = [("locA_1", g[0][3700:4200]),                                 # an allele two accessions carry, one of them with locA_7 too
         ("locA_2", mutate(rng, g[0][3700:4200], 0.03)),              # ... and an allele nobody carries
         ("locB_4", shared),                                          # an allele two accessions share
         ("locC_1", g[2][2000:2500]), ("locC_1", g[2][2000:2500]),    # the same record twice: MULTI / NA
         ("locD_1", mutate(rng, g[3][15500:16100], 0.05)), ("locD_2", mutate(rng, g[3][15500:16100], 0.05)),   # no allele found: no column
         ("locE_1", g[0][3700:3700 + K - 1])]                         # shorter than k: a warning, no row
    b = [("locF_3", g[1][3400:3800] + b"N" + g[1][3801:4200]),        # an N inside
         ("locA_7", g[2][8000:8400]),                                 # locus A again, another accession, another file
         ("locG_9_extra", g[3][15500:16000]),                         # one allele in one accession; allele = the text between the first two '_'
         ("locC_2", g[0][17000:17500])]
    return a, b


@pytest.fixture(scope="module")
def env(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_alleles")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in reversed(PHAGES)))
    run("build", "-s", "750000", "-n", "4", "-k", str(K), "-b", str(d / "phage"), "-r", str(tsv))
    oix = orc.Index.build_single(str(tsv), 750000, 4, K)
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    a, b = scheme(genomes)
    fa, fb = d / "scheme_a.fasta", d / "scheme_b.fasta"
    write_fasta(fa, a)
    write_fasta(fb, b)
    # the rows the oracle's perfect search gives, file by file, record by record
    rows, out_lines = [], []
    for f in (fa, fb):
        labels, seqs = orc.read_fasta_mf(str(f))
        for lab, s in zip(labels, seqs):
            km = orc.Kmers(K)
            if km.kmerize_string(s) != 0:
                out_lines.append(WARNING % lab.decode())
                continue
            words, missing = oix.search_perfect(km.keys())
            for c in range(len(PHAGES)):
                if not missing and words[0] >> c & 1:
                    rows.append((lab.decode(), oix.colors()[c]))
                    out_lines.append(f"{lab.decode()}\t{oix.colors()[c]}\t{len(km)}\t1.00")
    return d, str(d / "phage.bxi"), [str(fa), str(fb)], rows, out_lines


def tables(rows):
    """the three tables from (label, accession) rows, by the rules of the README: locus = label up to the first '_', allele = the text
    between the first two '_'; loci in byte order, accessions in order of their first row"""
    loci = sorted({lab.split("_")[0].encode() for lab, _ in rows})
    loci = [l.decode() for l in loci]
    accs, cells = [], {}
    for lab, acc in rows:
        if acc not in cells:
            accs.append(acc)
            cells[acc] = {}
        cells[acc].setdefault(lab.split("_")[0], []).append(lab.split("_")[1])
    header = "\t" + "\t".join(loci) + "\n"
    raw, det, rep = header, header, ""
    for acc in accs:
        r, dd = [acc], [acc]
        for l in loci:
            al = cells[acc].get(l)
            r.append(al[0] if al and len(al) == 1 else "NA")
            dd.append(al[0] if al and len(al) == 1 else ("MULTI" if al else "NOT_CALLED"))
        raw += "\t".join(r) + "\n"
        det += "\t".join(dd) + "\n"
        rep += f"{acc}; total: {len(cells[acc])}/{len(loci)}, multiple: {sum(len(v) > 1 for v in cells[acc].values())}\n"
    return {"raw.tsv": raw, "detailed.tsv": det, "report.out": rep}


def read_tables(prefix):
    return {ext: open(f"{prefix}.{ext}").read() for ext in TABLES}


def test_alleles_tables_from_one_search(env):
    d, bxi, files, rows, want_out = env
    plain_out, plain_err = run("search", "-b", bxi, "-q", *files, "-s", "-m")
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "t"))
    assert out == plain_out
    assert out[len(BANNER):].splitlines() == want_out
    closing = err.splitlines()[-1]
    assert closing.startswith("alleles: 4 accessions x 4 loci written to ")
    assert err == plain_err + closing + "\n"
    want = tables(rows)
    got = read_tables(d / "t")
    assert got == want
    # the scheme shows what it was cut for
    head = want["raw.tsv"].splitlines()[0].split("\t")
    assert head == ["", "locA", "locB", "locC", "locG"]        # locD: no allele found, locE: no k-mers, locF: the N's k-mers are in no accession
    det = [l.split("\t") for l in want["detailed.tsv"].splitlines()[1:]]
    assert det == [["Listeria_phage_B021", "1", "NOT_CALLED", "2", "NOT_CALLED"],         # accessions in order of their first row
                   ["Listeria_phage_B056", "MULTI", "NOT_CALLED", "MULTI", "NOT_CALLED"],  # locA_1 and locA_7; locC_1 twice
                   ["Listeria_phage_B051", "NOT_CALLED", "4", "NOT_CALLED", "NOT_CALLED"],
                   ["Listeria_phage_B545", "NOT_CALLED", "4", "NOT_CALLED", "9"]]           # locB_4 shared; locG_9 its own
    assert "Listeria_phage_B056\tNA\tNA\tNA\tNA\n" in want["raw.tsv"]
    assert "Listeria_phage_B056; total: 2/4, multiple: 2\n" in want["report.out"]
    assert WARNING % "locE_1" in out and not os.path.exists(d / "t.clean.tsv") and not os.path.exists(d / "t.dropped.txt")
    # the table writer alone, over this run's saved stdout (banner and warning lines included)
    (d / "saved_stdout.txt").write_text(out)
    p = subprocess.run([BIN, "alleles", "-r", str(d / "saved_stdout.txt"), "-o", str(d / "again")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert read_tables(d / "again") == want


def test_max_missing_partitions_the_accessions(env):
    d, bxi, files, rows, _ = env
    want = tables(rows)
    for n, kept in ((0, []), (2, ["Listeria_phage_B021", "Listeria_phage_B545"]), (4, sorted(PHAGES))):
        prefix = d / f"mm{n}"
        run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(prefix), "--max-missing", str(n))
        assert read_tables(prefix) == want
        clean = open(f"{prefix}.clean.tsv").read().splitlines(keepends=True)
        dropped = open(f"{prefix}.dropped.txt").read().splitlines()
        raw = want["raw.tsv"].splitlines(keepends=True)
        assert clean[0] == raw[0]
        in_clean = [l.split("\t")[0] for l in clean[1:]]
        assert sorted(in_clean) == kept and sorted(in_clean + dropped) == sorted(PHAGES)
        assert clean[1:] == [l for l in raw[1:] if l.split("\t")[0] in in_clean]
        assert dropped == [l.split("\t")[0] for l in raw[1:] if l.split("\t").count("NA") + l.split("\t").count("NA\n") > n]


def test_the_per_record_route_writes_the_same_files(env):
    """COLORID_REDUCE=host --gpus 1 is the group path on one rank: one cid_group_search_perfect call per record"""
    d, bxi, files, rows, _ = env
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "batched"))
    out_ref, err_ref = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "per_record"), "--gpus", "1",
                           env={"COLORID_REDUCE": "host"})
    announce = "1 ranks; per-accession counters are reduced through the host\n"
    assert err_ref.count(announce) == 1 and announce not in err
    assert out == out_ref
    assert err.replace(str(d / "batched"), "PREFIX") == err_ref.replace(announce, "").replace(str(d / "per_record"), "PREFIX")
    assert read_tables(d / "batched") == read_tables(d / "per_record") == tables(rows)
