"""`colorid search -g -m` and `-s -m` end to end: every record of a multi-FASTA is its own query.  -g -m (a batch of records is one
cid_search_segments call) prints, record by record, the rows `search -g` prints for a file holding that record alone (label in place
of the file name); -s -m prints what the group path's one call per record prints, byte for byte, whichever route it takes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
REFS = os.path.join(HERE, "golden", "refs")
PHAGES = ["Listeria_phage_B021", "Listeria_phage_B051", "Listeria_phage_B056", "Listeria_phage_B545"]
BANNER = "\n ************** initializing logger *****************\n\n"
K = 27
ACGT = np.frombuffer(b"ACGT", np.uint8)
WARNING = "Warning! no kmers in query '%s'; maybe your kmer length is larger than your query length?"


def run(*args, env=None):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout[len(BANNER):], p.stderr


@pytest.fixture(scope="module")
def env(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_segments")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in reversed(PHAGES)))
    run("build", "-s", "750000", "-n", "4", "-k", str(K), "-b", str(d / "phage"), "-r", str(tsv))
    oix = orc.Index.build_single(str(tsv), 750000, 4, K)
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    return d, str(d / "phage.bxi"), oix, genomes


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, np.uint8).copy()
    e = rng.random(len(a)) < rate
    a[e] = ACGT[rng.integers(0, 4, int(e.sum()))]
    return a.tobytes()


def write_fasta(path, records):
    with open(path, "wb") as f:
        for label, seq in records:
            f.write(b">" + label.encode() + b"\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + b"\n")


def gene_records(rng, genomes):
    recs = []
    for i, (g, start, n) in enumerate([(0, 100, 900), (1, 5000, 1500), (2, 20, 300), (3, 7000, 2000), (0, 12000, 64 + K - 1), (2, 9000, 65 + K - 1),
                                       (1, 300, 650), (3, 100, 1200)]):
        recs.append((f"cut{i}_g{g}", genomes[g][start:start + n]))
    recs.append(("subst_2pc", mutate(rng, genomes[1][2000:3000], 0.02)))
    recs.append(("subst_10pc", mutate(rng, genomes[3][4000:4800], 0.10)))
    recs.append(("exactly_k", genomes[2][500:500 + K]))
    recs.append(("from_no_genome", ACGT[rng.integers(0, 4, 700)].tobytes()))
    return recs


def gene_rows(orc, oix, label, seq, cov):
    """what `search -g` prints for a file holding this record alone, with the label as the query name (reports.rs:50-62)"""
    km = orc.Kmers(K)
    km.kmerize_vector(seq, 1)
    if len(km) == 0:
        return []
    hits = oix.search_count(km.keys(), km.counts())[0]
    return oix.generate_report_gene(label, hits, len(km), cov).splitlines()


def rows_by_label(out, labels):
    """stdout rows grouped by their first field; the groups must come in the order of `labels`"""
    groups, order = {}, []
    for line in out.splitlines():
        q = line.split("\t")[0]
        assert len(line.split("\t")) == 4, line
        if q not in groups:
            groups[q] = []
            order.append(q)
        else:
            assert order[-1] == q, "rows of one record are not contiguous"
        groups[q].append(line)
    assert order == [l for l in labels if l in groups]
    return groups


def test_gene_search_per_record_equals_one_search_per_record(orc, env):
    d, bxi, oix, genomes = env
    recs = gene_records(np.random.default_rng(5), genomes)
    mf = d / "panel.fasta"
    write_fasta(mf, recs)
    out, err = run("search", "-b", bxi, "-q", str(mf), "-g", "-m", "-p", "0.05")
    got = rows_by_label(out, [l for l, _ in recs])
    n_rows = 0
    for i, (label, seq) in enumerate(recs):
        one = d / f"one_{i}.fasta"
        write_fasta(one, [(label, seq)])
        single, _ = run("search", "-b", bxi, "-q", str(one), "-g", "-p", "0.05")
        want = ["\t".join([label] + line.split("\t")[1:]) for line in single.splitlines()]
        assert all(line.split("\t")[0] == str(one) for line in single.splitlines())
        assert got.get(label, []) == want, label
        assert want == gene_rows(orc, oix, label, seq, 0.05), label
        n_rows += len(want)
    assert n_rows >= len(recs) - 2 and "from_no_genome" not in got and len(got["exactly_k"]) >= 1
    assert got["exactly_k"][0].split("\t")[2:] == ["1", "1.000"]
    # the same file under plain -g is ONE query: the records' k-mers pooled
    pooled, _ = run("search", "-b", bxi, "-q", str(mf), "-g", "-p", "0.05")
    assert pooled.splitlines() and all(line.split("\t")[0] == str(mf) for line in pooled.splitlines())
    assert pooled.splitlines() != out.splitlines()
    assert WARNING[:20] not in err and WARNING[:20] not in out


def test_gene_search_records_without_kmers(orc, env):
    d, bxi, oix, genomes = env
    recs = [("first", genomes[0][50:400]), ("too_short", genomes[1][10:10 + K - 1]), ("all_n", b"N" * 200), ("last", genomes[3][900:1300])]
    for label in ("too_short", "all_n"):
        assert gene_rows(orc, oix, label, dict(recs)[label], 0.05) == []
    mf = d / "holes.fasta"
    write_fasta(mf, recs)
    out, err = run("search", "-b", bxi, "-q", str(mf), "-g", "-m", "-p", "0.05")
    got = rows_by_label(out, [l for l, _ in recs])
    assert sorted(got) == ["first", "last"]
    for label, seq in recs:
        assert got.get(label, []) == gene_rows(orc, oix, label, seq, 0.05)
    warned = [line for line in err.splitlines() if line.startswith("Warning!")]
    assert warned == [WARNING % "too_short", WARNING % "all_n"]


def test_gene_search_two_query_files_keep_their_order(orc, env):
    d, bxi, oix, genomes = env
    a = [("a0", genomes[2][100:700]), ("a1", genomes[0][3000:3500])]
    b = [("b0", genomes[1][100:900]), ("b1", genomes[2][4000:4300]), ("b2", genomes[3][10:500])]
    fa, fb = d / "two_a.fasta", d / "two_b.fasta"
    write_fasta(fa, a)
    write_fasta(fb, b)
    out, _ = run("search", "-b", bxi, "-q", str(fb), str(fa), "-g", "-m", "-p", "0.05")
    want = [row for label, seq in b + a for row in gene_rows(orc, oix, label, seq, 0.05)]
    assert out.splitlines() == want and len({r.split("\t")[0] for r in want}) == 5


def test_perfect_multifasta_is_byte_identical_to_the_per_record_path(orc, env):
    """`--gpus 1` with COLORID_REDUCE=host is the group path on one rank, which makes one cid_group_search_perfect call per record
    (the variable alone, without a device list, leaves a run on its one context: that run is compared too).  The group run
    announces itself with one stderr line of its own; apart from that line both streams are equal byte for byte."""
    d, bxi, oix, genomes = env
    rng = np.random.default_rng(11)
    recs = []
    for i in range(34):
        g = int(rng.integers(0, 4))
        st, n = int(rng.integers(0, len(genomes[g]) - 2500)), int(rng.integers(K, 2400))
        seq = genomes[g][st:st + n]
        if i % 5 == 4:
            seq = mutate(rng, seq, 0.01)     # some alleles that are in no accession
        recs.append((f"allele_{i}", seq))
    recs.insert(3, ("shorter_than_k", genomes[0][5:5 + K - 1]))
    recs.insert(9, ("with_an_n", genomes[1][1000:1400] + b"N" + genomes[1][1401:1800]))
    recs += [("dup_a", recs[0][1]), ("dup_b", recs[0][1]), ("dup_c", recs[0][1])]
    recs.append(("from_no_genome", ACGT[rng.integers(0, 4, 500)].tobytes()))
    mf = d / "alleles.fasta"
    write_fasta(mf, recs)
    args = ("search", "-b", bxi, "-q", str(mf), "-s", "-m")
    out, err = run(*args)
    assert (out, err) == run(*args, env={"COLORID_REDUCE": "host"})
    out_ref, err_ref = run(*args, "--gpus", "1", env={"COLORID_REDUCE": "host"})
    announce = "1 ranks; per-accession counters are reduced through the host\n"
    assert err_ref.count(announce) == 1 and announce not in err
    assert out == out_ref
    assert err == err_ref.replace(announce, "")
    labels, seqs = orc.read_fasta_mf(str(mf))
    assert len(labels) == len(recs) == 40
    want, want_err = [], []
    for lab, s in zip(labels, seqs):
        km = orc.Kmers(K)
        if km.kmerize_string(s) != 0:
            want.append(WARNING % lab.decode())
            continue
        want_err.append(f"{len(km)} kmers in query")
        words, missing = oix.search_perfect(km.keys())
        if missing:
            want_err.append("No perfect hits!")
            continue
        rows = [f"{lab.decode()}\t{oix.colors()[c]}\t{len(km)}\t1.00" for c in range(4) if words[0] >> c & 1]
        want_err.append(f"{len(rows)} hits")
        want += rows
    assert out.splitlines() == want
    assert [l for l in err.splitlines() if l.endswith("kmers in query") or l.endswith(" hits") or l == "No perfect hits!"] == want_err
    assert "No perfect hits!" in want_err and any(w.endswith("\t1.00") for w in want) and WARNING % "shorter_than_k" in want
