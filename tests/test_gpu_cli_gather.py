"""`colorid search --gather PREFIX`: PREFIX.gather.tsv against the table restated from tests/gather_ref.py over the oracle's k-mers
(kmers_from_fq_qual / kmers_fq_pe_qual / kmerize_vector, cleaned with the cut-off the run used) and the oracle's index: P[k] is the
oracle's perfect search of k-mer k alone.  Integer columns must be equal, printed decimals within one unit of their last digit; stdout
must be byte for byte what the run without the flag prints.

The sample: 2 000 reads (pairs) of 150 bases drawn from the first 12 kb of two of the four phages and from random sequence."""
import os
import subprocess

import numpy as np
import pytest

import gather_ref
from test_gpu_cli import BANNER, BIN, PHAGES, REFS
from util import synth_fastq_records, write_fastq_gz

pytestmark = pytest.mark.gpu

HEADER = "query\trank\taccession\tnew_kmers\tnew_share\tnew_depth\ttotal_kmers\tgenome_cov\ttotal_depth\tlive_before\texpected_false"
K, M, N_HASH = 27, 750000, 4
N_READS = 2000


def colorid(*args, **env):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.startswith(BANNER)
    return p.stdout, p.stderr


@pytest.fixture(scope="module")
def sample(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("gather")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in PHAGES))
    colorid("build", "-s", str(M), "-n", str(N_HASH), "-k", str(K), "-b", str(d / "phage"), "-r", str(tsv))
    oix = orc.Index.build_single(str(tsv), M, N_HASH, K)
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    rng = np.random.default_rng(41)
    noise = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 8000)])
    sources = [genomes[2][:12000], genomes[0][:12000], noise]
    files = []
    for mate in (0, 1):
        rng_m = np.random.default_rng(42)                                         # both mates from the same fragments
        recs = synth_fastq_records(rng_m, sources, N_READS, 150, mate=mate, err=0.003, lower_rate=0.0)
        files.append(str(d / f"reads_{mate + 1}.fastq.gz"))
        write_fastq_gz(files[-1], recs)
    fasta = str(d / "chimera.fasta")
    with open(fasta, "wb") as f:
        f.write(b">a\n" + genomes[2][:9000] + b"\n>b\n" + genomes[3][2000:9000] + b"\n>c\n" + noise[:3000] + b"\n")
    return d, str(d / "phage.bxi"), oix, files, fasta


_P = {}


def bits(oix, km):
    """P[k] for the k-mers of an oracle map; a k-mer's row is computed once per session"""
    keys = km.keys()
    P = np.zeros((len(keys), oix.n_colors), bool)
    for i in range(len(keys)):
        b = keys[i].tobytes()
        if b not in _P:
            _P[b] = np.unpackbits(oix.search_perfect(keys[i:i + 1])[0].view(np.uint8), bitorder="little")[:oix.n_colors].astype(bool)
        P[i] = _P[b]
    return P


def restated(orc, oix, query, km, min_new=1, max_rows=None):
    """the block of `query` as lists of fields: ints, floats, or strings"""
    P, freq, n = bits(oix, km), km.counts(), len(km)
    rows, n_hit, _ = gather_ref.gather(P, freq, min_new, max_rows)
    names, n_ref = oix.colors(), oix.n_ref_kmers()
    out = []
    for r, g in enumerate(rows):
        c = g["colour"]
        out.append([query, r + 1, names[c], g["new_kmers"], g["new_kmers"] / n, g["new_weight"] / g["new_kmers"], g["total_kmers"],
                    g["total_kmers"] / n_ref[c], g["total_weight"] / g["total_kmers"], g["live_before"],
                    g["live_before"] * orc.false_prob(M, N_HASH, n_ref[c])])
    left = n - sum(g["new_kmers"] for g in rows)
    out.append([query, "-", "unexplained", left, left / n, "-", n_hit, n_hit / n, "-", left, "-"])
    return out


DIGITS = {4: 4, 5: 2, 7: 2, 8: 2, 10: 1}    # column -> printed decimals


def assert_block(lines, want):
    assert len(lines) == len(want), f"{len(lines)} lines, want {len(want)}:\n" + "\n".join(lines[:8])
    for ln, w in zip(lines, want):
        got = ln.split("\t")
        assert len(got) == 11, ln
        for j, (g, x) in enumerate(zip(got, w)):
            if isinstance(x, float):
                d = DIGITS[j]
                assert len(g.split(".")[1]) == d, (ln, j)
                assert abs(float(g) - x) <= 10.0 ** -d * (1 + 1e-9), (ln, j, x)     # one unit of the last printed digit
            else:
                assert g == str(x), (ln, j, x)


def blocks(path):
    """{query: its lines} of a .gather.tsv, in file order"""
    lines = open(path).read().splitlines()
    assert lines[0] == HEADER
    out = {}
    for ln in lines[1:]:
        out.setdefault(ln.split("\t")[0], []).append(ln)
    return out


def check_adds_up(lines):
    rows = [ln.split("\t") for ln in lines]
    assert rows[-1][1] == "-" and rows[-1][2] == "unexplained" and all(r[1] == str(i + 1) for i, r in enumerate(rows[:-1]))
    first_live = int(rows[0][9])
    assert first_live - sum(int(r[3]) for r in rows[:-1]) == int(rows[-1][3])
    for a, b in zip(rows[:-2], rows[1:-1]):
        assert int(a[9]) - int(a[3]) == int(b[9])                                  # live_before runs down by what each row takes


@pytest.mark.parametrize("mode", ["se_f2", "pe_f0"])
def test_reads(orc, sample, tmp_path, mode):
    d, bxi, oix, files, _ = sample
    pe = mode.startswith("pe")
    cutoff = 2 if mode == "se_f2" else 0
    km = (orc.kmers_fq_pe_qual(files[0], files[1], K, 15) if pe else orc.kmers_from_fq_qual(files[0], K, 15)).clean_map(cutoff)
    args = ["search", "-b", bxi, "-q", files[0]] + (["-r", files[1]] if pe else []) + ["-f", str(cutoff), "-p", "0.02"]
    plain, _ = colorid(*args)
    pre = str(tmp_path / "cover")
    out, err = colorid(*args, "--gather", pre, "--gather-min", "1", COLORID_TIMING="1")
    assert out == plain and len(plain) > len(BANNER)                               # stdout: byte for byte the run without the flag
    assert "timing: --gather:" in err
    got = blocks(pre + ".gather.tsv")
    want = restated(orc, oix, files[0], km)
    assert list(got) == [files[0]] and len(want) >= 3                              # two phages and the line of the rest, at the least
    assert_block(got[files[0]], want)
    check_adds_up(got[files[0]])
    assert int(got[files[0]][0].split("\t")[9]) == len(km)
    # the k-mer map on the host: cid_search_gather instead of cid_search_gather_set, the same file
    host = str(tmp_path / "host")
    out, err = colorid(*args, "--gather", host, "--gather-min", "1", COLORID_HOST_KMERS="1")
    assert out == plain and "k-mer map on the host" in err
    assert open(host + ".gather.tsv").read() == open(pre + ".gather.tsv").read()


def test_fasta_query_and_two_files_in_one_table(orc, sample, tmp_path):
    d, bxi, oix, files, fasta = sample
    kf = orc.Kmers(K)
    for s in orc.read_fasta(fasta):
        kf.kmerize_vector(s, 1)
    kf = kf.clean_map(max(kf.auto_cutoff(), 0))
    kr = orc.kmers_from_fq_qual(files[1], K, 15)
    kr = kr.clean_map(max(kr.auto_cutoff(), 0))
    pre = str(tmp_path / "two")
    plain, _ = colorid("search", "-b", bxi, "-q", fasta, files[1], "-p", "0.02")
    out, _ = colorid("search", "-b", bxi, "-q", fasta, files[1], "-p", "0.02", "--gather", pre, "--gather-min", "1")
    assert out == plain
    got = blocks(pre + ".gather.tsv")
    assert list(got) == [fasta, files[1]]                                          # two blocks, in the order of the queries
    assert_block(got[fasta], restated(orc, oix, fasta, kf))
    assert_block(got[files[1]], restated(orc, oix, files[1], kr))
    for q in got:
        check_adds_up(got[q])
    # the chimera holds 9 000 bases of one phage and 7 000 of another: both are listed, each with what it adds
    names = [ln.split("\t")[2] for ln in got[fasta]]
    assert PHAGES[2] in names and PHAGES[3] in names


def test_defaults_and_the_cap(orc, sample, tmp_path):
    """--gather-min defaults to 1000, --gather-max to the number of accessions; --gather-max 1 ends the table after its first row"""
    d, bxi, oix, files, _ = sample
    km = orc.kmers_from_fq_qual(files[0], K, 15).clean_map(2)
    pre = str(tmp_path / "dflt")
    colorid("search", "-b", bxi, "-q", files[0], "-f", "2", "--gather", pre)
    want = restated(orc, oix, files[0], km, 1000)
    assert_block(blocks(pre + ".gather.tsv")[files[0]], want)
    assert all(w[3] >= 1000 for w in want[:-1]) and len(want) < len(restated(orc, oix, files[0], km))
    colorid("search", "-b", bxi, "-q", files[0], "-f", "2", "--gather", pre, "--gather-min", "1", "--gather-max", "1")
    got = blocks(pre + ".gather.tsv")[files[0]]                                    # the file of the earlier run is replaced, not appended to
    assert_block(got, restated(orc, oix, files[0], km, 1, 1))
    assert len(got) == 2
