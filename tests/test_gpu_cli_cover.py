"""`colorid search -g -m --coverage` end to end on the phage index of test_gpu_cli_segments.py: the rows and the first four columns are
those of `-g -m` on the same file, byte for byte and in the same order; the five appended columns are what tests/cover_ref.py gives from
the oracle index's bits, window by window."""
import os
import subprocess

import numpy as np
import pytest

import cover_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
REFS = os.path.join(HERE, "golden", "refs")
PHAGES = ["Listeria_phage_B021", "Listeria_phage_B051", "Listeria_phage_B056", "Listeria_phage_B545"]
BANNER = "\n ************** initializing logger *****************\n\n"
K = 27
COV = 0.05
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
WARNING = "Warning! no kmers in query '%s'; maybe your kmer length is larger than your query length?"


def run(*args, ok=True):
    p = subprocess.run([BIN, *args], capture_output=True, text=True)
    assert (p.returncode == 0) == ok, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout[len(BANNER):], p.stderr


def write_fasta(path, records):
    with open(path, "wb") as f:
        for label, seq in records:
            f.write(b">" + label.encode() + b"\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + b"\n")


@pytest.fixture(scope="module")
def env(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_cover")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in reversed(PHAGES)))
    run("build", "-s", "750000", "-n", "4", "-k", str(K), "-b", str(d / "phage"), "-r", str(tsv))
    oix = orc.Index.build_single(str(tsv), 750000, 4, K)
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    return d, str(d / "phage.bxi"), oix, genomes


def panel(rng, genomes):
    g = genomes
    sub = bytearray(g[2][2000:3000])
    sub[500] = ord("A") if sub[500] != ord("A") else ord("C")          # one substitution in the middle: k windows lose their k-mer
    return [("cut0_g0", g[0][100:1000]), ("cut1_g1", g[1][5000:6500]),
            ("one_substitution_g2", bytes(sub)),
            ("half_gene_g3", g[3][7000:7600] + ACGT[rng.integers(0, 4, 600)].tobytes()),
            ("with_nnn_g0", g[0][3000:3400] + b"NNN" + g[0][3400:3900]),
            ("duplication_g1", g[1][800:1400] + g[1][1000:1200] + g[1][1400:1800]),
            ("exactly_k", g[2][500:500 + K]),
            ("shorter_than_k", g[0][5:5 + K - 1]),
            ("from_no_genome", ACGT[rng.integers(0, 4, 700)].tobytes())]


def reference_cells(oix, seq):
    """(distinct k-mers, cover_ref cells [C]) of one record: its windows in order, the canonical upper-case k-mer of each, a window with a
    non-ACGT base invalid, FIRST through the record's own set, P from the oracle's perfect search of the window's k-mer alone"""
    L = max(0, len(seq) - K + 1)
    C = oix.n_colors
    P, first, seen = np.zeros((L, C), bool), np.zeros(L, bool), set()
    for w in range(L):
        fwd = seq[w:w + K]
        if any(b not in b"ACGTacgt" for b in fwd):
            continue
        rc = fwd.translate(COMP)[::-1]
        km = min(fwd, rc).upper()
        first[w] = km not in seen
        seen.add(km)
        words = oix.search_perfect(np.frombuffer(km, np.uint8).reshape(1, K))[0]
        P[w] = np.unpackbits(words.view(np.uint8), bitorder="little")[:C]
    return len(seen), cover_ref.cover(P, first, K)


def wanted_tail(cell, length):
    return ["%.3f" % (int(cell["bases_covered"]) / length), str(int(cell["longest_run"]) + K - 1), str(int(cell["n_runs"])),
            str(int(cell["first_window"]) + 1), str(int(cell["last_window"]) + K)]


def test_coverage_columns(orc, env):
    d, bxi, oix, genomes = env
    recs = panel(np.random.default_rng(23), genomes)
    mf = d / "panel.fasta"
    write_fasta(mf, recs)
    plain, plain_err = run("search", "-b", bxi, "-q", str(mf), "-g", "-m", "-p", str(COV))
    out, err = run("search", "-b", bxi, "-q", str(mf), "-g", "-m", "--coverage", "-p", str(COV))
    rows = [line.split("\t") for line in out.splitlines()]
    assert all(len(r) == 9 for r in rows) and len(rows) >= 7
    # columns 1-4: the rows of -g -m, byte for byte, in the same order
    assert ["\t".join(r[:4]) for r in rows] == plain.splitlines()
    warned = [line for line in err.splitlines() if line.startswith("Warning!")]
    assert warned == [WARNING % "shorter_than_k"] == [line for line in plain_err.splitlines() if line.startswith("Warning!")]
    # columns 5-9 from the oracle's bits
    colours = oix.colors()
    want, cells = [], {}
    for label, seq in recs:
        n_kmers, cell = reference_cells(oix, seq)
        cells[label] = cell
        for c in range(len(colours)):
            h = int(cell["kmers_hit"][c])
            if n_kmers and h and h / n_kmers >= COV:
                want.append([label, colours[c], str(n_kmers), "%.3f" % (h / n_kmers)] + wanted_tail(cell[c], len(seq)))
    assert rows == want
    by = {(r[0], r[1]): r for r in rows}
    own = lambda label, g: by[(label, PHAGES[g])]
    # a record of exactly k bases is one window: covered from base 1 to base k in one stretch.  (The longer cuts are NOT one stretch in
    # this index — the oracle's bits say so too, the build drops some of the genomes' k-mers — so they are held to the reference above.)
    assert own("exactly_k", 2)[2:] == ["1", "1.000", "1.000", str(K), "1", "1", str(K)]
    assert float(own("cut0_g0", 0)[4]) > 0.9 and float(own("cut1_g1", 1)[4]) > 0.9
    # one substitution: the k windows over it are gone, two stretches remain, and of the record's bases exactly one is uncovered
    c = cells["one_substitution_g2"][PHAGES.index("Listeria_phage_B056")]
    assert (int(c["n_runs"]), int(c["windows_hit"]), int(c["bases_covered"])) == (2, 1000 - K + 1 - K, 999)
    assert own("one_substitution_g2", 2)[4:] == ["0.999", "500", "2", "1", "1000"]
    # half a gene: the first 600 bases and nothing behind them
    r = own("half_gene_g3", 3)
    assert r[4] == "0.500" and r[7:] == ["1", "600"]
    # NNN in the middle: the windows over it are invalid and break the run; the record is covered up to its last base all the same
    r = own("with_nnn_g0", 0)
    assert int(r[6]) >= 2 and r[8] == "903" and int(cells["with_nnn_g0"]["windows_hit"].max()) <= 903 - K + 1 - (K + 2)
    # a duplication: 200 windows repeat earlier k-mers, so the k-mer share counts fewer k-mers than the record has windows
    n_kmers, cell = reference_cells(oix, dict(recs)["duplication_g1"])
    c1 = cell[PHAGES.index("Listeria_phage_B051")]
    assert n_kmers < 1200 - K + 1 and int(c1["kmers_hit"]) < int(c1["windows_hit"])
    assert "from_no_genome" not in {r[0] for r in rows}


def test_an_index_of_more_than_8192_accessions_is_refused_after_the_load(orc, env):
    d = env[0]
    wide = orc.Index(1009, 1, K, 8193)
    for c in range(8193):
        wide.set_color(c, f"acc_{c:05d}", 1)
    wide.insert(7, b"ACGTACGTACGTACGTACGTACGTACG")
    wide.save(str(d / "wide.bxi"))
    mf = d / "one.fasta"
    write_fasta(mf, [("r", b"ACGTACGTACGTACGTACGTACGTACGTTTGACA")])
    out, err = run("search", "-b", str(d / "wide.bxi"), "-q", str(mf), "-g", "-m", "--coverage", ok=False)
    assert out == "" and "Index loaded" in err and "--coverage serves indices of at most 8192 accessions" in err and "8193" in err
