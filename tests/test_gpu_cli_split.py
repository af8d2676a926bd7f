"""`colorid read_id|batch_id --split [--gz-matches]`: every read to the file of its label, in the classifying pass.  The bins are derived
from the run's own _reads.txt — column 2 by equality, rows whose last column is above one to `multiple_hits` — and every file must inflate
to exactly the records of its bin, in input order, as `header\\nsequence\\n+\\nquality\\n` (the restated read_filter of --taxon's tests)."""
import glob
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli import BANNER, BIN, PHAGES, REFS
from test_gpu_cli_filter import EOF_BLOCK, gunzip_all
from test_gpu_fastq import _write_bgzf, fastq_text, line_loop_records
from util import synth_fastq_records

pytestmark = pytest.mark.gpu

N_SIM = 4000                 # simulated reads of 250 bases, + the reads below: ~2.6 MB of text a file, three stretches of 1 MiB
CHIMERA, DECOY = "chimera of/B021", "decoy X"      # a '/' and spaces: both become '_' in file names
FIXED = ["no_hits", "too_short", "no_significant_hits", "multiple_hits"]
ENV = dict(COLORID_DEVICE_FASTQ_MB="1", CID_FASTQ_TIMING="1")


def colorid(*args, cwd=None, **env):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, cwd=cwd, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.startswith(BANNER)
    return p.stderr


def clean(label):
    return label.replace(" ", "_").replace("/", "_")


def bins_of(reads_txt):
    """per row of _reads.txt the label of its bin"""
    rows = [ln.split("\t") for ln in reads_txt.splitlines()]
    return ["multiple_hits" if int(r[-1]) > 1 else r[1] for r in rows], [r[1] for r in rows]


def restated(records, bins, label):
    return b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, s, q), b in zip(records, bins) if b == label)


def fasta(path, name, seq):
    with open(path, "w") as f:
        f.write(f">{name}\n" + "\n".join(seq[i:i + 70].decode() for i in range(0, len(seq), 70)) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def sample(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("split")
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    rng = np.random.default_rng(51)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    shared = genomes[0][5000:8000]                                                # a stretch two accessions hold: multiple_hits
    chimera, decoy = rand(10_000) + shared + rand(10_000), rand(20_000)
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n.replace('_', ' ')}\t{os.path.join(REFS, n + '.fasta')}\n" for n in PHAGES) +
                   f"{CHIMERA}\t{fasta(d / 'chimera.fasta', 'chimera', chimera)}\n{DECOY}\t{fasta(d / 'decoy.fasta', 'decoy', decoy)}\n")
    colorid("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / "phage"), "-r", str(tsv))
    sources = genomes + [chimera[:10_000], decoy, rand(40_000)]                   # the last: reads that hit nothing
    texts = []
    for mate in (0, 1):
        rng_m = np.random.default_rng(52)                                         # both mates from the same fragments
        recs = synth_fastq_records(rng_m, sources, N_SIM, 250, mate=mate, lower_rate=0.0)
        for i in range(500):                                                      # from the shared stretch (both mates the same read)
            a = int(rng_m.integers(0, len(shared) - 150))
            recs.append((b"shared%d/%d" % (i, mate + 1), shared[a:a + 150], b"I" * 150))
        for i in range(300):                                                      # shorter than k
            L = int(rng_m.integers(1, 27))
            recs.append((b"short%d/%d" % (i, mate + 1), genomes[1][i:i + L], b"I" * L))
        order = np.random.default_rng(53).permutation(len(recs))                  # the kinds mixed, the same way in either file
        text = fastq_text([recs[int(i)] for i in order])
        path = str(d / f"reads_{mate + 1}.fastq.gz")
        _write_bgzf(path, text, rng)
        texts.append((path, line_loop_records(text)))
    return d, str(d / "phage.bxi"), texts


def check_outputs(pre, n_files, texts, reads_txt, err):
    """the files of a --split run against the bins of its _reads.txt -> {label: [the text of each file]}"""
    bins, labels = bins_of(reads_txt)
    present = [b for b in dict.fromkeys(bins)]
    assert {"no_hits", "too_short", "multiple_hits"} <= set(present) and len(present) >= 3 + 4   # these three and several accessions have reads
    suffix = ["_R1", "_R2"] if n_files == 2 else [""]
    want_files = {f"{pre}_{clean(b)}{sfx}.fq.gz" for b in present for sfx in suffix}
    assert set(glob.glob(pre + "_*.fq.gz")) == want_files                         # a file per non-empty bin, none for an empty one
    out = {}
    for b in present:
        out[b] = []
        for f, sfx in enumerate(suffix):
            blob = open(f"{pre}_{clean(b)}{sfx}.fq.gz", "rb").read()
            assert blob[-28:] == EOF_BLOCK and len(blob) > 28
            text = gunzip_all(blob)                                               # zlib reads every member to the end of the file
            assert text == restated(texts[f][1], bins, b), (b, f)
            out[b].append(text)
    manifest = [ln.split("\t") for ln in open(pre + "_split.tsv").read().splitlines()]
    assert sorted(m[0] for m in manifest) == sorted(present) and all(len(m) == 2 + n_files for m in manifest)
    fixed = [b for b in FIXED if b in present]
    assert [m[0] for m in manifest][-len(fixed):] == fixed                        # bin order: the accessions, then the fixed bins in theirs
    for m in manifest:
        assert int(m[1]) == bins.count(m[0]) and m[2:] == [f"{pre}_{clean(m[0])}{sfx}.fq.gz" for sfx in suffix]
    assert sum(int(m[1]) for m in manifest) == len(bins)
    assert f"Wrote {len(bins)} {'read pairs' if n_files == 2 else 'reads'} to {len(present) * n_files} files" in err
    return out, bins, labels


@pytest.mark.parametrize("paired", [False, True])
def test_read_id_split_writes_every_bin(sample, tmp_path, paired):
    d, bxi, texts = sample
    files = [t[0] for t in texts[:2 if paired else 1]]
    plain = str(tmp_path / "plain")
    colorid("read_id", "-b", bxi, "-q", *files, "-n", plain, **ENV)
    pre = str(tmp_path / "dealt")
    err = colorid("read_id", "-b", bxi, "-q", *files, "-n", pre, "--split", **ENV)
    assert int(err.split("cid_fastq: ")[1].split(" steps")[0]) >= 3               # several steps: a bin's file grows step by step
    reads_txt = open(pre + "_reads.txt").read()
    assert reads_txt == open(plain + "_reads.txt").read()                         # byte for byte what the run without the flag writes
    assert open(pre + "_counts.txt").read() == open(plain + "_counts.txt").read()
    assert not glob.glob(plain + "_*.fq.gz") and not os.path.exists(plain + "_split.tsv")
    out, bins, labels = check_outputs(pre, len(files), texts, reads_txt, err)
    assert bins.count("multiple_hits") >= 300 and bins.count("too_short") >= 300 and bins.count(DECOY) > 100
    assert os.path.exists(f"{pre}_{clean(CHIMERA)}{'_R1' if paired else ''}.fq.gz")
    if not paired:
        # an accession label that no other label of the run contains: --taxon LABEL's rule (substring) then keeps the same rows
        assert not [lb for lb in set(labels) if DECOY in lb and lb != DECOY]
        tax = str(tmp_path / "one")
        colorid("read_id", "-b", bxi, "-q", *files, "-n", tax, "--taxon", DECOY, **ENV)
        assert gunzip_all(open(f"{tax}_{clean(DECOY)}.fq.gz", "rb").read()) == out[DECOY][0]


def test_split_gz_matches_writes_the_same_texts_in_fewer_bytes(sample, tmp_path):
    d, bxi, texts = sample
    size = {}
    for name, flags in (("literal", []), ("matches", ["--gz-matches"])):
        pre = str(tmp_path / name)
        err = colorid("read_id", "-b", bxi, "-q", texts[0][0], "-n", pre, "--split", *flags, **ENV)
        check_outputs(pre, 1, texts, open(pre + "_reads.txt").read(), err)
        size[name] = sum(os.path.getsize(p) for p in glob.glob(pre + "_*.fq.gz"))
    print(f"--split: {size['literal']} bytes, --split --gz-matches: {size['matches']} bytes")
    assert size["matches"] <= size["literal"]


def test_batch_id_split_writes_each_samples_files(sample, tmp_path, monkeypatch):
    d, bxi, texts = sample
    sheet = tmp_path / "samples.tsv"
    sheet.write_text(f"first\t{texts[0][0]}\nsecond\t{texts[1][0]}\t{texts[0][0]}\n")
    monkeypatch.chdir(tmp_path)                                                   # batch_id's prefixes are the samples' names: relative paths
    err = colorid("batch_id", "-b", bxi, "-q", str(sheet), "-T", "run", "--split", **ENV)
    one, two = err.split("Classifying second")
    check_outputs("first_run", 1, [texts[0]], open("first_run_reads.txt").read(), one)
    check_outputs("second_run", 2, [texts[1], texts[0]], open("second_run_reads.txt").read(), two)


def test_front_end_giving_way_leaves_no_partial_output(sample, tmp_path):
    """a refused stretch (injected through the library's switch) in the third step, when the members of the first are in the files: the
    run ends with an error and neither a .fq.gz nor the manifest is left"""
    d, bxi, texts = sample
    pre = str(tmp_path / "gone")
    p = subprocess.run([BIN, "read_id", "-b", bxi, "-q", texts[0][0], "-n", pre, "--split"], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_DEVICE_FASTQ_MB="1", CID_FASTQ_REFUSE_AT_STEP="2"))
    assert p.returncode != 0 and "--split" in p.stderr
    assert "removed the unfinished" in p.stderr                                   # files had been begun
    assert not glob.glob(pre + "_*.fq.gz") and not os.path.exists(pre + "_split.tsv")


@pytest.mark.parametrize("names", [("phage one", "phage_one"), ("no hits", "Listeria phage")])
def test_two_bins_of_one_file_name_are_refused_after_the_load(sample, tmp_path, names):
    d, bxi, texts = sample
    tsv = tmp_path / "ref_file.txt"
    tsv.write_text("".join(f"{name}\t{os.path.join(REFS, n + '.fasta')}\n" for name, n in zip(names, PHAGES)))
    colorid("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(tmp_path / "twins"), "-r", str(tsv))
    pre = str(tmp_path / "never")
    p = subprocess.run([BIN, "read_id", "-b", str(tmp_path / "twins.bxi"), "-q", texts[0][0], "-n", pre, "--split"], capture_output=True, text=True)
    assert p.returncode != 0 and "--split" in p.stderr
    other = "no_hits" if names[0] == "no hits" else names[1]
    assert f"'{names[0]}'" in p.stderr and f"'{other}'" in p.stderr               # both named
    assert not glob.glob(pre + "_*")                                              # no read file, no _reads.txt
