"""`colorid read_id|batch_id --taxon TAXON [--exclude]`: the reference's read_filter (src/read_filter.rs) fused into the classifying pass.
The kept set is computed from the run's own _reads.txt by the reference's rule (tab_to_map: column 2 contains the query); the
gunzipped outputs must be exactly those records, in order, as `header\\nsequence\\n+\\nquality\\n`."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from test_gpu_cli import BANNER, BIN, PHAGES, REFS
from test_gpu_fastq import _write_bgzf, fastq_text, line_loop_records
from util import synth_fastq_records

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
N_READS = 9000               # ~3 MB of text a file: three stretches of 1 MiB, so a step is filtered while the next one runs
TAXON = "phage B05"          # two of the four accessions; the space becomes '_' in the file names


def colorid(*args, cwd=None, **env):
    p = subprocess.run([BIN, *args], capture_output=True, text=True, cwd=cwd, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.startswith(BANNER)
    return p.stderr


def gunzip_all(blob):
    out, rest = [], blob
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def kept_by_the_reference_rule(reads_txt, taxon, exclude):
    rows = [ln.split("\t") for ln in reads_txt.splitlines()]
    return [(taxon in r[1]) != exclude for r in rows]


def restated(records, keep):
    return b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, s, q), k in zip(records, keep) if k)


@pytest.fixture(scope="module")
def sample(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("filter")
    tsv = d / "ref_file.txt"
    tsv.write_text("".join(f"{n.replace('_', ' ')}\t{os.path.join(REFS, n + '.fasta')}\n" for n in PHAGES))   # accession names with spaces
    colorid("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / "phage"), "-r", str(tsv))
    genomes = [b"".join(orc.read_fasta(os.path.join(REFS, n + ".fasta"))) for n in PHAGES]
    rng = np.random.default_rng(21)
    noise = [bytes(rng.choice(list(b"ACGT"), size=40_000).astype(np.uint8))]
    sources = genomes + noise * 2                                                 # a third of the reads hit nothing
    texts = []
    for mate in (0, 1):
        rng_m = np.random.default_rng(22)                                         # both mates from the same fragments
        recs = synth_fastq_records(rng_m, sources, N_READS, 150, mate=mate, lower_rate=0.0)
        text = fastq_text(recs)
        path = str(d / f"reads_{mate + 1}.fastq.gz")
        _write_bgzf(path, text, rng)
        texts.append((path, line_loop_records(text)))
    return d, str(d / "phage.bxi"), texts


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("exclude", [False, True])
def test_read_id_taxon_writes_the_kept_reads(sample, tmp_path, paired, exclude):
    d, bxi, texts = sample
    files = [t[0] for t in texts[:2 if paired else 1]]
    plain = str(tmp_path / "plain")
    colorid("read_id", "-b", bxi, "-q", *files, "-n", plain, COLORID_DEVICE_FASTQ_MB="1")
    pre = str(tmp_path / "filtered")
    err = colorid("read_id", "-b", bxi, "-q", *files, "-n", pre, "--taxon", TAXON, *(["--exclude"] if exclude else []),
                  COLORID_DEVICE_FASTQ_MB="1", CID_FASTQ_TIMING="1")              # 1 MiB stretches: several steps
    assert int(err.split("cid_fastq: ")[1].split(" steps")[0]) >= 3
    reads_txt = open(pre + "_reads.txt").read()
    assert reads_txt == open(plain + "_reads.txt").read()                         # byte for byte what the run without the flags writes
    assert open(pre + "_counts.txt").read() == open(plain + "_counts.txt").read()
    keep = kept_by_the_reference_rule(reads_txt, TAXON, exclude)
    assert len(keep) == N_READS and 0 < sum(keep) < N_READS
    names = [pre + "_phage_B05_R1.fq.gz", pre + "_phage_B05_R2.fq.gz"] if paired else [pre + "_phage_B05.fq.gz"]
    for name, (_, records) in zip(names, texts):
        blob = open(name, "rb").read()
        assert blob[-28:] == EOF_BLOCK
        assert gunzip_all(blob) == restated(records, keep), name
    assert not os.path.exists(plain + "_phage_B05.fq.gz")
    if exclude:
        assert f"Excluded {sum(keep)} read pairs  with classification containing '{TAXON}' from output files" in err
    else:
        assert f"Wrote {sum(keep)} read-pairs with classification containing '{TAXON}' to output files" in err


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("taxon,exclude", [("no such label", False), ("t", True)])
def test_a_run_that_keeps_nothing_leaves_whole_empty_files(sample, tmp_path, paired, taxon, exclude):
    """a taxon that no label contains, and --exclude of one that every label contains ("t": Listeria, no_hits, too_short,
    no_significant_hits): the files are made when the run opens them, not at a bin's first read, and hold the end-of-file block alone"""
    d, bxi, texts = sample
    files = []
    for mate, (_, records) in enumerate(texts[:2 if paired else 1]):
        files.append(str(tmp_path / f"few_{mate + 1}.fastq.gz"))
        _write_bgzf(files[-1], restated(records[:300], [1] * 300), np.random.default_rng(23))
    pre = str(tmp_path / "nothing")
    err = colorid("read_id", "-b", bxi, "-q", *files, "-n", pre, "--taxon", taxon, *(["--exclude"] if exclude else []))
    keep = kept_by_the_reference_rule(open(pre + "_reads.txt").read(), taxon, exclude)
    assert len(keep) == 300 and not any(keep)
    stem = pre + "_" + taxon.replace(" ", "_")
    for name in ([stem + "_R1.fq.gz", stem + "_R2.fq.gz"] if paired else [stem + ".fq.gz"]):
        assert open(name, "rb").read() == EOF_BLOCK, name
    if exclude:
        assert f"Excluded 0 read pairs  with classification containing '{taxon}' from output files" in err
    else:
        assert f"Wrote 0 read-pairs with classification containing '{taxon}' to output files" in err


def test_batch_id_taxon_writes_each_samples_files(sample, tmp_path):
    d, bxi, texts = sample
    sheet = tmp_path / "samples.tsv"
    sheet.write_text(f"first\t{texts[0][0]}\nsecond\t{texts[1][0]}\t{texts[0][0]}\n")
    err = colorid("batch_id", "-b", bxi, "-q", str(sheet), "-T", "run", "--taxon", TAXON, cwd=str(tmp_path))
    keep1 = kept_by_the_reference_rule(open(tmp_path / "first_run_reads.txt").read(), TAXON, False)
    keep2 = kept_by_the_reference_rule(open(tmp_path / "second_run_reads.txt").read(), TAXON, False)
    assert gunzip_all(open(tmp_path / "first_run_phage_B05.fq.gz", "rb").read()) == restated(texts[0][1], keep1)
    assert gunzip_all(open(tmp_path / "second_run_phage_B05_R1.fq.gz", "rb").read()) == restated(texts[1][1], keep2)
    assert gunzip_all(open(tmp_path / "second_run_phage_B05_R2.fq.gz", "rb").read()) == restated(texts[0][1], keep2)
    assert sum(keep1) and sum(keep2)
    assert f"Wrote {sum(keep1)} read-pairs" in err and f"Wrote {sum(keep2)} read-pairs" in err


@pytest.mark.parametrize("step", [0, 2])
def test_front_end_giving_way_leaves_no_partial_output(sample, tmp_path, step):
    """a refused stretch (injected through the library's switch) ends a --taxon run with an error, and its .fq.gz is gone:
    in the first step, when nothing has been written, and in the third, when the members of the first are in the file (a step is
    filtered after the next one was begun, so a refusal at the second still finds the file empty)"""
    d, bxi, texts = sample
    pre = str(tmp_path / "gone")
    p = subprocess.run([BIN, "read_id", "-b", bxi, "-q", texts[0][0], "-n", pre, "--taxon", TAXON], capture_output=True, text=True,
                       env=dict(os.environ, COLORID_DEVICE_FASTQ_MB="1", CID_FASTQ_REFUSE_AT_STEP=str(step)))
    assert p.returncode != 0 and "--taxon" in p.stderr
    name = pre + "_phage_B05.fq.gz"
    assert not os.path.exists(name)
    had = int(p.stderr.split(f"removed the unfinished {name} (")[1].split(" bytes")[0])
    print(f"refused at step {step}: {had} bytes had been written")
    assert (had > 0) == (step > 0)
