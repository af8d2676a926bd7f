"""`colorid read_id --taxon TAXON --gz-matches`: the kept reads compressed with LZ77 matches — the same reports, the same text in the
.fq.gz files as without the flag, in smaller files."""
import os

import pytest

from test_gpu_cli_filter import EOF_BLOCK, TAXON, colorid, gunzip_all, sample  # noqa: F401  (the phage index and the 9 000 read pairs)

pytestmark = pytest.mark.gpu


def test_read_id_gz_matches_writes_the_same_reads_in_smaller_files(sample, tmp_path):
    d, bxi, texts = sample
    files = [t[0] for t in texts]
    plain, lit, lz = str(tmp_path / "plain"), str(tmp_path / "lit"), str(tmp_path / "lz")
    colorid("read_id", "-b", bxi, "-q", *files, "-n", plain, COLORID_DEVICE_FASTQ_MB="1")
    colorid("read_id", "-b", bxi, "-q", *files, "-n", lit, "--taxon", TAXON, COLORID_DEVICE_FASTQ_MB="1")
    err = colorid("read_id", "-b", bxi, "-q", *files, "-n", lz, "--taxon", TAXON, "--gz-matches", COLORID_DEVICE_FASTQ_MB="1", COLORID_TIMING="1")
    assert "coder: LZ77 matches (--gz-matches)" in err
    for tail in ("_reads.txt", "_counts.txt"):
        assert open(lz + tail, "rb").read() == open(plain + tail, "rb").read()     # byte for byte what the run without the flags writes
    for tail in ("_phage_B05_R1.fq.gz", "_phage_B05_R2.fq.gz"):
        a, b = open(lit + tail, "rb").read(), open(lz + tail, "rb").read()
        assert b[-28:] == EOF_BLOCK
        text = gunzip_all(b)
        assert text and text == gunzip_all(a)
        print(f"{tail}: {len(text)} bytes of reads, {len(a)} without matches, {len(b)} with")
        assert len(b) < len(a)
    assert "Wrote " in err and f"containing '{TAXON}' to output files" in err
    assert not os.path.exists(plain + "_phage_B05_R1.fq.gz")
