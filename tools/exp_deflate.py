#!/usr/bin/env python3
"""The device BGZF compressor four ways on the FASTQ text of EXP_READS (1 M) synthetic 150-bp reads with Illumina-style headers, once with
41 quality letters (the worst case for matches) and once with 4 binned ones (EXP_QUALS=both | 41 | binned):
  literals only   cid_bgzf_deflate_dev            time of the kernels on the ctx stream (events around the call, text and members resident)
  with matches    cid_bgzf_deflate_lz_dev         the same
  zlib level 1, zlib level 6 (what the reference's read_filter writes with)   over the same text cut into the same 65 280-byte pieces,
                                                  on EXP_THREADS (16) host threads
and the size of the members each way (zlib's raw streams + the 26 bytes of a member's header and trailer).  One JSON line per text.
Kernel by kernel: run under rocprofv3 --kernel-trace --stats."""
import ctypes as C, json, os, sys, time, zlib
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import colorid_amd

R = int(os.environ.get("EXP_READS", 1_000_000))
T = int(os.environ.get("EXP_THREADS", 16))
QUALS = os.environ.get("EXP_QUALS", "both")
REPS = 6
ctx = colorid_amd.Context(0)
lib = ctx.lib


def make_text(binned):
    rng = np.random.default_rng(1)
    reads = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (R, 150))]
    if binned:
        qual = np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, size=(R, 150), p=[0.9, 0.06, 0.03, 0.01])]
    else:
        p = np.linspace(1, 8, 41)
        qual = rng.choice(np.arange(33, 74, dtype=np.uint8), size=(R, 150), p=p / p.sum())
    return b"".join(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n" % (1101 + i // 5000, 1000 + (i * 37) % 30000, 1000 + (i * 101) % 30000) +
                    reads[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n" for i in range(R))


def device(fn, text, d_text):
    """-> (ms of the first call, ms of the later ones, bytes of the members); the members read back by zlib"""
    cap = lib.cid_bgzf_deflate_bound(len(text))
    n = (len(text) + 65279) // 65280
    d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(n, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nm = C.c_size_t(0)
    times = []
    for rep in range(REPS):
        ctx.timer_start()
        rc = fn(ctx.h, d_text.data_ptr(), len(text), d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
        assert rc == 0, lib.cid_last_error()
        times.append(ctx.timer_stop_ms())
    total = int(d_total.cpu()[0])
    members = d_out.cpu().numpy()[:total].tobytes()
    back, rest = [], members
    while rest:
        d = zlib.decompressobj(31)
        back.append(d.decompress(rest)); rest = d.unused_data
    assert b"".join(back) == text
    return round(times[0], 2), [round(t, 2) for t in times[1:]], total


def host(text, level):
    def gz(i):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(co.compress(text[i:i + 65280]) + co.flush()) + 26

    t0 = time.perf_counter()
    with ThreadPoolExecutor(T) as ex:
        size = sum(ex.map(gz, range(0, len(text), 65280)))
    return round((time.perf_counter() - t0) * 1e3, 1), size


for binned in {"both": (False, True), "41": (False,), "binned": (True,)}[QUALS]:
    text = make_text(binned)
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    out = {"qualities": "4 binned" if binned else "41 letters", "reads": R, "text_MB": round(len(text) / 1e6, 1), "members": (len(text) + 65279) // 65280}
    for name, fn in (("literals", lib.cid_bgzf_deflate_dev), ("matches", lib.cid_bgzf_deflate_lz_dev)):
        first, later, size = device(fn, text, d_text)
        out.update({f"{name}_ms_first": first, f"{name}_ms_later": later, f"{name}_out_MB": round(size / 1e6, 2), f"{name}_ratio": round(len(text) / size, 3)})
        sizes = dict(out.get("_sizes", {}), **{name: size}); out["_sizes"] = sizes
    for level in (1, 6):
        ms, size = host(text, level)
        out.update({f"zlib{level}_threads": T, f"zlib{level}_ms": ms, f"zlib{level}_out_MB": round(size / 1e6, 2), f"zlib{level}_ratio": round(len(text) / size, 3)})
        out["_sizes"][f"zlib{level}"] = size
    s = out.pop("_sizes")
    # the share of zlib's saving over the literal-only members that the matches achieve
    out["share_of_zlib1_saving"] = round((s["literals"] - s["matches"]) / (s["literals"] - s["zlib1"]), 3)
    out["share_of_zlib6_saving"] = round((s["literals"] - s["matches"]) / (s["literals"] - s["zlib6"]), 3)
    print(json.dumps(out), flush=True)
    del d_text
