#!/usr/bin/env python3
"""cid_bgzf_deflate_dev on the FASTQ text of 1 M synthetic 150-bp reads (Illumina-style headers, 41 quality letters): time of the kernels
on the ctx stream (events around the call, text and members resident), the size of the members, and zlib level 6 — what the
reference's read_filter writes with — over the same text cut into the same 65 280-byte pieces on EXP_THREADS (16) host threads.
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
rng = np.random.default_rng(1)
reads = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (R, 150))]
p = np.linspace(1, 8, 41)
qual = rng.choice(np.arange(33, 74, dtype=np.uint8), size=(R, 150), p=p / p.sum())
text = b"".join(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n" % (1101 + i // 5000, 1000 + (i * 37) % 30000, 1000 + (i * 101) % 30000) +
                reads[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n" for i in range(R))
ctx = colorid_amd.Context(0)
lib = ctx.lib
cap = lib.cid_bgzf_deflate_bound(len(text))
n = (len(text) + 65279) // 65280
d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
d_len = torch.empty(n, dtype=torch.int32, device="cuda")
d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
nm = C.c_size_t(0)
times = []
for rep in range(6):
    ctx.timer_start()
    rc = lib.cid_bgzf_deflate_dev(ctx.h, d_text.data_ptr(), len(text), d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    assert rc == 0, lib.cid_last_error()
    times.append(ctx.timer_stop_ms())
total = int(d_total.cpu()[0])
members = d_out.cpu().numpy()[:total].tobytes()
back, rest = [], members
while rest:
    d = zlib.decompressobj(31)
    back.append(d.decompress(rest)); rest = d.unused_data
assert b"".join(back) == text


def gz(i):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return len(co.compress(text[i:i + 65280]) + co.flush()) + 26


t0 = time.perf_counter()
with ThreadPoolExecutor(T) as ex:
    zsize = sum(ex.map(gz, range(0, len(text), 65280)))
zms = (time.perf_counter() - t0) * 1e3
print(json.dumps({"reads": R, "text_MB": round(len(text) / 1e6, 1), "members": n, "device_ms_first": round(times[0], 2),
                  "device_ms_later": [round(t, 2) for t in times[1:]], "device_out_MB": round(total / 1e6, 1), "device_ratio": round(len(text) / total, 3),
                  "zlib6_threads": T, "zlib6_ms": round(zms, 1), "zlib6_out_MB": round(zsize / 1e6, 1), "zlib6_ratio": round(len(text) / zsize, 3)}))
