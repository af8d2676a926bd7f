"""CPU check of `collapse`'s plan (colorid_amd/csrc/cid_collapse.hpp, compiled with g++): a stand-alone program builds the plan for chosen
many-to-one maps — identity, reverse permutation, all into one, neighbour pairs, c mod G, groups across the borders of file words, one
group of everything but three singletons — over 1 to 300 file colours, evaluates random records through it as k_put_records_grouped does
and compares with a plain bit-by-bit loop.  Built plain and under AddressSanitizer + UBSan, and run as a child process."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_shim", "collapse_main.cpp")


# (the sanitizer runtimes are linked statically: the program's own, whatever else the process loads)
@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                                       "-static-libubsan"])])
def test_plans_agree_with_the_bit_by_bit_loop(tmp_path, name, flags):
    exe = str(tmp_path / f"collapse_main_{name}")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "collapse plan: all maps agree" in p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
