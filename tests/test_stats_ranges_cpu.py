"""csrc/stats_ranges.h, the range partition of the NIW statistics pass (range_bound, range_heads, range_owner, head_slot), checked on the
CPU: tests/tools/stats_ranges_check.cpp walks item layouts the way niw_stats_kernel writes its slabs and the way niw_reduce_kernel reads
them, and asserts that the two agree slot for slot -- every (T, groups) up to T = 48, layouts of up to 2048 mostly small or empty bins,
and item counts around 2^31 / 64 where the products need 64 bits.  Built with AddressSanitizer and UBSan where the compiler has them
(the runtime comes from the compiler's own link of that program; nothing sanitized is loaded into this process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "stats_ranges_check.cpp")


def test_writer_and_reader_agree_on_every_slot(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "stats_ranges_check")
    base = [gxx, "-std=c++17", "-O1", "-Wall", "-g", SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # (the runtimes linked statically where the compiler has them: the program then runs the same whatever else the environment preloads)
    built = subprocess.run(base + san + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        built = subprocess.run(base, capture_output=True, text=True)      # this g++ has no sanitizer runtime: the checks themselves still run
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stats_ranges_check ok" in run.stdout
