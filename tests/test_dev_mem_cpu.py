"""csrc/dev_mem.h, the owners of every device and pinned buffer of the C ABI glue, checked on the CPU: tests/tools/dev_mem_check.cpp
puts counting stand-ins under the five runtime calls the header makes and is built with AddressSanitizer and UBSan (the sanitizer runtime
comes from the compiler's own link of that program; nothing sanitized is loaded into this process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "dev_mem_check.cpp")
ROCM_INCLUDE = "/opt/rocm/include"


def test_owners_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime_api.h")):
        pytest.skip("needs g++ and the HIP runtime API header")
    exe = str(tmp_path / "dev_mem_check")
    cmd = [gxx, "-std=c++17", "-Wall", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    # (the runtimes linked statically where the compiler has them: the program then runs the same whatever else the environment preloads)
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("this g++ has no AddressSanitizer / UBSan runtime")
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dev_mem_check ok" in run.stdout
