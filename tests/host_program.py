"""Shared recipe of the stand-alone host programs (tests/cpu/*_host_main.cpp): the program is compiled together with
csrc/rtd_api.hip (as it is) and the shadow launchers of tests/cpu/host_asan_shadow.cpp against the stand-in runtime of
tests/cpu/fake_hip, with the address / undefined-behaviour sanitizer runtimes linked in statically, and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu")
API = os.path.join(ROOT, "pythonic-disort_amd", "csrc", "rtd_api.hip")


def build(tmp_path, main, name, defines=(), api=API):
    """Compiles tests/cpu/<main> + rtd_api.hip + the shadow launchers into tmp_path/<name>; skips the test without g++."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    srcs = [os.path.join(CPU, main), api, os.path.join(CPU, "host_asan_shadow.cpp")]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wno-unused-result", *["-D" + d for d in defines],
                    "-I", os.path.join(CPU, "fake_hip"), "-x", "c++", *srcs, "-o", exe, "-ldl", "-lpthread"], check=True)
    return exe


def build_trace_library(tmp_path, name="librtd_trace.so"):
    """rtd_api.hip + the shadow launchers as a plain shared library that logs its runtime calls (-DFAKE_HIP_TRACE) and that the
    Python front end loads through RTD_LIB; no sanitizer, so a Python process needs nothing preloaded.  Skips the test without g++."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    lib = str(tmp_path / name)
    subprocess.run([gxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-Wno-unused-result", "-DFAKE_HIP_TRACE", "-I", os.path.join(CPU, "fake_hip"),
                    "-x", "c++", API, os.path.join(CPU, "host_asan_shadow.cpp"), "-o", lib, "-ldl", "-lpthread"], check=True)
    return lib


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB"):
        env.pop(k, None)
    return subprocess.run([exe, *args], env=env, capture_output=True, text=True, timeout=600)


def build_and_run(tmp_path, main, name):
    return run(build(tmp_path, main, name))
