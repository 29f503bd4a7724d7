"""The host side of rtd_plan_request_nt / rtd_plan_get_nt under the address / undefined-behaviour sanitizers, as a stand-alone
program.

tests/cpu/nt_request_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly.  Raw, thermal and band uploads with and without a request, on plans of one window, of windows of 4
and retained.  The preparation kernels of the corrections' inputs are rtd_api.hip's own, so the stand-in runtime runs them thread
by thread on heap memory: the carve of a band's unweighted moments in the staging block, the plan's buffers with one row of the
weighted phase function per profile, what rtd_plan_get_nt copies out (by value), the refusals and their order before any
allocation, and the windows of an evaluation of raw columns -- all bounds-checked on the CPU before any of it runs on a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu")


def test_request_entry_points_are_clean_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nt_request_host")
    srcs = [os.path.join(CPU, "nt_request_host_main.cpp"), os.path.join(ROOT, "pythonic-disort_amd", "csrc", "rtd_api.hip"),
            os.path.join(CPU, "host_asan_shadow.cpp")]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wno-unused-result", "-I", os.path.join(CPU, "fake_hip"), "-x", "c++", *srcs,
                    "-o", exe, "-ldl", "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB"):
        env.pop(k, None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "NT REQUEST HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
