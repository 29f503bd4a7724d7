"""The host side of the actinic-flux entry points under the address / undefined-behaviour sanitizers, as a stand-alone program.

tests/cpu/actinic_host_main.cpp is compiled together with csrc/rtd_api.hip (as it is) and the shadow launchers of
tests/cpu/host_asan_shadow.cpp against the stand-in runtime of tests/cpu/fake_hip, with the sanitizer runtimes linked in
statically, and run directly.  rtd_actinic_kernel and rtd_band_reduce_kernel are rtd_api.hip's own, so the stand-in runtime runs
them thread by thread on heap memory: rtd_plan_fetch_actinic and rtd_plan_fetch_band_actinic after run, run_fetch, evaluate and
evaluate_band, in all three tau-orders, every output pointer NULL in turn, windows of 4 over 15 columns in groups of 5, a plan
without a beam, the lazily grown buffers, every RTD_ERR_STATE case -- all bounds-checked on the CPU, and every element recomputed
in long double from the u0 fetched from the same plan, before any of it runs on a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = os.path.join(ROOT, "tests", "cpu")


def test_actinic_entry_points_are_clean_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "actinic_host")
    srcs = [os.path.join(CPU, "actinic_host_main.cpp"), os.path.join(ROOT, "pythonic-disort_amd", "csrc", "rtd_api.hip"),
            os.path.join(CPU, "host_asan_shadow.cpp")]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wno-unused-result", "-I", os.path.join(CPU, "fake_hip"), "-x", "c++", *srcs,
                    "-o", exe, "-ldl", "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB"):
        env.pop(k, None)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ACTINIC HOST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
