"""What the Python front end asks of the device, call by call, held to a recorded trace: the counterpart of test_plan_trace_cpu.py one
layer up.

tests/cpu/frontend_trace_driver.py runs scripted scenarios of pydisort(), pydisort_batch(), pydisort_band(), the two streamed forms
and every method of ``Plan`` over csrc/rtd_api.hip, the stand-in runtime and the shadow launchers, built with -DFAKE_HIP_TRACE as a
plain shared library (no sanitizer: nothing is preloaded).  After each call it prints the runtime calls the library made and the
keys, shapes and dtypes of what came back, or the exception and its message.  tests/golden/frontend_trace/<scenario>.txt were
recorded with pydisort_amd/ as it stood BEFORE the front end's repeated plan state, checks and result arrays were folded -- all but
`unset`, which holds the calls that raised AttributeError by accident then and a ValueError since.  A result array of another shape,
a pointer handed over in another order, a flag bit dropped from the evaluate word, a message that lost a word is a changed line
here, on the CPU."""
import os
import subprocess
import sys

import pytest

import host_program

SCENARIOS = ["batch", "raw", "thermal", "band", "streamed", "single", "refused", "unset"]
GOLDEN = os.path.join(host_program.ROOT, "tests", "golden", "frontend_trace")
DRIVER = os.path.join(host_program.CPU, "frontend_trace_driver.py")


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    return host_program.build_trace_library(tmp_path_factory.mktemp("frontend_trace"))


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_the_front_end_calls_of_a_scenario_equal_the_recorded_trace(library, scenario):
    env = dict(os.environ, RTD_LIB=library, FAKE_HIP_TOTAL=str(8 << 30))
    for k in ("RTD_POOL_BYTES", "RTD_WORK_BYTES", "RTD_NO_PIPELINE", "RTD_RCCL_STUB", "PYTHONPATH"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, DRIVER, scenario], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"FRONTEND TRACE {scenario} OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    # a library built without the trace macro logs nothing: the comparison of the shapes alone must not pass for it
    assert any(g.startswith("launch ") for g in got) and any(" D2H " in g for g in got)
    with open(os.path.join(GOLDEN, scenario + ".txt")) as f:
        want = f.read().splitlines()
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, f"line {first + 1}: got {got[first:first + 1]}, recorded {want[first:first + 1]}"
