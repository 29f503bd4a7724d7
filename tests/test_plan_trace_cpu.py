"""What the host side of librtd does, call by call, held to a recorded trace.

tests/cpu/plan_trace_host_main.cpp drives scripted scenarios through the public C entry points over the stand-in runtime and the
shadow launchers, both built with -DFAKE_HIP_TRACE: every stream, event, copy, fill, allocation and launch appends one text line
(streams and events as ordinals, device pointers as allocation + byte offset).  tests/golden/host_trace/<scenario>.txt were recorded
with csrc/rtd_api.hip as it stood BEFORE its repeated plan-state, buffer and result code was folded; the output must equal them line
for line.  A flag left out of one "inputs changed" transition, a table launch on another stream, a `3 * C * nt` that became `C * nt`
is a changed line here, on the CPU, under the address / undefined-behaviour sanitizers, before any of it runs on a GPU.

Scenarios g (viewing angles, with the corrections at the angles on one and on three windows), h (requested surfaces, rtd_plan_get_bdrf
and the plan-free helpers) and i (Lambertian coupling) were recorded the same way, twice with identical output, from commit 3587553
("Lambertian albedo sweeps from one solve, coupled on the device"): rtd_api.hip as it stood before its fetch, one-shot and scratch-block
code was folded.  They use 6 columns (3 profiles x 2 spectral points), the fewest that windows or chunks of 2 split in three."""
import os

import pytest

import host_program

SCENARIOS = ["a", "b", "b_serial", "c", "d", "e", "f", "g", "h", "i"]
GOLDEN = os.path.join(host_program.ROOT, "tests", "golden", "host_trace")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program.build(tmp_path_factory.mktemp("plan_trace"), "plan_trace_host_main.cpp", "plan_trace_host", defines=["FAKE_HIP_TRACE"])


def _lines(name):
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_the_host_calls_of_a_scenario_equal_the_recorded_trace(exe, scenario):
    r = host_program.run(exe, scenario)
    assert r.returncode == 0 and f"PLAN TRACE {scenario} OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), _lines(scenario)
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, f"line {first + 1}: got {got[first:first + 1]}, recorded {want[first:first + 1]}"


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return host_program.build(tmp_path_factory.mktemp("plan_trace_selftest"), "plan_trace_host_main.cpp", "plan_trace_selftest",
                              defines=["FAKE_HIP_TRACE", "RTD_TRACE_SELFTEST"])


@pytest.mark.parametrize("scenario", ["b", "g"])
def test_the_trace_sees_a_view_that_changed(selftest, scenario):
    """Sensitivity: with -DRTD_TRACE_SELFTEST the shadow of the tables launcher reports one column more than its view has -- what a
    wrong window count would look like -- and the comparison must fail (b: a windowed plan; g: its last part is one too)."""
    r = host_program.run(selftest, scenario)
    assert r.returncode == 0, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), _lines(scenario)
    assert len(got) == len(want) and got != want
    changed = [w for g, w in zip(got, want) if g != w]
    assert changed and all(w.startswith("tables ") for w in changed)
