"""The host planner of vbm_synthesis_ranges (csrc/range_plan.h) without a device: tests/native/range_plan_host.cpp
plans random and edge ranges over seeded synthetic indexes at max_batch 2, 3, 7 and 64 and checks every plan against a
linear scan of the index: the samples each range gets, that a range without samples has no piece, that the packets
of a range's pieces are k .. m in order (behind the failed packets between k and its pre-roll, which the planner
decodes with them: they give no samples, and a good packet ahead of k is an error), that every pre-roll packet is
the last good packet of the range's stream before its piece, and that pieces, sub-call rows and output rows keep
within max_batch.  The program is built and run as a process of its own, plain and under the address and
undefined-behaviour sanitizers; nothing of it is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_and_run(tmp_path, flags):
    exe = str(tmp_path / "range_plan_host")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-Wall", *flags,
                           "-I" + os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "range_plan_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("range_plan_host ok:"), run.stdout + run.stderr


def test_planner_against_a_linear_scan(tmp_path):
    build_and_run(tmp_path, [])


def test_planner_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    link = subprocess.run(["c++", "-std=c++17", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")],
                          capture_output=True, text=True)
    if link.returncode != 0:
        pytest.skip("the compiler does not link with " + " ".join(SANITIZE) + ": " + link.stderr.strip()[-300:])
    build_and_run(tmp_path, SANITIZE)
