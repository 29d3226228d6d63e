"""The separable step in the plan of a filter chain, on the CPU.

``csrc/vf_chain_plan.h`` knows the step kind 7, ``kSep`` (4, 6, 9 and -1 stay the "unknown kind N"
that the other checkers pin).  g++ builds ``tests/chain/chain_plan_sep_check.cc`` against it -- with
``-fsanitize=address,undefined``, as its siblings are built -- a stand-alone program that checks: kind
7 is accepted with tap counts up to 31 and bad sides are refused with a message of their own, the
conv and rank limit and message unchanged; a separable step is never placed in place and nothing
folds across one; ``single_kind`` reports it; its vertical radius is kh / 2 and a chain's reach
passes 100 rows; and a scalar model of the steps run band by band, on only the rows the plan says
exist, equals the whole frame for programs with separable steps (two in a row, one feeding a
binary step, one between a rank and a table) over H in {1, 2, 9, 40, 70}, the three borders and
every capacity from 2 R + 1 rows up.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "chain", "chain_plan_sep_check.cc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("chain_sep") / "chain_plan_sep_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout)


def test_kind_7_is_accepted_and_kinds_4_6_9_stay_refused(checker):
    out = _run(checker, "validate")
    assert out["failed"] == 0 and out["checked"] >= 50, out


def test_never_in_place_no_fold_single_kind_and_reach(checker):
    out = _run(checker, "plan")
    assert out["failed"] == 0 and out["checked"] == 14, out


def test_bands_of_programs_with_separable_steps_equal_the_whole_frame(checker):
    out = _run(checker, "grid")
    assert out["failed"] == 0 and out["bad_reads"] == 0, out
    assert out["cases"] > 1000 and out["multi_band"] > 500 and out["bands"] > out["cases"], out
