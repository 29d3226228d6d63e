"""The JPEG decode plan's selection rules, on the CPU.

``csrc/vf_jpeg_plan.h`` resolves the ``VF_JPEG_*`` switches of an entry call and the traits of
its batch into the one ``DecodePlan`` that every later stage reads (the resync at
``wait_invert`` included).  The header is host-only C++, so g++ builds it here -- with
``-fsanitize=address,undefined`` -- into ``tests/plan/jpeg_plan_check.cc``, which fills
``JpegSwitches`` directly and checks every rule case by case, then every combination of the
span sync's switches and traits against the (G, table layout) pairs ``dec_syncg`` instantiates
(anything else is ``hipErrorInvalidValue`` on the GPU).  ``JpegSwitches::read()`` is checked in
a child process that has the fourteen variables set.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "plan", "jpeg_plan_check.cc")

NAMES = ["VF_JPEG_SYNC", "VF_JPEG_SYNC_LSB", "VF_JPEG_SYNC_TABS4", "VF_JPEG_SYNC_G", "VF_JPEG_SYNC_QUEUED",
         "VF_JPEG_SYNC_WARM", "VF_JPEG_SYNC_STATS", "VF_JPEG_CHUNKS", "VF_JPEG_WRITE4", "VF_JPEG_FUSE",
         "VF_JPEG_FUSE_IDCT", "VF_JPEG_IDCT24", "VF_JPEG_FETCH_LEARN", "VF_JPEG_TRACE"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("plan") / "jpeg_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(exe, mode, env=None):
    p = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


def test_every_selection_rule(checker):
    out = json.loads(_run(checker, "rules"))
    assert out["failed"] == 0 and out["checks"] >= 90  # every block of rules() ran


def test_span_sync_form_is_always_instantiated(checker):
    """G in {unset, -1 .. 9} x TABS4, LSB in {unset, 0, 1} x tabs4 x pow2bpm."""
    out = json.loads(_run(checker, "exhaustive"))
    assert out == {"cases": 12 * 3 * 3 * 2 * 2, "failed": 0}


def test_read_picks_up_each_switch(checker):
    base = {k: v for k, v in os.environ.items() if not k.startswith("VF_JPEG_")}
    unset = dict(line.split("=", 1) for line in _run(checker, "read", base).splitlines())
    assert unset == {n: "<unset>" for n in NAMES}
    env = dict(base, **{n: "value-%d" % i for i, n in enumerate(NAMES)})
    got = dict(line.split("=", 1) for line in _run(checker, "read", env).splitlines())
    assert got == {n: "value-%d" % i for i, n in enumerate(NAMES)}
    for n in NAMES:  # and one at a time: no name read into another's field
        one = dict(line.split("=", 1) for line in _run(checker, "read", dict(base, **{n: "x"})).splitlines())
        assert one == {m: "x" if m == n else "<unset>" for m in NAMES}
