"""How the table filter cuts frames into launches, on the CPU.

``csrc/vf_lut_split.h`` turns a list of frames, a capacity and a channel count into the kernel
launches ``vf_lut_frames_host`` issues: a frame larger than the staging capacity is cut wherever
the capacity ends, mid-pixel if need be, and each launch carries the channel of its first byte.
The header is host-only C++, so g++ builds it here -- with ``-fsanitize=address,undefined`` --
into ``tests/lut/lut_split_check.cc``, a stand-alone program that checks that the launches tile
every frame exactly once and in order, each fit the capacity and carry ``phase ==
offset_in_frame % channels``, and that running them byte by byte gives the whole-frame filter.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lut", "lut_split_check.cc")

SMALL = [0, 1, 2, 3, 15, 16, 17, 47, 48, 49]
CAPACITIES = [1, 2, 3, 16, 17, 48, 50, 4096, 4099]  # multiples of 3 and not


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("lut") / "lut_split_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(exe, cap, channels, sizes):
    p = subprocess.run([exe, str(cap), str(channels)] + [str(s) for s in sizes], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, (cap, channels, sizes, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout)


def _launches(sizes, cap):
    return sum((s + cap - 1) // cap for s in sizes)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("cap", CAPACITIES)
def test_frames_are_tiled_once_in_order_with_their_phase(checker, cap, channels):
    sizes = SMALL + [cap - 1, cap, cap + 1, 3 * cap + 2]
    out = _run(checker, cap, channels, sizes)
    assert out == {"frames": len(sizes), "launches": _launches(sizes, cap), "failed": 0}
    # and with the frames in another order: a cut frame does not disturb the ones after it
    sizes = [3 * cap + 2, 0, cap + 1] + SMALL[::-1] + [cap, cap - 1]
    out = _run(checker, cap, channels, sizes)
    assert out == {"frames": len(sizes), "launches": _launches(sizes, cap), "failed": 0}


def test_no_frames_and_degenerate_arguments(checker):
    assert _run(checker, 16, 3, []) == {"frames": 0, "launches": 0, "failed": 0}
    assert _run(checker, 16, 3, [0, 0]) == {"frames": 2, "launches": 0, "failed": 0}
    assert _run(checker, 0, 3, [5, 6]) == {"frames": 2, "launches": 0, "failed": 0}
    assert _run(checker, 16, 0, [5, 6]) == {"frames": 2, "launches": 0, "failed": 0}
