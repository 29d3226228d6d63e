"""The pixel split of the colour-matrix kernel's launcher, on the CPU.

``csrc/vf_pixel_split.h`` cuts a range of whole 3-byte pixels into a head, a body of 48-byte units
that starts where a pixel starts and where ``dst`` is 16-byte aligned, and a tail.  It is plain C++
(the library compiles the same text), so g++ builds it here -- with
``-fsanitize=address,undefined`` -- into ``tests/mix/pixel_split_check.cc``, a stand-alone program,
which checks every ``dst`` offset 0..15 against every length 0, 3, ..., 300 (and three past 2^32):
head, body and tail add up; ``head % 3 == 0``; ``(dst + head) % 16 == 0`` or the range is all head;
the body is a multiple of 48; ``tail < 48``.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "mix", "pixel_split_check.cc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("mix") / "pixel_split_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def test_every_offset_and_length(checker):
    p = subprocess.run([checker], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    out = json.loads(p.stdout)
    assert out["failed"] == 0 and out["checked"] == 16 * (101 + 3), out
    assert out["all_head"] > 16 and out["with_body"] > 16 * 60, out
