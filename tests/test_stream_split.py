"""How the per-byte kernels' launchers cut a byte range, on the CPU.

``csrc/vf_stream_split.h`` splits a range into the head bytes before a 16-B boundary, a body of
whole vectors and the tail bytes, and cuts a body above 512 MiB into sub-launches of at most
256 MiB; the launchers of the invert, table, binary and shifting kernels all go through it.  It is
host-only arithmetic, so g++ builds it here -- with ``-fsanitize=address,undefined`` -- into
``tests/stream/stream_split_check.cc``, a stand-alone program that allocates nothing and so checks
the cut at 12.7 GB and 25.4 GB too: every pointer offset 0..15, sizes around 0, 16, a tile,
512 MiB and those; the parts add up, the chunks cover the body once and in order in whole tiles,
``first`` and ``last`` are each set once, and the table kernel's three channel phases are
``(phase + offset) % 3``.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "stream", "stream_split_check.cc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stream") / "stream_split_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


# vectors per tile: 256 lanes x U, U = 4 in the library and 1, 2, 8 in tools/tune_invert.hip
@pytest.mark.parametrize("tile", [256, 512, 1024, 2048])
def test_split_and_chunks_at_every_offset_up_to_25_gigabytes(checker, tile):
    p = subprocess.run([checker, str(tile)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (tile, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    out = json.loads(p.stdout)
    # 107 sizes (6 centres x 11 distances less the 7 below zero, and 48 around the cut) x 16 offsets
    assert out["cases"] == 107 * 16 and out["failed"] == 0, out
    assert out["chunks"] > 4 * out["cases"], out  # the large sizes are cut: into 3, 48 and 95 chunks
