"""The host-side plan of the resize, on the CPU.

``csrc/vf_resize_plan.h`` holds the limits of the filter's arguments with their refusal messages, the result's
size, the mode a frame resolves to, and the rules that the kernel compiles as well: ``col_coef``, ``row_coef``,
``nearest_index``, ``area_pixel``, ``linear_pixel`` and ``tile_footprint``.  g++ builds
``tests/resize/resize_plan_check.cc`` against it -- with ``-fsanitize=address,undefined`` and
``-ffp-contract=off``, a stand-alone program, as ``test_warp_plan.py`` builds its checker -- and every number it
prints must equal the golden values of ``tests/golden/resize_plan.json``, which were dumped from ``_resize_ref``
(``python tests/test_resize_plan.py --write`` dumps them again); the reference is compared live as well, so a
difference names its pixel.  Doubles cross as their bit patterns.
"""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import _resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "resize", "resize_plan_check.cc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_plan.json")

AXES = [(n, d) for n in range(1, 41) for d in range(1, 61)]  # frames up to 40, destinations up to 60


def _digest(values):
    return hashlib.sha256(np.ascontiguousarray(values, dtype="<i8").tobytes()).hexdigest()[:16]


def _axis_ref(n, d):
    scale = R.scales(n, n, (d, d))[0]
    cs, a0, a1 = R.axis_coef(scale, d, n, True)
    rs, b0, b1 = R.axis_coef(scale, d, n, False)
    return np.stack([cs, a0, a1, rs, b0, b1, R.nearest_index(scale, d, n)], axis=1).reshape(-1)


def _pixel_cases():
    """(frame, dsize or None, fx, fy, interp): every mode, both forms, sizes up to 40 x 40 -> 60 x 60."""
    rng = np.random.default_rng(26)
    cases = []
    pairs = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 3), (1, 1)), ((2, 2), (7, 5)), ((9, 1), (4, 1)), ((1, 9), (1, 20)),
             ((17, 11), (17, 11)), ((17, 11), (34, 22)), ((34, 22), (17, 11)), ((37, 23), (60, 60)), ((40, 40), (13, 7)),
             ((40, 40), (59, 3)), ((30, 20), (10, 10)), ((40, 32), (8, 2))]
    for (w, h), dsize in pairs:
        for interp in (R.NEAREST, R.LINEAR, R.AREA):
            c = int(rng.choice([1, 3]))
            img = rng.integers(0, 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)
            cases.append((img, dsize, 0.0, 0.0, interp))
    for k, l in [(1, 1), (2, 2), (3, 2), (2, 3), (3, 3), (4, 4), (7, 5), (16, 16)]:
        if 9 * k <= 40 and 5 * l <= 40:
            cases.append((rng.integers(0, 256, (5 * l, 9 * k, 3), dtype=np.uint8), (9, 5), 0.0, 0.0, R.AREA))
    cases.append((rng.integers(0, 256, (32, 32), dtype=np.uint8), (2, 2), 0.0, 0.0, R.AREA))  # 16 x 16
    for (w, h), fx, fy in [((37, 35), 0.3, 0.3), ((5, 7), 0.5, 0.5), ((7, 5), 0.5, 0.5), ((7, 7), 0.5, 0.25), ((11, 5), 1 / 3, 0.5),
                           ((9, 9), 1.5, 2.0), ((3, 3), 0.1, 0.1)]:
        for interp in (R.NEAREST, R.LINEAR, R.AREA):
            cases.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), None, fx, fy, interp))
    return cases


def _pixel_ref(img, dsize, fx, fy, interp):
    """"dw dh" and the bytes, or None where the reference refuses."""
    try:
        out = R.resize(img, dsize, fx, fy, interp)
    except ValueError:
        return None
    return np.concatenate([[out.shape[1], out.shape[0]], out.reshape(-1).astype(np.int64)])


def _golden():
    return {"axis": {f"{n} {d}": _digest(_axis_ref(n, d)) for n, d in AXES},
            "pixels": ["refused" if r is None else _digest(r) for r in (_pixel_ref(*c) for c in _pixel_cases())]}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("resize_plan") / "resize_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _run(checker, mode, lines):
    p = subprocess.run([checker, mode], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (mode, p.returncode, p.stderr[-4000:])
    out = p.stdout.splitlines()
    assert len(out) == len(lines), (mode, len(out), len(lines))
    return out


def _self_check(checker, mode, at_least):
    p = subprocess.run([checker, mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    out = json.loads(p.stdout)
    assert out["failed"] == 0 and out["checked"] >= at_least, out


def _bits(v):
    return str(struct.unpack("<Q", struct.pack("<d", float(v)))[0])


def test_the_limits_and_their_reasons(checker):
    _self_check(checker, "limits", 29)


def test_the_footprint_of_a_tile_by_brute_force(checker):
    _self_check(checker, "footprint", 5000)


def test_coefficients_and_nearest_indices(checker, golden):
    got = _run(checker, "axis", [f"{n} {d}" for n, d in AXES])
    assert set(golden["axis"]) == {f"{n} {d}" for n, d in AXES}
    for (n, d), line in zip(AXES, got):
        g = np.array([int(v) for v in line.split()], np.int64)
        want = _axis_ref(n, d)
        assert np.array_equal(g, want), (n, d, g.reshape(-1, 7), want.reshape(-1, 7))
        assert _digest(g) == golden["axis"][f"{n} {d}"], (n, d)


def test_pixels_of_every_mode_and_both_forms(checker, golden):
    cases = _pixel_cases()
    lines = []
    for img, dsize, fx, fy, interp in cases:
        c = 3 if img.ndim == 3 else 1
        dw, dh = dsize if dsize else (0, 0)
        lines.append(f"{img.shape[1]} {img.shape[0]} {c} {dw} {dh} {_bits(fx)} {_bits(fy)} {interp} {img.tobytes().hex()}")
    got = _run(checker, "pixels", lines)
    assert len(golden["pixels"]) == len(cases)
    refused = 0
    for (img, dsize, fx, fy, interp), line, gold in zip(cases, got, golden["pixels"]):
        want = _pixel_ref(img, dsize, fx, fy, interp)
        if want is None:
            refused += 1
            assert line.strip() == "refused" and gold == "refused", (img.shape, dsize, fx, fy, interp)
            continue
        g = np.array([int(v) for v in line.split()], np.int64)
        assert np.array_equal(g, want), (img.shape, dsize, fx, fy, interp)
        assert _digest(g) == gold
    assert 0 < refused < len(cases) // 2


if __name__ == "__main__" and "--write" in sys.argv:
    with open(GOLDEN, "w") as f:
        json.dump(_golden(), f, indent=0, sort_keys=True)
        f.write("\n")
