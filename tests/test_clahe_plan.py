"""The host-side plan of CLAHE, on the CPU.

``csrc/vf_clahe_plan.h`` holds the limits of the filter's arguments with their refusal messages, the
tile geometry, and the rules that the kernels compile as well: ``clip_of``, ``clahe_table`` (clip,
redistribute, scale), ``clahe_weights`` and ``clahe_pixel``.  g++ builds
``tests/clahe/clahe_plan_check.cc`` against it -- with ``-fsanitize=address,undefined`` and
``-ffp-contract=off``, a stand-alone program, as ``test_level_plan.py`` builds its checker -- and every
number it prints must equal ``_clahe_ref``'s, which is written from the rule's definition with
``np.float32`` arithmetic.  Floats cross as their bit patterns.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _clahe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-video-filter_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "clahe", "clahe_plan_check.cc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("clahe_plan") / "clahe_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


def _run(checker, mode, lines):
    p = subprocess.run([checker, mode], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (mode, p.returncode, p.stderr[-4000:])
    out = p.stdout.splitlines()
    assert len(out) == len(lines), (mode, len(out), len(lines))
    return [[int(v) for v in line.split()] for line in out]


def test_the_limits_and_their_reasons(checker):
    p = subprocess.run([checker, "limits"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    out = json.loads(p.stdout)
    assert out["failed"] == 0 and out["checked"] >= 70, out


# (W, H, tiles_x, tiles_y): both axes divide; one divides (the full-tile pad); neither; a side of 1; a
# pad larger than the axis (it reflects more than once)
GEOMETRY = [(64, 64, 8, 8), (1920, 1080, 8, 8), (16, 16, 16, 16), (64, 66, 8, 8), (66, 64, 8, 8), (1920, 1081, 8, 8),
            (130, 250, 8, 8), (241, 135, 16, 16), (13, 17, 2, 4), (1, 1, 8, 8), (1, 1, 1, 1), (5, 1, 8, 8), (1, 5, 8, 8),
            (300, 3, 16, 1), (7, 5, 8, 8), (2, 2, 16, 16), (3, 2, 16, 16), (2, 9, 7, 8), (53, 97, 1, 1), (480, 480, 8, 8)]


def test_geometry_and_the_reflected_margin(checker):
    got = _run(checker, "geometry", [f"{w} {h} {tx} {ty}" for w, h, tx, ty in GEOMETRY])
    for (w, h, tx, ty), g in zip(GEOMETRY, got):
        he, we, th, tw = R.geometry(h, w, tx, ty)
        want = [we, he, tw, th, tw * th] + [R.reflect101(p, w) for p in range(w, we)] + \
               [R.reflect101(p, h) for p in range(h, he)]
        assert g == want, (w, h, tx, ty)
    assert R.geometry(66, 64, 8, 8) == (72, 72, 9, 9)  # the width divides and is padded by a full 8 all the same
    assert R.geometry(64, 64, 8, 8) == (64, 64, 8, 8)
    assert R.geometry(1, 1, 8, 8) == (8, 8, 1, 1) and R.reflect101(7, 1) == 0
    assert [R.reflect101(p, 2) for p in range(2, 8)] == [0, 1, 0, 1, 0, 1]  # more than one reflection


def test_clip_of(checker):
    cases = [(1, 1), (1, 32400), (1, 65535), (1, 65536), (256, 1), (256, 255), (256, 256), (256, 32400), (512, 32400),
             (512, 81), (640, 32400), (10240, 32400), (1 << 16, 32400), (1 << 17, 100), (1 << 24, 32400),
             (1 << 24, (1 << 31) - 1), (3, (1 << 31) - 1), (512, 1), (511, 128), (513, 128)]
    got = _run(checker, "clip", [f"{q} {a}" for q, a in cases])
    for (q, a), g in zip(cases, got):
        assert g == [R.clip_of(q, a)], (q, a)
    assert R.clip_of(1, 32400) == 1 and R.clip_of(256, 32400) == 126 and R.clip_of(512, 32400) == 253
    assert R.clip_of(1 << 16, 32400) == 32400 and R.clip_of(1 << 24, 32400) > 32400  # at or above the area: no bin is cut


def _with_excess(rng, clip, excess, others=40):
    """A histogram whose excess above ``clip`` is exactly ``excess``: one bin at clip + excess, ``others`` at or below
    the clip."""
    h = np.zeros(256, np.int64)
    bins = rng.choice(256, others + 1, replace=False)
    h[bins[0]] = clip + excess
    h[bins[1:]] = rng.integers(0, clip + 1, others)
    return h


def _table_cases():
    rng = np.random.default_rng(20261021)
    cases = []  # (name, h, clip in counts)
    one = np.zeros(256, np.int64)
    one[0] = 1
    cases += [("area_1", one, 0), ("area_1_clip_1", one, 1)]
    two = np.zeros(256, np.int64)
    two[[3, 200]] = 1
    cases += [("area_2", two, 0), ("area_2_clip_1", two, 1)]
    two_same = np.zeros(256, np.int64)
    two_same[77] = 2
    cases += [("area_2_one_bin", two_same, 1)]
    for b in (0, 100, 255):
        for area in (81, 32400, 57600):
            full = np.zeros(256, np.int64)
            full[b] = area
            for clip in (0, 1, R.clip_of(512, area), area, 2 * area):
                cases.append((f"full_bin_{b}_area_{area}_clip_{clip}", full, clip))
    for residual in (0, 1, 2, 3, 85, 86, 127, 128, 129, 254, 255):  # step: -, 256, 128, 85, 3, 2, 2, 2, 1, 1, 1
        for batch in (0, 1, 7):
            cases.append((f"residual_{residual}_batch_{batch}", _with_excess(rng, 50, 256 * batch + residual), 50))
    for area in ((1 << 24) - 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 31) - 1):  # the int-to-float conversion rounds
        h = np.zeros(256, np.int64)
        h[[3, 200]] = [1, area - 1]
        cases += [(f"area_{area}", h, 0), (f"area_{area}_clipped", h, area // 3)]
        spread = rng.multinomial(area, np.full(256, 1 / 256)).astype(np.int64)
        cases += [(f"spread_{area}", spread, 0), (f"spread_{area}_clipped", spread, int(spread.mean()))]
    for k in range(60):
        area = int(rng.integers(1, 1 << int(rng.integers(1, 25))))
        nb = int(min(area, rng.integers(1, 257)))
        p = rng.random(nb) ** 3
        h = np.zeros(256, np.int64)
        h[rng.choice(256, nb, replace=False)] = rng.multinomial(area, p / p.sum())
        for q in (0, 1, 256, 512, 10240):
            cases.append((f"random_{k}_q{q}", h, R.clip_of(q, area) if q else 0))
    return cases


def test_clahe_table_equals_the_reference(checker):
    cases = _table_cases()
    lines = [f"{int(h.sum())} {clip} " + " ".join(str(int(v)) for v in h) for _, h, clip in cases]
    got = _run(checker, "table", lines)
    assert len(got) > 390
    bad = [name for (name, h, clip), g in zip(cases, got) if not np.array_equal(g, R.table(h, int(h.sum()), clip))]
    assert not bad, bad[:10]


def test_the_cases_exercise_what_they_are_there_for():
    """The reference itself on the edges, so a case that stops exercising its edge shows."""
    h = np.zeros(256, np.int64)
    h[[3, 200]] = [1, 1 << 24]
    assert np.float32((1 << 24) + 1) == np.float32(1 << 24)  # 2^24 + 1 is no float32
    assert R.table(h, (1 << 24) + 1, 0)[200] == 255
    # residual 128: step 2, every second bin gains one; 129: step 1, the first 129 bins gain one
    flat = np.zeros(256, np.int64)
    flat[9] = 128 + 10
    r = R.redistribute(flat, 10)
    assert r[0] == 1 and r[1] == 0 and r[254] == 1 and r[255] == 0 and r[9] == 10 and sum(r) == 138
    flat[9] = 129 + 10
    r = R.redistribute(flat, 10)
    assert r[:129] == [1] * 9 + [11] + [1] * 119 and r[129] == 0 and sum(r) == 139
    flat[9] = 1 + 10
    assert R.redistribute(flat, 10)[0] == 1 and sum(R.redistribute(flat, 10)) == 11
    flat[9] = 255 + 10
    assert R.redistribute(flat, 10)[254] == 1 and R.redistribute(flat, 10)[255] == 0
    # the closed form of the plan header, against cv2's loop, for every residual
    for residual in range(1, 256):
        step = max(256 // residual, 1)
        gained = [1 if v % step == 0 and v // step < residual else 0 for v in range(256)]
        h1 = np.zeros(256, np.int64)
        h1[0] = residual + 1
        want = R.redistribute(h1, 1)
        want[0] -= 1
        assert gained == want, residual


AXES = [(tw * tiles - cut, tw, tiles) for tw in (1, 3, 17, 240) for tiles in (1, 2, 8, 16) for cut in (0, 1)
        if tw * tiles - cut >= 1] + [(5, 1, 8), (1, 1, 8), (130, 17, 8), (300, 19, 16)]


def _raw(n, side):
    x = np.arange(n, dtype=np.int64).astype(np.float32)
    return np.floor(x * (np.float32(1.0) / np.float32(side)) - np.float32(0.5)).astype(np.int64)


def test_weights_of_every_coordinate_and_the_cell_starts(checker):
    got = _run(checker, "weights", [f"{n} {side} {tiles}" for n, side, tiles in AXES])
    for (n, side, tiles), g in zip(AXES, got):
        t1, t2, a, a1 = R.weights(n, side, tiles)
        raw = _raw(n, side)
        per = np.array(g[:5 * n], np.int64).reshape(n, 5)
        assert np.array_equal(per[:, 0], t1) and np.array_equal(per[:, 1], t2) and np.array_equal(per[:, 2], raw), (n, side, tiles)
        assert np.array_equal(per[:, 3].astype(np.uint32), a.view(np.uint32)), (n, side, tiles)
        assert np.array_equal(per[:, 4].astype(np.uint32), a1.view(np.uint32)), (n, side, tiles)
        starts = g[5 * n:]
        assert len(starts) == tiles + 2
        want = [int(np.searchsorted(raw, k, side="left")) for k in range(-1, tiles + 1)]  # raw never falls
        assert np.all(np.diff(raw) >= 0) and starts == want, (n, side, tiles, starts, want)
        assert raw.min() >= -1 and raw.max() <= tiles - 1
    # the first and the last half tile: both indices clamp to the same tile
    t1, t2, a, a1 = R.weights(1920, 240, 8)
    assert np.all(t1[:120] == 0) and np.all(t2[:120] == 0) and t1[120] == 0 and t2[120] == 1
    assert np.all(t1[1800:] == 7) and np.all(t2[1800:] == 7) and t1[1799] == 6 and t2[1799] == 7


def test_clahe_pixel_equals_the_reference(checker):
    rng = np.random.default_rng(77)
    lines, want = [], []
    for n, side, tiles in [(1920, 240, 8), (1080, 135, 8), (48, 3, 16), (136, 17, 8), (300, 19, 16)]:
        _, _, a, a1 = R.weights(n, side, tiles)
        for _ in range(400):
            i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
            t = rng.integers(0, 256, 4) if rng.random() < 0.8 else rng.choice([0, 255, 254, 1], 4)
            f = np.array([a[i], a1[i], a[j], a1[j]], np.float32)
            lines.append(" ".join(str(int(v)) for v in t) + " " + " ".join(str(int(v)) for v in f.view(np.uint32)))
            want.append(int(R.blend(t[0], t[1], t[2], t[3], f[0], f[1], f[2], f[3])))
    got = _run(checker, "pixel", lines)
    assert [g[0] for g in got] == want
