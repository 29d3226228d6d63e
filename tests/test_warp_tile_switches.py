"""The warp's tile switches, ``VF_WARP_ROWS`` and ``VF_WARP_LDS``: that the cases of
``tests/test_gpu_warp.py::test_the_tile_switches_change_no_byte`` reach what they are chosen for.  Needs no GPU."""
import os

import _warp_ref as R
from test_gpu_warp import (LDS, MAX_LDS, MAX_ROWS, SWITCH_SIZES, SWITCHES, TILE_H, TILE_W, _clamped, _maps, _tile_boxes,
                           _tile_paths)


def test_the_switch_cases_are_what_they_are_chosen_for():
    """Needs no GPU.  The constants the cases were written for are still the sources'; at 64 rows and the cap a box
    larger than the default budget is staged, so the large dynamic allocation is launched and used past its first
    16 KiB; 16 rows at the cap stage the shrink's box, which the default budget refuses; 16 bytes stage next to
    nothing, but not nothing."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-video-filter_amd", "csrc",
                            "vf_warp.hip")).read()
    for name, value in (("kTileW", TILE_W), ("kTileRows", TILE_H), ("kMaxTileRows", MAX_ROWS), ("kWarpLds", LDS),
                        ("kMaxWarpLds", MAX_LDS)):
        assert re.findall(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+)\s*;" % name, src) == [str(value)], name
    assert len(re.findall(r'env_size\("VF_WARP_LDS"', src)) == 1 and len(re.findall(r'env_size\("VF_WARP_ROWS"', src)) == 1
    assert "static const size_t lds" not in src  # read at every launch, which test_the_tile_switches_change_no_byte relies on
    assert MAX_LDS + 2 * MAX_ROWS * 4 < 65536  # the dynamic LDS and the static row bases
    assert [_clamped(r, b) for r, b in [(100, 1000), (0, 1000000), (64, 16), (5, 61440)]] == \
        [(64, 992), (1, 61440), (64, 16), (5, 61440)]
    assert {_clamped(r, b) for r, b in SWITCHES} >= {(64, 61440), (64, 992), (1, 16), (1, 61440), (64, 16), (5, 992)}
    assert sum(1 for r, b in SWITCHES if _clamped(r, b) == (64, 61440)) >= 3  # 61440, 1000000, and 100 rows
    m = _maps(70, 130)["rows_x2"][1]
    for c in (1, 3):
        for interp in (R.LINEAR, R.NEAREST):
            boxes = _tile_boxes(70, 130, c, m, interp, 64, MAX_LDS)
            assert len(boxes) == 6 and boxes[0][0] == "lds", (c, interp, boxes)
            assert _tile_paths(70, 130, c, m, interp)[0] == "lds"  # and 16 rows fit the default budget
    big = _tile_boxes(70, 130, 3, m, R.LINEAR, 64, MAX_LDS)[0]
    assert big == ("lds", 208 * 128) and LDS < big[1] <= MAX_LDS
    assert _tile_boxes(70, 130, 3, m, R.LINEAR, 64, LDS)[0] == ("budget", 208 * 128)
    assert _tile_boxes(70, 130, 3, m, R.LINEAR, 64, 992)[0][0] == "budget"
    shrink = [4, 0, 0, 0, 4, 0]
    assert _tile_boxes(300, 80, 3, shrink, R.LINEAR, TILE_H, MAX_LDS)[0] == ("lds", 768 * 62)
    assert _tile_paths(300, 80, 3, shrink, R.LINEAR, 64, MAX_LDS)[0] == "border"  # 64 rows of it leave the frame
    # 16 bytes: one row of at most 16 bytes.  The flip of 65 x 17 in tiles of one row has a second tile column of one
    # pixel, which is staged; every tile of more rows, and every tile of 64 pixels, takes the general path
    flip = R.resolve(R.FLIP_BOTH, None, TILE_W + 1, TILE_H + 1)
    one = _tile_paths(TILE_W + 1, TILE_H + 1, 3, flip, R.NEAREST, 1, 16)
    assert one.count("lds") == TILE_H + 1 and one.count("budget") == TILE_H + 1
    for w, h in SWITCH_SIZES:
        for rows in (5, 64):
            paths = _tile_paths(w, h, 3, _maps(w, h)["rotate30_scale1.3"][1], R.LINEAR, rows, 16)
            assert "lds" not in paths and ("budget" in paths or (w, h, rows) != (160, 48, 5)), (w, h, rows)
    # the rotation of 160 x 48 has staged tiles and border tiles in one frame at 1 and 5 rows a tile; at 64 rows every
    # tile of it touches the border, and the shift of 70 x 130 has a staged second row of tiles under a first that
    # reads row -1
    for rows in (1, 5):
        paths = _tile_paths(160, 48, 3, _maps(160, 48)["rotate30_scale1.3"][1], R.LINEAR, rows, MAX_LDS)
        assert "lds" in paths and "border" in paths, (rows, paths)
    paths = _tile_paths(70, 130, 3, _maps(70, 130)["shift_32nds"][1], R.LINEAR, 64, MAX_LDS)
    assert paths[:4] == ["border", "border", "lds", "border"], paths
