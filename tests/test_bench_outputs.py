"""bench.py's command line: a plain run does the headline's timed steps and nothing beside
them, --full brings every other leg back, and --dump-outputs writes what the last timed step
computed (checked against the oracle on the GPU)."""
import os
import sys

import numpy as np
import pytest

import bench
from oracle import oracle

LEG_SWITCHES = ("no_traffic", "no_e2e", "no_jpeg", "no_distributor", "no_sizes", "no_sweep", "no_per_frame")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.select_legs(bench.parse())


def test_plain_run_has_no_legs_beside_the_headline(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (args.gpus, args.steps, args.warmup) == (1, 7, 3)
    assert not args.full and args.dump_outputs is None
    assert all(getattr(args, k) for k in LEG_SWITCHES)
    assert args.cpu_seconds == 0.0


def test_full_run_keeps_every_leg_and_its_switches(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3", "--full")
    assert args.full and not any(getattr(args, k) for k in LEG_SWITCHES)
    assert args.cpu_seconds == 10.0 and args.dist_reps == 5
    args = _parse(monkeypatch, "--full", "--no-sweep", "--cpu-seconds", "2", "--dump-outputs", "d")
    assert args.no_sweep and not args.no_jpeg and args.cpu_seconds == 2.0 and args.dump_outputs == "d"


def test_leg_children_keep_the_options_their_parent_gave(monkeypatch):
    """The legs' child processes are started without --full: they are no plain runs, and what
    the parent passed (the JPEG leg's libjpeg-turbo sample length among it) reaches them."""
    cmd = bench.jpeg_child_cmd(0, 32, 10.0)
    assert cmd[1] == os.path.abspath(bench.__file__) and "--full" not in cmd
    args = _parse(monkeypatch, *cmd[2:])
    assert bench.is_child(args) and args.jpeg_child == 0 and args.batch == 32
    assert args.cpu_seconds == 10.0
    assert _parse(monkeypatch, *bench.jpeg_child_cmd(3, 32, 0)[2:]).cpu_seconds == 0.0
    for argv in (["--probe", "--steps", "20", "--batch", "32", "--ring-gb", "2.4"],
                 ["--cpu-worker", "5.0"], ["--host-copy-child", "3.0"]):
        args = _parse(monkeypatch, *argv)
        assert bench.is_child(args) and args.cpu_seconds == 10.0
        assert not any(getattr(args, k) for k in LEG_SWITCHES)
    assert not bench.is_child(_parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3"))


def test_last_step_outputs_is_the_slot_the_last_step_wrote():
    ring = ["d0", "d1", "d2", "d3", "d4", "d5"]
    assert [bench.last_step_outputs(ring, k) for k in (1, 2, 6, 7, 20, 300)] == ["d0", "d1", "d5", "d0", "d1", "d5"]
    assert bench.last_step_outputs(["d0", "d1"], 4) == "d1"


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_steps_output(vf_ctx, tmp_path):
    """Two ring slots of two 1080p frames, four steps: the last one (step 3) writes slot 1,
    whose inputs are frames 2 and 3; slot 0 is poisoned after the run, so the buffer that the
    bench's own choice (last_step_outputs) hands to dump_outputs has to be slot 1.  Every
    dumped array is the oracle's invert of those frames, in float32 / float64, and the sample's
    positions are the same on every call."""
    from vfilter import sharding
    from vfilter.synthetic import synthetic_frame
    batch, steps = 2, 4
    srcs, dsts, batch_bytes, _ = bench.make_ring(vf_ctx, batch, 0.0, np)
    try:
        assert len(srcs) == 2 and batch_bytes == batch * bench.FRAME_BYTES
        vf_ctx.bench_device_ring(srcs, dsts, batch_bytes, steps)
        vf_ctx.memset_device(dsts[0], 0x5A, batch_bytes)
        vf_ctx.sync()
        dst = bench.last_step_outputs(dsts, steps)
        paths = bench.dump_outputs(vf_ctx, dst, batch, batch_bytes, str(tmp_path / "out"), np)
        again = bench.dump_outputs(vf_ctx, dst, batch, batch_bytes, str(tmp_path / "again"), np)
    finally:
        for p in srcs + dsts:
            vf_ctx.free_device(p)
    frames = [synthetic_frame(sharding.synthetic_seed(i), bench.H, bench.W) for i in (2, 3)]
    want = oracle.invert(np.stack(frames))
    assert sorted(paths) == ["output_frame0", "output_row_sums", "output_sample"]
    got = {k: np.load(v) for k, v in paths.items()}
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["output_frame0"].dtype == np.float32 and got["output_sample"].dtype == np.float32
    assert got["output_row_sums"].dtype == np.float64
    assert np.array_equal(got["output_frame0"], want[0].astype(np.float32))
    assert np.array_equal(got["output_row_sums"],
                          want.reshape(batch, bench.H, -1).sum(axis=2, dtype=np.float64))
    flat = want.reshape(-1)
    assert got["output_sample"].shape == (bench.DUMP_SAMPLE,)
    assert got["output_sample"][0] == flat[0] and got["output_sample"][-1] == flat[-1]
    idx = np.sort(np.random.default_rng(0).integers(0, batch_bytes, bench.DUMP_SAMPLE))
    assert np.array_equal(got["output_sample"][1:-1], flat[idx[1:-1]].astype(np.float32))
    for k in paths:
        assert os.path.basename(again[k]) == k + ".npy"
        assert np.array_equal(np.load(again[k]), got[k])
