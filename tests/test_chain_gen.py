"""The generated programs of ``tests/_chain_gen.py`` are worth running: the draw is deterministic,
every program is valid by the rules of ``vf_chain_plan.h``'s ``validate()`` (transcribed here; the
library's own verdict is ``tests/test_chain_plan.py``'s), every feature that the hand-written twelve
of ``tests/_chain_ref.py`` lack is held by at least one program, and the reference outputs stay
pictures: at most 8 of the 64 have fewer than 16 distinct values on the 40 x 175 x 3 noise frame.
The features that need the plan (folding, buffers) are in ``tests/test_chain_plan.py``.
"""
import collections

import numpy as np
import pytest

import _chain_gen as G
import _chain_ref as CR

SETS = [(3, G.PROGRAMS), (1, G.PROGRAMS_1)]


def _counts(progs):
    cnt = collections.Counter()
    for name in G.GENERATED:
        cnt.update(G.features(progs[name]))
    return cnt


def test_the_draw_is_deterministic_and_the_sets_have_their_size():
    for channels, progs in SETS:
        assert len(G.GENERATED) == 64 and all(n in progs for n in G.GENERATED)
        assert len(progs) > 64  # and the hand-written ones
        for seed in (0, 17, 63):
            again = G.generate(seed, channels)
            first = progs["g%02d" % seed]
            assert len(again) == len(first)
            for x, y in zip(again, first):
                assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert any(len(G.PROGRAMS[n]) != len(G.PROGRAMS_1[n]) for n in G.GENERATED)  # the channels seed the draw


@pytest.mark.parametrize("channels,progs", SETS)
def test_every_program_is_valid(channels, progs):
    for name, prog in progs.items():
        n = len(prog)
        assert 1 <= n <= CR.MAX_STEPS, name
        read = set()
        for i, st in enumerate(prog, 1):
            ops = G.operands(st)
            assert all(0 <= v < i for v in ops), (name, i)
            read.update(ops)
            if st[0] == "table":
                t = np.asarray(st[2])
                assert t.dtype == np.uint8 and t.shape in ((256,), (256, 3)), (name, i)
                assert t.ndim == 1 or channels == 3, (name, i)
                for col in t.reshape(256, -1).T:
                    assert np.array_equal(np.sort(col), np.arange(256)), (name, i, "not a permutation")
            elif st[0] == "conv":
                k = np.asarray(st[2])
                assert k.shape[0] in G.SIDES and k.shape[1] in G.SIDES and 0 <= st[3] <= 8, (name, i)
                assert int(k.sum()) == 1 << st[3] and st[4] in CR.BORDERS, (name, i)
                assert int(np.abs(k).sum()) <= 65536 and np.abs(k).max() <= 32767, (name, i)
            elif st[0] == "rank":
                if st[2] == "median":
                    assert st[3] in (3, 5) and st[4] == "replicate", (name, i)
                else:
                    e = np.asarray(st[3])
                    assert st[2] in ("erode", "dilate") and e.shape[0] in G.SIDES and e.shape[1] in G.SIDES, (name, i)
                    assert e.any() and set(np.unique(e)) <= {0, 1} and st[4] in CR.BORDERS, (name, i)
            else:
                assert st[0] == "bin" and st[1] in G.BIN_OPS, (name, i)
                assert st[2] != st[3] or st[1] in G.SAME_OPERAND_OPS, (name, i)
        assert read == set(range(n)), (name, "a dead value")  # every value but the last is read


@pytest.mark.parametrize("channels,progs", SETS)
def test_the_generated_programs_hold_every_named_feature(channels, progs):
    cnt = _counts(progs)
    for feature in ("same_operand", "shared_with_neighbourhood", "two_neighbourhood_readers_of_different_kh",
                    "wider_than_tall", "taller_than_wide", "one_row", "mixed_borders", "neighbourhood_without_reach",
                    "length_1", "length_8", "narrow_form", "wide_form", "ends_with_neighbourhood", "ends_with_table",
                    "ends_with_bin", "table_with_two_readers", "tables_fold") + tuple("op_" + op for op in G.BIN_OPS):
        assert cnt[feature] >= 1, (channels, feature, sorted(cnt.items()))
    # no rare accidents: the features the band and JPEG tests select by are common
    assert cnt["wider_than_tall"] >= 16 and cnt["one_row"] >= 8 and cnt["mixed_borders"] >= 16, sorted(cnt.items())
    assert cnt["same_operand"] >= 8 and cnt["shared_with_neighbourhood"] >= 16, sorted(cnt.items())
    assert all(cnt["length_%d" % n] >= 1 for n in range(1, CR.MAX_STEPS + 1)), sorted(cnt.items())


def test_the_hand_written_programs_hold_what_they_are_there_for():
    for channels, progs in SETS:
        f = {n: G.features(p) for n, p in progs.items() if n.startswith("x_")}
        assert "table_with_two_readers" in f["x_table_two_readers"]
        assert "tables_fold" in f["x_tables_fold"] and ("tables_fold_3_then_1" in f["x_tables_fold"]) == (channels == 3)
        for name in ("x_separable", "x_separable_rank"):
            assert {"one_row", "taller_than_wide", "mixed_borders", "ends_with_neighbourhood"} <= f[name]
        assert {"two_neighbourhood_readers_of_different_kh", "ends_with_table"} <= f["x_two_readers"]
        assert "op_subtract" in f["x_subtract_over_b"] and G.readers(progs["x_subtract_over_b"], 1) == [3, 4]


def test_the_reference_outputs_stay_pictures():
    """A condition of the set, not a measurement: at most 8 of the 64 reference outputs on
    ``CR.noise(40, 175, 3)`` have fewer than 16 distinct values.  This draw has 3: g06, g18 and g39,
    where successive erosions of noise, or a difference of a value with its own erosion, run into 0."""
    img = CR.noise(40, 175, 3)
    distinct = {n: len(np.unique(CR.run(img, G.PROGRAMS[n]))) for n in G.GENERATED}
    few = sorted(n for n, d in distinct.items() if d < 16)
    assert len(few) <= 8, (few, [distinct[n] for n in few])
    gray = CR.noise(13, 17, 1)
    assert sum(len(np.unique(CR.run(gray, G.PROGRAMS_1[n]))) < 16 for n in G.GENERATED) <= 8
