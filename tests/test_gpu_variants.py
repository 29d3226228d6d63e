"""The kernels behind the library's read-once switches.  ``VF_HIST_REPLICAS`` (1, 4, 16), ``VF_HIST_NT``,
``VF_HIST_BLOCKS``, ``VF_CLAHE_REPLICAS`` (1, 4), ``VF_CLAHE_HIST_WGS``, ``VF_CLAHE_APPLY_WGS`` and ``VF_LUT_LAYOUT=1``
select instantiations that are compiled into the shipped library and that any user can select; each is read once
into a function-local static, so each setting needs a process of its own.  The switches sit in different files
and do not interact, so three children cover them (``VARIANTS``).  A child (``tests/_variant_child.py``) runs the
comparisons of ``tests/_variant_cases.py``, every one exact against the numpy reference the kernel's own tests
use, and prints one JSON line.

The children run one at a time, each in a fresh process under a time limit of its own.  After a child that ended
by a signal, at its time limit or with a HIP error, the remaining variants fail without starting a process.

What the work-group switches do to CLAHE: ``VF_CLAHE_HIST_WGS=1`` gives one slice a tile, so on case a one
workgroup counts 20 rows in five ``kRows`` rounds; 100000 gives one row a slice on every case; ``VF_CLAHE_APPLY_WGS=1``
makes one strip a cell.  ``test_the_variants_are_what_they_are_chosen_for`` and ``test_the_switches_are_still_read``
need no GPU.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import _clahe_shapes as S
import _variant_cases as V

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "_variant_child.py")
TIMEOUT = 180  # seconds a child; one takes a few

VARIANTS = {
    "V1": dict(VF_HIST_REPLICAS=1, VF_HIST_NT=1, VF_CLAHE_REPLICAS=1, VF_LUT_LAYOUT=1, VF_CLAHE_HIST_WGS=1,
               VF_CLAHE_APPLY_WGS=1),
    "V2": dict(VF_HIST_REPLICAS=4, VF_CLAHE_REPLICAS=4, VF_HIST_BLOCKS=3, VF_CLAHE_HIST_WGS=100000,
               VF_CLAHE_APPLY_WGS=100000),
    "V3": dict(VF_HIST_REPLICAS=16, VF_HIST_NT=1, VF_CLAHE_HIST_WGS=7, VF_CLAHE_APPLY_WGS=50),
}
# the file that reads each switch
READ_BY = {"VF_HIST_REPLICAS": "vf_level.hip", "VF_HIST_NT": "vf_level.hip", "VF_HIST_BLOCKS": "vf_level.hip",
           "VF_CLAHE_REPLICAS": "vf_clahe.hip", "VF_CLAHE_HIST_WGS": "vf_clahe.hip", "VF_CLAHE_APPLY_WGS": "vf_clahe.hip",
           "VF_LUT_LAYOUT": "vf_lut.hip"}

_stop = []  # why no further child may start


def _source(name):
    return open(os.path.join(S.CSRC, name)).read()


def test_the_switches_are_still_read():
    """Nothing outside a process shows which instantiation ran, so this is the only guard against a renamed switch
    or a dropped branch turning a variant into a second run of the default: every variable a variant sets is still
    read, once, by the file it belongs to; ``vf_level.hip`` still maps 1, 4 and 16, and ``vf_clahe.hip`` 1 and 4, to
    an instantiation of their own; the nontemporal flag and the second table layout still select theirs."""
    assert {k for env in VARIANTS.values() for k in env} == set(READ_BY)
    for var, name in READ_BY.items():
        assert len(re.findall(r'static const \w+ \w+ = env_size\("%s",' % var, _source(name))) == 1, (var, name)
    level, clahe, lut = _source("vf_level.hip"), _source("vf_clahe.hip"), _source("vf_lut.hip")
    for r in (1, 4, 16):
        assert len(re.findall(r"case %d:\s*return launch_hist_nt<C3, %d>\(" % (r, r), level)) == 1, r
    assert re.search(r"default:\s*return launch_hist_nt<C3, kHistReplicas>\(", level)
    assert re.search(r"constexpr int kHistReplicas = 8;", level)  # none of 1, 4, 16: each variant leaves the default
    assert re.search(r'nt = env_size\("VF_HIST_NT", 0\) == 1;\s*return nt \? launch_hist_as<C3, R, true>\(', level)
    for r in (1, 4):
        assert len(re.findall(r"reps == %d\s*\? launch_hist_as<C3, %d>\(" % (r, r), clahe)) == 1, r
    assert re.search(r":\s*launch_hist_as<C3, kClaheReplicas>\(", clahe) and S.constants_in_the_sources()[4] == 8
    assert re.search(r'layout = env_size\("VF_LUT_LAYOUT", 0\) == 1 \? 1 : 0;', lut)
    assert re.search(r"if \(layout == 1\)\s*return c3 \? launch_lut_stream<true, 1>\(.*\n\s*: launch_lut_stream<false, 1>\(", lut)
    assert re.search(r"struct LutLds<1> \{\s*static constexpr int kWords = 768;", _source("vf_lut_lds.h"))


def test_the_variants_are_what_they_are_chosen_for():
    assert len(V.comparisons()) == V.EXPECTED == 58 and len({name for name, _ in V.comparisons()}) == 58
    a, b, c = (S.CASES[k] for k in "abc")
    # one workgroup a tile: on case a 20 rows in five rounds, on case c 37 rows in ten; one strip a cell
    one = S.plan(*a, 3, hist_wgs=1, apply_wgs=1)
    assert (one.slices, one.rows, S.rounds(one.rows), one.strips) == (1, 20, [4] * 5, 1)
    assert S.rounds(S.plan(*c, 3, hist_wgs=1).rows) == [4] * 9 + [1] and S.rounds(S.plan(*b, 1, hist_wgs=1).rows) == [4] * 5 + [1]
    # 100000: one row a slice, and as many strips as a tile has rows, most of them empty in the edge cells
    for case in (a, b, c):
        many = S.plan(*case, 1, hist_wgs=100000, apply_wgs=100000)
        assert (many.rows, many.slices, many.strips) == (1, many.th, many.th)
    # 7 and 50 are below the tiles and the cells of every case but a, where they give 2 slices of 10 rows and 6 strips
    assert [(p.slices, p.rows, p.strips) for p in (S.plan(*k, 1, hist_wgs=7, apply_wgs=50) for k in (a, b, c))] == \
        [(2, 10, 6), (1, 21, 1), (1, 37, 1)]
    assert S.strip_cut(10, 6) == ([2] * 5, 1) and S.strip_cut(20, 6) == ([4] * 5, 1)


def _run_child(name):
    if _stop:
        pytest.fail("not started: " + _stop[0])
    env = {k: v for k, v in os.environ.items() if k not in READ_BY}
    env.update({k: str(v) for k, v in VARIANTS[name].items()})
    try:
        done = subprocess.run([sys.executable, CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              timeout=TIMEOUT, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired as e:
        _stop.append("%s was killed at its time limit of %d s" % (name, TIMEOUT))
        pytest.fail(_stop[0] + "\n" + (e.stdout or b"").decode(errors="replace")[-2000:])
    text = done.stdout.decode(errors="replace")
    if done.returncode < 0:
        _stop.append("%s ended by signal %d" % (name, -done.returncode))
    elif re.search(r"hip ?error|HIP error|illegal memory access|hipError", text):
        _stop.append("%s reported a HIP error" % name)
    return done.returncode, text


@gpu
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant(name):
    status, text = _run_child(name)
    tail = text[-3000:]
    assert status == 0, (name, status, tail)
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (name, tail)
    result = json.loads(lines[0])
    assert result["failures"] == [] and result["stopped"] is None, (name, result)
    assert result["ran"] == V.EXPECTED, (name, result)
