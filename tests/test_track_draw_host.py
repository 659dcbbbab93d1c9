"""The track image's shared code (csrc/gf_track_draw.hpp) without a GPU: tests/native/track_draw_host.cpp checks the literals of the definition, the binning
function and the builder's refusals, and renders whole frames on the CPU by the per-pixel function the kernel walks; here those frames are compared byte for
byte with tests/track_draw_ref.py, the definition restated in Python.  The program is built twice, plain and with -fsanitize=address,undefined: a stand-alone
program, nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import track_draw_ref as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def prog(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("track_draw_host_" + request.param) / "track_draw_host"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                          ["-o", str(out), os.path.join(ROOT, "tests", "native", "track_draw_host.cpp")])
    return str(out)


def test_literals_binning_and_refusals(prog):
    r = subprocess.run([prog, "selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _render(prog, tmp_path, gray, cur, cnt, prev, has):
    h, w = gray.shape
    n = len(cnt)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, n], np.int32).tobytes() + gray.tobytes() + np.ascontiguousarray(cur, np.float32).tobytes() + np.ascontiguousarray(cnt, np.int32).tobytes() +
                np.ascontiguousarray(prev, np.float32).tobytes() + np.ascontiguousarray(has, np.uint8).tobytes())
    r = subprocess.run([prog, "render", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(dst, np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("seed,w,h,n", [(1, 67, 45, 40), (2, 64, 48, 120), (3, 33, 90, 0), (4, 130, 37, 60)])
def test_whole_frames_equal_the_python_restatement(prog, tmp_path, seed, w, h, n):
    rng = np.random.default_rng(seed)
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cur, cnt, prev, has = TD.random_lists(rng, n, w, h, reach=25.0)
    want, by_index, by_green, margin = TD.render(gray, cur, cnt, prev, has, with_rules=True)
    assert margin > 1e-9, "an arrow tip within 1e-9 of a tie of lrint"
    got = _render(prog, tmp_path, gray, cur, cnt, prev, has)
    assert np.array_equal(got, want), "%d pixels differ" % (got != want).any(2).sum()
    if n >= 40:
        assert by_index > 0 and by_green > 0   # both rules of the order decided pixels


def test_the_worked_example_in_the_python_restatement():
    """the same literals on the other side, so that header and restatement do not only agree with each other"""
    gray = np.full((24, 32), 7, np.uint8)
    img = TD.render(gray, [(15, 10)], [1], [(5, 10)], [True])
    green = (img == TD.GREEN).all(2)
    want = np.zeros_like(green)
    want[9:12, 4:17] = True
    want[8, 5:8] = want[12, 5:8] = True
    want_dot = TD.dot_mask(15, 10, 32, 24) & ~want
    assert TD.tips((15, 10), (5, 10))[:2] == ((6, 11), (6, 9))
    assert green.sum() == 45 and np.array_equal(green, want)
    assert (img[want_dot] == (242, 0, 13)).all() and (img[~want & ~want_dot] == 7).all()
    assert (TD.render(gray, [(9, 9)], [1], [(9, 9)], [True]) == TD.GREEN).all(2).sum() == 9
    assert TD.dot_mask(10, 10, 21, 21).sum() == 81
    assert [int(round(255 * (1 - min(1.0, k / 20.)))) for k in range(21)] == list(TD.C0) and [int(round(255 * min(1.0, k / 20.))) for k in range(21)] == list(TD.C2)
    assert 255 * (1 - 14 / 20.) == 76.50000000000001 and 255 * (1 - 18 / 20.) == 25.499999999999993
