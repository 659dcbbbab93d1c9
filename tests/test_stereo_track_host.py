"""The stereo stage of the tracker's host bookkeeping without a GPU: tests/native/stereo_track_host.cpp is a CPU tracker made of the stage functions of
csrc/gf_track_host.hpp (after_detect with stereo_stage at the reference's place, the right-hand packing) with the oracle's LK in the place of the kernels, the
left-to-right pass as stereo_lk_body runs it.  It is held to the restatement of tests/stereo_ref.py bit for bit after every frame: ids, camera ids, all eight
fields, n_out, the left state and the right-hand state.  A stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import roi_ref as RR
import stereo_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGHT_PROJ, RIGHT_DIST, stamp = SR.RIGHT_PROJ, SR.RIGHT_DIST, SR.stamp   # the program computes the same stamps
OBS = np.dtype([("id", "<i4"), ("cam", "<i4"), ("v", "<f8", 8)])
MAP = np.dtype([("id", "<i4"), ("p", "<f4", 2)])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("stereo_track_host") / "stereo_track_host"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]   # the oracle's own: -ffp-contract=off -fno-fast-math decide its bits
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(out), os.path.join(ROOT, "tests", "native", "stereo_track_host.cpp"),
                           os.path.join(ROOT, "oracle", "tracker_oracle.cpp")])
    return str(out)


def _run(exe, tmp_path, case, flow_back, has_right, opts=()):
    w, h, max_cnt, min_dist = case
    left, right = SR.scene(w, h)
    frames, dump = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(frames, "wb") as f:
        f.write(np.array([w, h, SR.K], np.int32).tobytes())
        f.write(np.stack(left).tobytes())
        f.write(np.stack(right).tobytes())
        f.write(np.asarray(has_right, np.uint8).tobytes())
    args = [exe, str(frames), str(dump), str(max_cnt), str(min_dist), str(flow_back)] + [float(v).hex() for v in RIGHT_PROJ + RIGHT_DIST] + list(opts)
    out = subprocess.run(args, capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout
    return open(dump, "rb").read(), out.stdout


def _take(raw, at, dtype, n):
    a = np.frombuffer(raw, dtype, n, at)
    return a, at + n * np.dtype(dtype).itemsize


def _hold(oracle, raw, case, flow_back, has_right, remove_at=-1, reset_at=-1):
    """every frame of the program's file against the restatement; returns the restatement's tracker and the right observations per frame"""
    w, h, max_cnt, min_dist = case
    left, right = SR.scene(w, h)
    ref = SR.Tracker(oracle, max_cnt, min_dist, flow_back, lambda p: SR.pinhole_lift(RIGHT_PROJ, RIGHT_DIST, p))
    census = dict(ref.census)
    at, rights = 0, []
    for k in range(SR.K):
        if k == reset_at:
            for key in census:
                census[key] += ref.census[key]
            ref.reset()
        ids, cam, obs = ref.track(stamp(k), left[k], right[k] if has_right[k] else None)
        (n,), at = _take(raw, at, "<i4", 1)
        rec, at = _take(raw, at, OBS, int(n))
        what = "frame %d" % k
        assert n == len(ids), "%s: n_out %d, the restatement's %d" % (what, n, len(ids))
        assert np.array_equal(rec["id"], ids) and np.array_equal(rec["cam"], cam), "%s: ids or camera ids differ" % what
        assert np.array_equal(rec["v"].view(np.uint64), np.ascontiguousarray(obs).view(np.uint64)), "%s: observations differ" % what
        sids, scnt, spts = ref.state()
        (m,), at = _take(raw, at, "<i4", 1)
        gids, at = _take(raw, at, "<i4", int(m)); gcnt, at = _take(raw, at, "<i4", int(m)); gpts, at = _take(raw, at, "<f4", 2 * int(m))
        assert np.array_equal(gids, sids) and np.array_equal(gcnt, scnt) and np.array_equal(gpts.view(np.uint32), spts.reshape(-1).view(np.uint32)), "%s: left state differs" % what
        (r,), at = _take(raw, at, "<i4", 1)
        rids, at = _take(raw, at, "<i4", int(r)); rpts, at = _take(raw, at, "<f4", 2 * int(r))
        assert np.array_equal(rids, ref.ids_right) and np.array_equal(rpts.view(np.uint32), ref.cur_right_pts.reshape(-1).view(np.uint32)), "%s: right-hand lists differ" % what
        (q,), at = _take(raw, at, "<i4", 1)
        pm, at = _take(raw, at, MAP, int(q))
        want = sorted(ref.prev_un_right_pts_map.items())
        assert [int(i) for i in pm["id"]] == [i for i, _ in want], "%s: prev_un_right_pts_map holds other ids" % what
        if q:
            assert np.array_equal(pm["p"].view(np.uint32), np.stack([p for _, p in want]).view(np.uint32)), "%s: prev_un_right_pts_map differs" % what
        rights.append((ids[cam == 1], obs[cam == 1]))
        if k == remove_at:
            ref.remove_outliers([int(i) for i in sids if i % 7 == 3])
    assert at == len(raw)
    for key in census:
        census[key] += ref.census[key]
    return census, rights


ALL = [1] * SR.K
_CENSUS = {}


@pytest.mark.parametrize("flow_back", [0, 1])
@pytest.mark.parametrize("case", SR.CASES, ids=RR.size_id)
def test_stage_is_the_restatement(exe, oracle, tmp_path, case, flow_back):
    raw, _ = _run(exe, tmp_path, case, flow_back, ALL)
    census, rights = _hold(oracle, raw, case, flow_back, ALL)
    print(RR.size_id(case), "flow_back", flow_back, census)
    assert census["points"] == SR.K * case[2]
    assert 4 * census["kept"] >= census["points"], census
    assert sum(len(i) for i, _ in rights) == census["kept"]
    moving = sum(int((o[:, 5:7] != 0).any(axis=1).sum()) for _, o in rights[1:])
    assert moving > census["kept"] // 4, "hardly any right velocity is non-zero"
    if flow_back:
        _CENSUS[case] = census
        assert census["points"] - census["fwd_fail"] - census["rev_fail"] - census["border"] - census["distance_alone"] == census["kept"]
    else:
        assert census["kept"] == census["points"] - census["fwd_fail"]
        w, h = case[:2]
        outside = sum(int((~SR.in_border(o[:, 3:5].astype(np.float32), w, h)).sum()) for _, o in rights)
        print("right points kept outside the border:", outside)


def test_every_rejection_reason_occurs(exe, oracle, tmp_path):
    """over 132 x 97 and 64 x 61 together with FLOW_BACK, each of the four terms of the conjunction rejects at least one point"""
    for case in SR.CASES:
        if case not in _CENSUS:
            raw, _ = _run(exe, tmp_path, case, 1, ALL)
            _CENSUS[case] = _hold(oracle, raw, case, 1, ALL)[0]
    total = {k: sum(_CENSUS[c][k] for c in SR.CASES) for k in _CENSUS[SR.CASES[0]]}
    print(total)
    for reason in ("fwd_fail", "rev_fail", "border", "distance_alone"):
        assert total[reason] >= 1, (reason, total)


def test_a_frame_without_a_right_image(exe, oracle, tmp_path):
    """frame 3 comes without its right image: the stage is skipped, the right-hand state stays, and frame 4 takes its velocities against frame 2's map over the
    newest dt -- at least one of them is non-zero, and the restatement (which keeps the stale map) gives the same bits"""
    has = [1, 1, 1, 0, 1, 1]
    case = SR.CASES[0]
    raw, _ = _run(exe, tmp_path, case, 1, has)
    _, rights = _hold(oracle, raw, case, 1, has)
    assert len(rights[3][0]) == 0
    assert (rights[4][1][:, 5:7] != 0).any(), "no right velocity is non-zero on the frame behind the gap"


def test_remove_outliers_between_frames(exe, oracle, tmp_path):
    case = SR.CASES[0]
    raw, out = _run(exe, tmp_path, case, 1, ALL, ["remove=2"])
    assert "removeOutliers behind frame 2: 0 ids" not in out
    _hold(oracle, raw, case, 1, ALL, remove_at=2)


def test_reset(exe, oracle, tmp_path):
    case = SR.CASES[0]
    raw, _ = _run(exe, tmp_path, case, 1, ALL, ["reset=3"])
    _, rights = _hold(oracle, raw, case, 1, ALL, reset_at=3)
    assert len(rights[3][0]) > 0 and not (rights[3][1][:, 5:7] != 0).any(), "the frame behind a reset has right velocities"


def test_output_one_short_of_both_eyes(exe, oracle, tmp_path):
    case = SR.CASES[0]
    raw, out = _run(exe, tmp_path, case, 1, ALL, ["short=4"])
    assert "short output:" in out
    _hold(oracle, raw, case, 1, ALL)


def test_scene_recipe():
    w, h = SR.CASES[0][:2]
    left, right = SR.scene(w, h)
    L, R = left[2], right[2]
    assert np.array_equal(R[0:5, :w - 3], L[0:5, 3:]) and np.array_equal(R[h - 5:, :w - 12], L[h - 5:, 12:])
    assert (R[h // 2 - 8:h // 2 + 8, w // 2 - 10:w // 2 + 10] == 128).all() and not np.array_equal(right[2], right[3])
