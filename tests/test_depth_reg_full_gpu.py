"""Depth registration onto a PINHOLE_FULL colour camera on the device: gf_depth_register_batch_device_ex / gf_depth_register_batch_ex held byte for byte to the
numpy restatement of tests/depth_reg_full_ref.py (an eight-coefficient colour camera on 64 x 48 and on an odd-sized pitched frame with guard bytes, in one batch
with a PINHOLE entry and each alone; the PINHOLE entry's bytes are those of gf_depth_register_batch), and the tracker with a PINHOLE_FULL sequence fed raw depth
held in all eight fields to a handle without registration fed the frames registered beforehand.  There is no tolerance anywhere.  Run with -m gpu."""
import numpy as np
import pytest

import depth_reg_full_ref as full_ref
import depth_reg_ref as ref
import test_depth_reg_gpu as base

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def expected(c):
    """the restatement on a case, computed once and never changed"""
    if c["name"] not in _EXPECTED:
        out, census = full_ref.register(c["depth"], c["reg"], c["colour"], c["wc"], c["hc"])
        assert census["writes"] > 0.5 * c["depth"].size and census["multi_pixel"] > 0, "the case shows nothing"
        out.setflags(write=False)
        _EXPECTED[c["name"]] = out
    return _EXPECTED[c["name"]]


def cam_of(gf, col):
    if len(col) == 8:
        return gf.CameraModel.make(gf.CAMERA_PINHOLE, col[:4], col[4:])
    return gf.CameraModelEx.make(gf.CAMERA_PINHOLE_FULL, col[:4], col[4:])


def run_block(gf, cases, src_extra=0, dst_extra=0, offset=0):
    import torch
    src = [base.Plane(c["reg"]["width"], c["reg"]["height"], 2 * c["reg"]["width"] + src_extra, offset, c["depth"]) for c in cases]
    dst = [base.Plane(c["wc"], c["hc"], 2 * c["wc"] + dst_extra, offset, None, 0xC3) for c in cases]
    torch.cuda.synchronize()
    gf.depth_register_device([s.ref for s in src], [base.reg_of(gf, c["reg"]) for c in cases], [cam_of(gf, c["colour"]) for c in cases], [(c["wc"], c["hc"]) for c in cases],
                             [d.ref for d in dst])
    out = []
    for c, s, d in zip(cases, src, dst):
        frame, rest_ok = d.read()
        assert rest_ok, "%s: a byte outside the registered frame's rows was written" % c["name"]
        sf, s_ok = s.read()
        assert s_ok and np.array_equal(sf, c["depth"]), "%s: the source was written" % c["name"]
        out.append(frame)
    return out


def held(cases, frames, what):
    for c, f in zip(cases, frames):
        want = expected(c)
        assert np.array_equal(f, want), "%s, %s: %d of %d pixels differ from the restatement" % (what, c["name"], int((f != want).sum()), want.size)


def test_the_restatement_is_the_existing_one_but_for_the_projection():
    """a guard on the tests below, no evidence of the feature: the new restatement given the pinhole's projection is the existing restatement byte for byte, and
    with the PINHOLE_FULL projection it is not the one with the pinhole's first four coefficients, so the tests below can tell the two apart"""
    c = full_ref.cases()[0]
    pin, _ = ref.register(c["depth"], c["reg"], c["colour"][:8], c["wc"], c["hc"])
    own, _ = full_ref.register_with(ref.distort_to_plane, c["depth"], c["reg"], c["colour"][:8], c["wc"], c["hc"])
    assert np.array_equal(pin, own)
    assert (pin != expected(c)).mean() > 0.05


@pytest.mark.parametrize("src_extra,dst_extra,offset", [(0, 0, 0), (6, 10, 2)], ids=["tight", "pitched_with_guard_bytes"])
def test_block_equals_restatement_in_one_batch_and_alone(gf, src_extra, dst_extra, offset):
    """tight: dword loads and 16-byte stores where the sizes allow; (6, 10, 2): pitches that are odd multiples of 2 at byte 2, u16 loads and stores, with guard
    bytes behind every row and a guard frame behind every frame.  full_odd is 47 x 39 into 61 x 45."""
    cases = full_ref.cases()
    assert [len(c["colour"]) for c in cases] == [12, 8, 12]
    held(cases, run_block(gf, cases, src_extra, dst_extra, offset), "one batch of PINHOLE_FULL, PINHOLE, PINHOLE_FULL")
    for c in cases:
        held([c], run_block(gf, [c], src_extra, dst_extra, offset), "alone")
    held(cases[::-1], run_block(gf, cases[::-1], src_extra, dst_extra, offset), "reversed")


def test_pinhole_entry_keeps_the_bytes_of_the_old_call(gf):
    cases = full_ref.cases()
    regs, sizes = [base.reg_of(gf, c["reg"]) for c in cases], [(c["wc"], c["hc"]) for c in cases]
    wide = gf.depth_register([c["depth"] for c in cases], regs, [cam_of(gf, c["colour"]) for c in cases], sizes)      # gf_depth_register_batch_ex: a CameraModelEx among them
    held(cases, wide, "gf_depth_register_batch_ex")
    old = gf.depth_register([cases[1]["depth"]], [regs[1]], [cam_of(gf, cases[1]["colour"])], [sizes[1]])[0]          # gf_depth_register_batch
    assert np.array_equal(old, wide[1]) and np.array_equal(old, base.expected(ref.cases()[1]))
    alone = gf.depth_register([cases[1]["depth"]], [regs[1]], [gf.CameraModelEx.of(cam_of(gf, cases[1]["colour"]))], [sizes[1]])[0]   # the PINHOLE in the wide struct
    assert np.array_equal(old, alone)
    # every other model stays refused by name, in either struct; the old struct cannot say PINHOLE_FULL
    c = cases[0]
    for cam, word in ((gf.CameraModelEx.make("SCARAMUZZA", poly=[-60, 0, 1e-3], inv_poly=[90, 50], affine=[1, 0, 0, 32, 24]), "SCARAMUZZA"),
                      (gf.CameraModelEx.make("MEI", c["colour"][:4], xi=1.0), "MEI"), (gf.CameraModel.make(3, c["colour"][:4]), "model")):
        with pytest.raises(gf.GfError, match=word):
            gf.depth_register([c["depth"]], [regs[0]], [cam], [sizes[0]])


def test_tracker_registers_onto_a_pinhole_full_camera(gf):
    """sequence 0: a PINHOLE_FULL colour camera and a 128 x 96 depth camera in 0.25 mm counts; sequence 1: a PINHOLE with the identity registration; sequence 2:
    none.  Against a handle with the same cameras and no registration, fed the frames registered beforehand by the building block: ids, all eight fields of every
    observation and the states, through lists that skip and reorder."""
    W, H, K = base.W, base.H, base.K
    _, raw = base.tracker_inputs()
    r0, r1 = base.regs_of_tracker(W, H)
    colour0 = base.COLOUR + full_ref.KINECT8
    cam0 = cam_of(gf, colour0)
    raw_planes = [[base.Plane(r["width"], r["height"], None, 0, raw[b][k]) for k in range(K)] for b, r in ((0, r0), (1, r1))] + [[base.Plane(W, H, None, 0, raw[2][k]) for k in range(K)]]
    pre0, pre1 = [base.Plane(W, H) for _ in range(K)], [base.Plane(W, H) for _ in range(K)]
    gf.depth_register_device([p.ref for p in raw_planes[0]], [base.reg_of(gf, r0)] * K, [cam0] * K, [(W, H)] * K, [p.ref for p in pre0])
    gf.depth_register_device([p.ref for p in raw_planes[1]], [base.reg_of(gf, r1)] * K, [cam_of(gf, base.COLOUR + (0.0,) * 4)] * K, [(W, H)] * K, [p.ref for p in pre1])
    want0, _ = full_ref.register(raw[0][0], r0, colour0, W, H)
    assert np.array_equal(pre0[0].read()[0], want0) and (want0 != 0).mean() > 0.7

    def common(t):
        t.set_seq_camera(0, cam0)
        assert t.get_seq_camera(0, gf.CameraModelEx).as_dict() == cam0.as_dict()

    def with_reg(t):
        t.set_seq_depth_reg(0, base.reg_of(gf, r0))            # onto the PINHOLE_FULL camera set before it
        t.set_seq_depth_reg(1, base.reg_of(gf, r1))
        common(t)                                             # and the camera again, while the registration is set
        with pytest.raises(gf.GfError, match="SCARAMUZZA"):
            t.set_seq_camera(0, gf.CameraModelEx.make("SCARAMUZZA", poly=[-60, 0, 1e-3], inv_poly=[90, 50], affine=[1, 0, 0, 80, 60]))
        with pytest.raises(gf.GfError, match="KANNALA_BRANDT"):
            t.set_seq_camera(1, gf.CameraModel.make("KANNALA_BRANDT", [80.5, 81.25, 79.5, 59.5], [-0.01, 0, 0, 0]))

    a, st_a = base.drive(gf, raw_planes, lambda t: (common(t), with_reg(t)))
    b, st_b = base.drive(gf, [pre0, pre1, raw_planes[2]], common)
    base.same_run(a, b, "registered in the call against registered beforehand")
    calls = sum(1 for L in base.LISTS if 0 in L or 1 in L)
    assert st_a["launches"] == 2 * calls and st_a["frames"] == sum((0 in L) + (1 in L) for L in base.LISTS)      # two launches per call whatever the mix
    assert st_b == {"launches": 0, "frames": 0, "kernel_ms": 0.0}
    depths = np.concatenate([res[i][1][:, 7] for (res, _), L in zip(a, base.LISTS) for i, s in enumerate(L) if s == 0])
    assert len(depths) > 50 and (depths > 0).mean() > 0.5, "sequence 0 reports no depths: the test would show nothing"
    # the pairs of sequence 0 are PINHOLE_FULL's: the building block's bits on the reported pixels
    res, _ = a[0]
    obs = res[base.LISTS[0].index(0)][1]
    blk = gf.camera_lift([cam0], [obs[:, 3:5]], rays=False)[0][0]
    assert np.array_equal(obs[:, 0:2].astype(np.float32).view(np.uint32), blk.view(np.uint32))
