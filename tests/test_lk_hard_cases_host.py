"""CPU test of the LK hard-case inputs (tests/lk_hard_cases.py): conditions on the INPUTS, met by the oracle alone.  The builders are only worth running on the
GPU if they reach the exits of lk_level and the sums they were built for; this holds them to that, and the committed census to its recomputation.  No GPU needed."""
import json
import os
import numpy as np
import lk_hard_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_leaves_the_lk_results_unchanged(oracle):
    """gfo_lk_census computes what gfo_lk computes, bit for bit (points, status, iteration count), on one thread and with the point loop on four; and every point
    has an exit at every level the call ran"""
    for c in L.cases():
        a = oracle.lk(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
        b = oracle.lk_census(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2], c["name"]
        levels = min(c["max_level"], 3 if c["prev"].shape == (L.H, L.W) else 2) + 1
        assert np.all(b[3][:, :levels] > 0) and np.all(b[3][:, levels:] == 0), c["name"]
        assert not np.any(b[4] & b[1]), "a re-checked point keeps no status"
    c = L.cases()[3]
    one = oracle.lk_census(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
    oracle.set_threads(4)
    try:
        four = oracle.lk_census(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
        plain = oracle.lk(c["prev"], c["next"], c["pts"], c["init"], max_level=c["max_level"])
    finally:
        oracle.set_threads(1)
    assert all(np.array_equal(x, y) for x, y in zip(one, four))
    assert np.array_equal(plain[0].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(plain[1], one[1]) and plain[2] == one[2]


def test_hard_cases_reach_every_exit_and_32_bit_sums_and_the_committed_census(oracle):
    """The bars: every exit of lk_level at level 0 and above it, the oscillation exit in the passes the tracker itself runs (max_level 1 from a predicted start),
    the bounds re-check, exact sums of 2^31 and more (a signed 32-bit total anywhere would wrap), neighbours in a wavefront that leave level 0 by different exits,
    and enough tracked points for the coordinate comparison to mean something.  profiles/lk_exit_census.json keeps the census, with the census of the inputs the
    suite had before beside it; it is recomputed here and compared exactly."""
    doc = L.census_document(oracle)
    f = doc["figures"]
    print(json.dumps(f))
    assert f["min_eig_level0"] >= 8 and f["min_eig_above_then_status_1"] >= 8
    assert f["template_out_level0"] >= 8 and f["template_out_above"] >= 8
    assert f["start_outside_level0"] >= 8 and f["start_outside_above"] >= 8
    assert f["left_image_level0"] >= 2 and f["left_image_above"] >= 2
    assert f["oscillation_level0"] >= 8 and f["oscillation_level1"] >= 8 and f["oscillation_level0_predicted_pass"] >= 4
    cap = f["max_count_by_level_3_2_1_0"]
    assert cap[3] >= 8 and sum(v >= 8 for v in cap[:3]) >= 2
    assert f["recheck"] >= 1
    assert f["max_abs_A"] >= 2 ** 31 and f["max_abs_b"] >= 2 ** 31
    ok4, n4 = f["groups_of_4_with_3_level0_exits"]
    ok2, n2 = f["groups_of_2_with_2_level0_exits"]
    assert 2 * ok4 >= n4 and 2 * ok2 >= n2
    assert 3 * f["status_1"] >= f["points"]
    # what the older inputs reach, for the record the file keeps: no eigenvalue rejection, no oscillation exit at levels 1 and 0, no re-check, sums below 2^29
    old = doc["test_lk_bit_exact_inputs"]["total"]
    assert old["exits_at_levels_3_2_1_0"]["min_eig"] == [0, 0, 0, 0] and old["exits_at_levels_3_2_1_0"]["oscillation"][2:] == [0, 0] and old["recheck"] == 0
    assert max(old["max_abs_A"], old["max_abs_b"]) < 2 ** 29
    with open(os.path.join(ROOT, "profiles", "lk_exit_census.json")) as fh:
        committed = json.load(fh)
    assert committed == json.loads(json.dumps(doc)), "profiles/lk_exit_census.json differs from its recomputation (python tests/lk_hard_cases.py rewrites it)"
