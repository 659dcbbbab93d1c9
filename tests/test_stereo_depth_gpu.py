"""stereo_depth_kernel through gf_stereo_depth_batch / _batch_device against the numpy restatement of tests/stereo_depth_ref.py, bit for bit in depth_mm and why:
the cases of the CPU test (every reason code, both sides of every gate, every model without transcendentals on either eye) as one batch and one set at a time;
sets of 0, 1, 63, 64, 65 and 130 matches, an empty set between full ones and a set behind a longer one; output rows between guard bytes; two runs the same bytes;
KANNALA_BRANDT to a count.  Run with -m gpu."""
import numpy as np
import pytest

import stereo_depth_ref as ref

pytestmark = pytest.mark.gpu

GUARD8, GUARD16 = 0xA7, 0xA7A7


@pytest.fixture(scope="module")
def expected():
    return {c["name"]: ref.depth(c["left"], c["right"], c["cfg"], c["lu"], c["ru"], c["st"]) for c in ref.cases() + [ref.kb_case()]}


def _args(cs):
    return ([ref.gf(c["left"]) for c in cs], [ref.gf(c["right"]) for c in cs], [ref.gf_cfg(c["cfg"]) for c in cs], [c["lu"] for c in cs], [c["ru"] for c in cs], [c["st"] for c in cs])


def _same(cs, mm, why, expected):
    for c, m, w in zip(cs, mm, why):
        want_mm, want_why = expected[c["name"]]
        assert np.array_equal(w, want_why), "%s: reasons differ at %s: %s, the restatement's %s" % (c["name"], np.nonzero(w != want_why)[0][:8], w[w != want_why][:8], want_why[w != want_why][:8])
        assert np.array_equal(m, want_mm), "%s: depths differ at %s" % (c["name"], np.nonzero(m != want_mm)[0][:8])


def test_one_batch_equals_the_restatement_and_the_host_form(gf, expected):
    cs = ref.cases()
    mm, why = gf.stereo_depth(*_args(cs))
    _same(cs, mm, why, expected)
    total = {k: sum(int((w == v).sum()) for w in why) for k, v in ref.WHY.items()}
    assert all(v >= 2 for v in total.values()), total                     # the device reached every reason code
    hm, hw = gf.stereo_depth_host(*_args(cs))
    assert all(np.array_equal(a, b) for a, b in zip(mm, hm)) and all(np.array_equal(a, b) for a, b in zip(why, hw))


def test_one_set_at_a_time(gf, expected):
    for c in ref.cases():
        mm, why = gf.stereo_depth(*_args([c]))
        _same([c], mm, why, expected)


def test_device_tables_between_guards_and_twice_the_same_bytes(gf, expected):
    """the edge sets in the order 64, 0, 130, 1, 63, 65 through gf_stereo_depth_batch_device: the output rows lie between guard bytes, which survive, and a second
    run leaves the same bytes"""
    import torch
    cs = [c for c in ref.cases() if c["name"].startswith("edge_")]
    counts = [len(c["lu"]) for c in cs]
    assert counts == [64, 0, 130, 1, 63, 65]
    n, lead = sum(counts), 37
    cat = lambda k, t: torch.from_numpy(np.ascontiguousarray(np.concatenate([c[k] for c in cs]), t)).cuda()
    d_l, d_r, d_st = cat("lu", np.float32), cat("ru", np.float32), cat("st", np.uint8)
    runs = []
    for _ in range(2):
        d_mm = torch.from_numpy(np.full(lead + n + 51, GUARD16, np.uint16).view(np.int16)).cuda()
        d_why = torch.from_numpy(np.full(lead + n + 51, GUARD8, np.uint8)).cuda()
        gf.stereo_depth_device([ref.gf(c["left"]) for c in cs], [ref.gf(c["right"]) for c in cs], [ref.gf_cfg(c["cfg"]) for c in cs], counts, d_l.data_ptr(), d_r.data_ptr(),
                               d_st.data_ptr(), d_mm.data_ptr() + 2 * lead, d_why.data_ptr() + lead)
        torch.cuda.synchronize()
        runs.append((d_mm.cpu().numpy().view(np.uint16), d_why.cpu().numpy()))
    mm, why = runs[0]
    assert (mm[:lead] == GUARD16).all() and (mm[lead + n:] == GUARD16).all() and (why[:lead] == GUARD8).all() and (why[lead + n:] == GUARD8).all()
    first = np.concatenate([[0], np.cumsum(counts)])
    _same(cs, [mm[lead + first[b]:lead + first[b + 1]] for b in range(len(cs))], [why[lead + first[b]:lead + first[b + 1]] for b in range(len(cs))], expected)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


def test_kannala_brandt_to_a_count(gf, expected):
    c = ref.kb_case()
    (mm,), (why,) = gf.stereo_depth(*_args([c]))
    want_mm, want_why = expected["kb"]
    far = ~ref.near_a_gate(c)
    assert far.sum() >= 0.9 * len(far) and np.array_equal(why[far], want_why[far])
    both = (why == ref.WHY["ok"]) & (want_why == ref.WHY["ok"])
    assert both.sum() >= 20 and np.abs(mm[both].astype(np.int64) - want_mm[both].astype(np.int64)).max() <= 1


def test_refusals_launch_nothing(gf):
    c = ref.cases()[0]
    bad = dict(c["cfg"], max_depth=70.0)
    with pytest.raises(gf.GfError, match="65.535"):
        gf.stereo_depth([ref.gf(c["left"])], [ref.gf(c["right"])], [ref.gf_cfg(bad)], [c["lu"]], [c["ru"]], [c["st"]])
