"""A frame size per sequence without a GPU: the header's declarations, gfamd's binding, the exported names, and tests/native/seq_size_host.cpp -- the limits of
gf_tracker_set_seq_size, the table of sizes in force and the plan of a call with sizes (gf_seq_size.hpp) in a stand-alone host program under the address and
undefined-behaviour sanitizers, its plans held against a restatement here and its geometry against test_tracker_sizes_gpu.levels()."""
import itertools
import os
import re
import subprocess

import pytest

from test_tracker_sizes_gpu import SIZES, levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "groundfusion_hip.h")
NAMES = ("gf_tracker_set_seq_size", "gf_tracker_get_seq_size")
MAX_SIZES = 8
M64 = (1 << 64) - 1


def test_header_declares_the_entry_points_behind_their_citation():
    header = open(HEADER).read()
    for fn in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define GF_MAX_SEQ_SIZES 8\s*)?^int %s\(" % fn, header, re.S | re.M)
        assert m, "%s is not declared behind a comment" % fn
        assert "feature_tracker.cpp:108-109" in m.group(1), "%s: the comment in front of it does not cite feature_tracker.cpp:108-109" % fn
    assert re.search(r"^#define GF_MAX_SEQ_SIZES 8$", header, re.M)
    assert re.search(r"^int gf_tracker_set_seq_size\(gf_tracker\* h, int seq, int width, int height\);", header, re.M)
    assert re.search(r"^int gf_tracker_get_seq_size\(gf_tracker\* h, int seq, int\* width, int\* height\);", header, re.M)


def test_names_are_exported_and_in_the_library():
    import gfamd
    lib = gfamd.lib()
    for name in NAMES:
        assert name in gfamd.EXPORTS and hasattr(lib, name), name
    assert gfamd.MAX_SEQ_SIZES == MAX_SIZES
    for name in ("set_seq_size", "get_seq_size", "seq_size", "device_size_offsets"):
        assert hasattr(gfamd.FeatureTracker, name), name


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "groundfusion_hip.h"\nint main(void) { int (*set)(gf_tracker*, int, int, int) = gf_tracker_set_seq_size; '
                   'int (*get)(gf_tracker*, int, int*, int*) = gf_tracker_get_seq_size; return (set && get ? 0 : 1) + GF_MAX_SEQ_SIZES - 8; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", "-o", str(tmp_path / "c99.o"), str(src)])


# ---- the plan of a call, restated: sizes[row] = (w, h), row_of[seq]
def plan(sizes, row_of, seq, bpp=None):
    p = {"row": [row_of[q] for q in seq]}
    p["wh"] = [sizes[r] for r in p["row"]]
    px = [w * h for w, h in p["wh"]]
    scale = bpp or [1] * len(seq)
    p["gray_off"] = [sum(a * b for a, b in zip(px[:i], scale)) for i in range(len(seq))]
    p["depth_off"] = [2 * sum(px[:i]) for i in range(len(seq))]
    p["mask_off"] = [sum(px[:i]) for i in range(len(seq))]
    p["bytes"] = (sum(a * b for a, b in zip(px, scale)), 2 * sum(px), sum(px))
    p["sized"] = int(any(r != 0 for r in p["row"]))
    p["max"] = (max([w for w, _ in p["wh"]] + [0]), max([h for _, h in p["wh"]] + [0]))
    rows = list(dict.fromkeys(p["row"]))                       # distinct, in the order of their first appearance
    members = [[i for i, r in enumerate(p["row"]) if r == g] for g in rows]
    p["groups"] = [(g, sum(len(m) for m in members[:k]), len(members[k])) for k, g in enumerate(rows)]
    p["member"] = [i for m in members for i in m]
    return p


def digest_of(plans):
    d = 14695981039346656037
    for p in plans:
        n = len(p["row"])
        vals = [n, p["sized"], p["max"][0], p["max"][1], p["bytes"][0], p["bytes"][1], p["bytes"][2], len(p["groups"])]
        for i in range(n):
            vals += [p["row"][i], p["wh"][i][0], p["wh"][i][1], p["gray_off"][i], p["depth_off"][i], p["mask_off"][i], p["member"][i]]
        for g in p["groups"]:
            vals += list(g)
        for v in vals:
            d = ((d ^ v) * 1099511628211) & M64
    return d


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seq_size") / "seq_size_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "seq_size_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_limits_tables_and_plans_under_the_sanitizers(host_output):
    assert "all: ok" in host_output and host_output.count(": ok") == 5
    for part in ("limits", "geometry", "orders", "lists"):
        assert re.search(r"^%s: ok" % part, host_output, re.M), part
    assert "(%d plans)" % sum(len(list(itertools.permutations(range(n)))) for n in range(1, 9)) in host_output


def test_geometry_of_every_size_is_build_geom(host_output):
    """each size's geometry against levels(), test_tracker_sizes_gpu's restatement of build_geom; every size of SIZES fits the slot of every size that dominates it"""
    rows = [list(map(int, l.split()[1:])) for l in host_output.splitlines() if l.startswith("geom ")]
    assert [(r[0], r[1]) for r in rows] == [(c[0], c[1]) for c in SIZES]
    for r, case in zip(rows, SIZES):
        lv, img_bytes = levels(r[0], r[1])
        assert r[2] == len(lv) == case[2] and r[3] == img_bytes, r
        assert [tuple(r[4 + 4 * k:8 + 4 * k]) for k in range(r[2])] == lv, r
    dominated = [(a, b) for a in SIZES for b in SIZES if b[0] <= a[0] and b[1] <= a[1]]
    assert all(levels(b[0], b[1])[1] <= levels(a[0], a[1])[1] for a, b in dominated)
    assert "fits %d\n" % len(dominated) in host_output


def test_plans_of_every_order_of_one_to_eight_sizes(host_output):
    """lists of 1 .. 8 sizes in every order: the program's digest of its plans is the digest of the plans restated here"""
    pick = [(2560, 1440), (640, 480), (1280, 720), (640, 160), (644, 481), (320, 240), (64, 48), (40, 36)]
    found = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^orders (\d+) (\d+) (\d+)$", host_output, re.M)}
    assert sorted(found) == list(range(1, 9))
    for n in range(1, 9):
        perms = list(itertools.permutations(range(n)))   # lexicographic, as std::next_permutation walks them
        assert found[n] == (len(perms), digest_of(plan(pick, list(range(n)), s) for s in perms)), n


def test_named_lists_in_full(host_output):
    """one size only, every position a different size, a reversed list, two small sequences beside a large one: every table of the plan, number for number"""
    sizes = [(644, 481), (640, 480), (640, 160), (320, 240), (64, 48), (40, 36)]
    row_of = [0, 1, 2, 3, 4, 5, 4, 4]
    seen = set()
    for line in host_output.splitlines():
        if not line.startswith("plan "):
            continue
        head, meta, row, off, groups, member = [x.split() for x in line.split("|")]
        name, seq = head[1], list(map(int, head[3:]))
        p = plan(sizes, row_of, seq)
        assert [int(meta[1]), (int(meta[3]), int(meta[4])), tuple(map(int, meta[6:9]))] == [p["sized"], p["max"], p["bytes"]], name
        assert list(map(int, row[1:])) == p["row"], name
        o = list(map(int, off[1:]))
        assert (o[0::3], o[1::3], o[2::3]) == (p["gray_off"], p["depth_off"], p["mask_off"]), name
        g = list(map(int, groups[1:]))
        assert list(zip(g[0::3], g[1::3], g[2::3])) == p["groups"], name
        assert list(map(int, member[1:])) == p["member"], name
        seen.add(name)
    assert seen == {"all", "reverse", "two", "own_only", "one_size", "small_small_large", "different", "empty"}
    # what the restatement itself says about the named shapes
    assert plan(sizes, row_of, [0])["sized"] == 0 and plan(sizes, row_of, [6, 4, 7])["groups"] == [(4, 0, 3)]
    assert plan(sizes, row_of, [4, 0, 7])["member"] == [0, 2, 1] and len(plan(sizes, row_of, [3, 0, 5, 1, 4, 2])["groups"]) == 6
