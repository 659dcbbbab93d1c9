"""The per-sequence tracker parameters without a GPU: gfamd's ctypes mirror of gf_tracker_seq_cfg against the header, and tests/native/seq_cfg_host.hip -- the
limits of gf_tracker_set_seq_cfg and the circle tables of gf_seq_cfg.hpp in a stand-alone host program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "double": C.c_double}


def _struct_fields(header, name):
    """[(field, C type name)] of `typedef struct name { ... } name;`, in the order of the header"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_ctypes_mirror_of_the_header():
    import gfamd
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    fields = _struct_fields(header, "gf_tracker_seq_cfg")
    assert len(fields) == 12
    assert [(n, CTYPES[t]) for n, t in fields] == list(gfamd.TrackerSeqCfg._fields_)
    # the twelve values are the oracle's TrackerCfg, and the handle's cfg carries every one of them under the same name
    import oracle_py
    assert list(gfamd.TrackerSeqCfg._fields_) == list(oracle_py.TrackerCfg._fields_)
    handle = dict(gfamd.TrackerCfg._fields_)
    assert all(handle[n] is t for n, t in gfamd.TrackerSeqCfg._fields_)
    for fn in ("gf_tracker_set_seq_cfg", "gf_tracker_get_seq_cfg", "gf_tracker_reset_seq", "gf_estimator_group_create_each"):
        assert re.search(r"^int %s\(" % fn, header, re.M), fn


def test_limits_and_circle_tables_under_the_sanitizers(tmp_path):
    exe = tmp_path / "seq_cfg_host"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "native", "seq_cfg_host.hip")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all: ok" in out.stdout and out.stdout.count(": ok") == 4
