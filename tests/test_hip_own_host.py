"""gf_hip_own.hpp (the owning device / page-locked buffers, stream and event wrappers every handle of the library is made of) on its own:
tests/native/hip_own_host.hip includes nothing else of the library.  Without a GPU every way of getting memory must fail and leave the object empty; with one,
alloc is exact and zeroed, fit only grows, and a move leaves its source empty.  hipcc compiles it as tests/test_copy_list_host.py compiles its program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("hip_own") / "hip_own_host"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-o", str(path),
                           os.path.join(ROOT, "tests", "native", "hip_own_host.hip")])
    return str(path)


def _run(exe, mode, checks, env=None):
    out = subprocess.run([exe, mode], capture_output=True, text=True, env=env)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert out.stdout.count(": ok") == checks


def test_without_a_device_nothing_is_held(exe):
    _run(exe, "nodevice", 13, dict(os.environ, HIP_VISIBLE_DEVICES="-1"))   # the same on a machine that has one


@pytest.mark.gpu
def test_alloc_fit_and_moves_on_the_device(exe):
    _run(exe, "device", 19)
