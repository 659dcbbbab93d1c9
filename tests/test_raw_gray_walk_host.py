"""The raw-format conversion kernels (csrc/gf_cvt_kernels.hpp: Bayer, YUV 4:2:2, MONO16 -> MONO8) walked on the CPU: tests/native/raw_gray_host.hip runs the
per-thread work of every (block, thread) of every launch form on heap buffers of exactly the frames' sizes and compares the bytes with a plain double loop over
the definition -- all seven formats, widths 3 .. 65, heights around the band height, row paddings, source offsets 0 .. 3, batch 1 and 3, guard bands around the
destination.  A second build carries AddressSanitizer on the host code: a stencil that read outside a frame would read outside its allocation there.  hipcc
compiles it (the header holds __global__ functions); no HIP call is made, so it runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-Xarch_host", "-fsanitize=address", "-g"]], ids=["plain", "address sanitizer on the host code"])
def test_every_thread_of_every_form(tmp_path, flags):
    exe = tmp_path / "raw_gray_host"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17"] + flags + ["-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "raw_gray_host.hip")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(": ok") == 7 and "FAILED" not in out.stdout
