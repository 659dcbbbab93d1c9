"""cvt_mixed_kernel (csrc/gf_cvt_kernels.hpp: one pixel format per frame, the conversion launch of gf_tracker_set_seq_format and gf_cvt_gray_mixed*) walked on
the CPU: tests/native/cvt_mixed_host.hip runs every (block, thread) of both parts of a mixed launch through the function the kernel itself calls, on heap buffers
of exactly the frames' sizes, and compares the whole destination with a plain double loop over the definitions of gf_pixfmt.hpp -- all twelve formats plus
skipped entries in one launch, in permuted order, widths 3 .. 65, heights around the Bayer band height, source offsets 0 .. 3, tight and odd pitches, the grid
of a call that reads its tables and of one that cannot, guard bands around the destination and the fill of the skipped slots.  A second build carries
AddressSanitizer on the host code: a read outside a frame reads outside its allocation there.  hipcc compiles it; no HIP call is made, so it runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-Xarch_host", "-fsanitize=address", "-g"]], ids=["plain", "address sanitizer on the host code"])
def test_every_thread_of_a_mixed_launch(tmp_path, flags):
    exe = tmp_path / "cvt_mixed_host"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-std=c++17"] + flags + ["-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "cvt_mixed_host.hip")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout and "324 cases" in out.stdout and "FAILED" not in out.stdout
