"""The integer code the range-sensor kernels share (csrc/sense_rays.hpp: the rays, march(), clip_of; csrc/grid_census.hpp: the
head / chunks / tail split of a streamed array, the census' classes) without a GPU.  tests/sense_rays_check.cpp is built with
the address and undefined-behaviour sanitizers and run as a process of its own; the kernels that use the same functions are held
bit for bit by tests/test_gpu_sense.py, test_gpu_evidence.py, test_gpu_gain.py and test_gpu_mi.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/sense_rays_check.cpp")
    exe = str(tmp_path_factory.mktemp("sense_rays") / "sense_rays_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"),
                    os.path.join(ROOT, "tests", "sense_rays_check.cpp"), "-o", exe], check=True)
    return exe


def test_rays_march_and_split(program):
    """R = 1 .. 24, every ray: Ray and march() visit the closed form's offsets; march() ends at the disc, at the clip (clip_of at
    the corners, the edges and the interior of a 7 x 5 grid) and at the first blocking visit; element sizes 1 and 4, every base
    offset, n = 0 .. 40: head, whole loads and tail cover [0, n) once, the loads 16-byte aligned.  The program stops at the first
    wrong answer and names the line"""
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "sense rays: ok", (out.returncode, out.stdout, out.stderr)
