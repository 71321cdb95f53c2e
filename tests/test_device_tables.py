"""The cache of the small tables the grid queries keep per device (csrc/device_tables.hpp: the ring offsets, the clearance
walk, the fleet layer's spans) without a GPU: hits and misses by (device, key), the user count that keeps a live layer's
table through a release, and every block handed to `free` exactly once.  tests/device_tables_check.cpp is built with the
address and undefined-behaviour sanitizers and run as a process of its own; tests/test_gpu_fleet_layer.py sees the user
count through real layers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/device_tables_check.cpp")
    exe = str(tmp_path_factory.mktemp("device_tables") / "device_tables_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "device_tables_check.cpp"), "-o", exe], check=True)
    return exe


def test_device_tables_policy(program):
    """a miss then a hit, the same key on another device, held entries through a release, give-back then release, give-back of
    an unknown block, release of an empty cache, 200 inserts: the program stops at the first wrong answer and names the line"""
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "device tables: ok", (out.returncode, out.stdout, out.stderr)
