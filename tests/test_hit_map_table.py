"""The host-side policy of the inflated collision map (csrc/hit_map_table.hpp) without a GPU: which buffer a build gets, when
it is reallocated or cleared, which stamp comes next, when a tick may reuse the last build -- and the offset set of the
dilation against the oracle's ring search.  tests/hit_map_table_check.cpp is built with the address and undefined-behaviour
sanitizers and run as a process of its own; tests/test_gpu_collision_state.py sees the same rules through real builds."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLL = (0.7, 1.0, 0.2, 0.8)      # the radii of tests/test_gpu_collision_state.py
COLL2 = (0.3, 0.6, 0.1, 0.5)
RES, N = 0.1, 41


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/hit_map_table_check.cpp")
    exe = str(tmp_path_factory.mktemp("hit_map_table") / "hit_map_table_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "hit_map_table_check.cpp"),
                    "-o", exe], check=True)
    return exe


def test_map_table_policy(program):
    """300 builds on one key (a clear at the build after stamp 255 only), grow / shrink, two keys, 66 keys and release, the
    epoch key's hits and every way to miss it: the program stops at the first wrong answer and names the line"""
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "hit map table: ok", (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("coll", [COLL, COLL2])
def test_ring_offsets_are_the_oracles_dilation(program, coll):
    """One occupied cell in the middle of a 41 x 41 grid at 0.1 m: the oracle's collisionCheck at the centre of every cell
    is "(occupied cell - this cell) is one of ring_offsets" (the radii in cells as csrc/entry_util.hpp derives them)"""
    r_bnd, r_col, r_max = (math.floor(coll[0] / RES), math.floor((coll[0] + coll[2]) / RES), math.floor(coll[1] / RES))
    out = subprocess.run([program, str(r_bnd), str(r_col), str(r_max)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout, out.stderr)
    offsets = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(set(offsets)) == len(offsets) > 0
    data = np.zeros((N, N), dtype=np.int8)
    mid = N // 2
    data[mid, mid] = 100
    xmin, ymin = -2.0, -1.0
    g = po.GridMap(xmin, xmin + N * RES, ymin, ymin + N * RES, RES, data.reshape(-1))
    assert (g.xsize, g.ysize) == (N, N)
    hits = set()
    for i in range(N):
        for j in range(N):
            x, y = xmin + (j + 0.5) * RES, ymin + (i + 0.5) * RES
            assert g.world2grid(x, y) == (i, j)     # (the pose is inside the cell it stands for)
            if po.collision_check(coll, g, np.array([x, y, 0.0]))[0]:
                hits.add((mid - j, mid - i))      # (dx, dy) = cell - centre
    assert len(hits) > 0 and len(hits) == len(offsets), (len(hits), len(offsets))
    assert hits == set(offsets)
