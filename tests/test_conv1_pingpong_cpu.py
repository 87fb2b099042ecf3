"""The schedule of the ping-pong first-block forward (seld_amd/csrc/conv1_pp_sched.h) walked on the host: a stand-alone program includes the header
the kernel includes and, for every shape of tests/test_conv1_pingpong_gpu.py plus the bench shape, checks that every tile is visited exactly once
and that both wave groups of every block take the same number of barriers (a mismatch would hang the workgroup)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 5), (1, 10), (1, 15), (3, 25), (3, 1730), (4, 2600), (32, 3000)]


def test_schedule_visits_every_tile_once_with_equal_barrier_counts(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "conv1_pp_sched_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "seld_amd", "csrc"),
                    os.path.join(ROOT, "tests", "conv1_pp_sched_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    args = [str(v) for shape in SHAPES for v in shape]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok ") == len(SHAPES), r.stdout
    assert "ok B=32 H=3000: 9600 tiles, 512 virtual workgroups, 256 blocks, 19 trips, 39 barriers per wave" in r.stdout


def test_gpu_test_shapes_are_the_ones_walked_here():
    with open(os.path.join(ROOT, "tests", "test_conv1_pingpong_gpu.py")) as f:
        src = f.read()
    for B, H in SHAPES[:-1]:
        assert f"({B}, {H})" in src
