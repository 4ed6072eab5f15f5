"""The host planner of the sequential merge fold (holoagent_amd/csrc/hmsg_fold_host.h: the pair rule stated once, the box table
kept from step to step, the pair list produced in an ahead and a late part) against its own reference enumerator, over random
fold histories: tests/host_cpp/fold_host_plan.cpp, a stand-alone program that includes nothing but that header.  It is built with
g++ and run here twice -- plain, and with the address and undefined-behaviour sanitizers of the host compiler (a program of its
own with the runtimes linked in statically: nothing of it is loaded into Python, and it does not care what else the process
environment has the loader bring along)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_cpp", "fold_host_plan.cpp")
INC = os.path.join(ROOT, "holoagent_amd", "csrc")
HISTORIES = 3000      # 1-40 steps each: about 60 000 fold steps, a second or two


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host_cpp/fold_host_plan.cpp")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", exe] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(HISTORIES)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = r.stdout.strip().splitlines()[-1].split()
    return dict(zip(line[0::2], (int(v) for v in line[1::2])))


def test_planned_pair_lists_equal_the_reference_enumerator(tmp_path):
    got = _build_and_run(tmp_path, "fold_host_plan", ["-O2"])
    assert got["histories"] == HISTORIES and got["steps"] > 10 * HISTORIES
    # both ways to a pair list were taken, thousands of times each, and the lists were not trivially empty
    assert got["ahead_steps"] > 1000 and got["late_only_steps"] > 1000 and got["pairs"] > got["steps"]
    for key in ("changed", "unchanged", "absorbed_far", "no_masks", "next_absent", "dropped", "empty_out", "degenerate"):
        assert got[key] > 100, (key, got)


def test_planner_under_the_host_sanitizers(tmp_path):
    got = _build_and_run(tmp_path, "fold_host_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert got["histories"] == HISTORIES and got["ahead_steps"] > 1000 and got["late_only_steps"] > 1000
