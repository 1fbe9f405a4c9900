"""Workspaces are part of the C ABI: callers allocate what the size functions return, and the entry points carve those bytes.  No GPU.
  * every size function, the two offsets of ngp_field_train_live_list, and the refusal (return code and message) of a workspace one byte short
    equal tests/golden/workspace_sizes.json, recorded by tools/workspace_sizes.py from the library BEFORE the layouts moved onto one carver;
  * the carver itself (csrc/ngp_workspace.h) under AddressSanitizer and UBSan, as a stand-alone program (tests/helpers/carver_check.cpp)."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    spec = importlib.util.spec_from_file_location("workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(tool.GOLDEN) as f:
        golden = json.load(f)
    return golden, json.loads(json.dumps(tool.collect()))      # through JSON: tuples and lists compare alike


def test_every_size_function_returns_the_recorded_bytes(recorded):
    golden, now = recorded
    assert sorted(now["sizes"]) == sorted(golden["sizes"]) and len(golden["sizes"]) == 17
    for name, rows in golden["sizes"].items():
        assert now["sizes"][name] == rows, name


def test_size_functions_refuse_shapes_with_zero(recorded):
    golden, _ = recorded
    by_args = lambda name: {tuple(r[:-1]): r[-1] for r in golden["sizes"][name]}  # noqa: E731
    assert by_args("ngp_field_train_workspace")[(0,)] == 0
    mesh, plan = by_args("ngp_marching_cubes_workspace"), by_args("ngp_plan_workspace")
    assert mesh[(1, 17, 17)] == 0 and mesh[(17, 17, 1025)] == 0 and mesh[(2, 2, 2)] > 0 and mesh[(1024, 1024, 1024)] > 0
    assert plan[(1, 1)] == 0 and plan[(256, 1)] == 0 and plan[(2, 0)] == 0 and plan[(2, 65537)] == 0 and plan[(255, 65536)] > 0


def test_live_list_offsets_are_the_recorded_ones(recorded):
    golden, now = recorded
    assert now["live_list"] == golden["live_list"]
    assert golden["live_list"][0][:2] == [0, -1]                # an empty batch has no list


def test_a_workspace_one_byte_short_is_refused_as_recorded(recorded):
    golden, now = recorded
    assert sorted(now["refusals"]) == sorted(golden["refusals"])
    for name, (rc, message) in golden["refusals"].items():
        assert now["refusals"][name] == [rc, message], name
        assert rc in (-1, -3)                                   # NGP_EINVAL or NGP_EWORKSPACE, never a launch error: nothing reached the device


def test_carver_under_address_and_ub_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "carver_check")
    # (the sanitizer runtimes linked statically: the program then runs the same whatever else the loader brings in)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) and "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    "-I", os.path.join(ROOT, "nerf-navigation_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "carver_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "carver ok", run.stdout + run.stderr
