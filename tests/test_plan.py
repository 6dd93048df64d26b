"""What a program's plan (csrc/orb_plan.h) chooses, pinned on the CPU: tests/plan_dump.cpp is compiled for the host only, run once per
environment of tests/golden/plan/cases.json, and every line it prints -- pipelines, band heights, threads, tile widths, slot tables,
the instance of k_front a full batch takes -- is compared with the file, which was recorded from the code as it stood before the plan
had a header of its own (NOTEBOOK.md, "The plan's record").  No device is involved: the plan is integer arithmetic on the host."""
import json
import os
import subprocess

import pytest

from tinyslam_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = json.load(open(os.path.join(ROOT, "tests", "golden", "plan", "cases.json")))
# build.py's flags that bear on host arithmetic (the plan evaluates blur_tap() in binary32), and no optimiser: compiling is the cost
HOST_FLAGS = [f for f in build.HIPCC_FLAGS if f in ("-std=c++17", "-ffp-contract=off", "-fno-fast-math")]


@pytest.fixture(scope="session")
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    # (host only, linked without the HIP runtime: the object still names the device binary it would have carried; nothing reads that symbol)
    subprocess.run([build._hipcc(), "-x", "hip", "--offload-host-only", "--offload-arch=gfx950", "-no-hip-rt", "-O1", "-Wall", "-Wno-unused-function"] + HOST_FLAGS +
                   ["-Wl,--unresolved-symbols=ignore-all", "-o", exe, os.path.join(ROOT, "tests", "plan_dump.cpp")], check=True, timeout=300)
    return exe


def run_group(exe, group):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TINYORB_")}
    env.update(group["env"])
    r = subprocess.run([exe], input="".join(c["case"] + "\n" for c in group["cases"]), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(group["cases"]), r.stdout[-2000:]
    return [json.loads(line) for line in lines]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: ",".join("%s=%s" % kv for kv in g["env"].items()) or "no-switch")
def test_plan_is_the_recorded_one(plan_dump, group):
    for c, got in zip(group["cases"], run_group(plan_dump, group)):
        assert got == c["expect"], "%s under %s" % (c["case"], group["env"])


def instances(plan_dump, case, env=None):
    """-> [(instance, reason)] per level for `W H depth max_batch flags` on an MI355X's LDS, as TINYORB_FRONT_TRACE words them"""
    got, = run_group(plan_dump, {"env": env or {}, "cases": [{"case": case + " 0 0 2097152 163840"}]})
    assert got["error"] is None and got["fused"]
    return [(lvl["geo"], lvl["why"]) for lvl in got["levels"]]


def test_headline_program_takes_the_specialised_instances(plan_dump):
    """tests/test_gpu_front_specialised.py reads the same from the trace line on the GPU: 1280x720, depth 2, RGBA, a batch of 8."""
    assert instances(plan_dump, "1280 720 2 8 0") == [("specialised 720p-L0", None), ("specialised 720p-L1", None)]
    assert instances(plan_dump, "1280 720 2 8 0", {"TINYORB_FRONT_GENERIC": "1"}) == [("generic", "TINYORB_FRONT_GENERIC")] * 2


# that file's NEAR_MISSES: the case, its switches, and the first field that rules the specialised instance out at each level
NEAR_MISSES = {
    "w1272": ("1272 720 2 8 0", {}, ["gw", "blur_p"]),
    "w1288": ("1288 720 2 8 0", {}, ["gw", "gw"]),
    "h712": ("1280 712 2 8 0", {}, ["gh", "h"]),
    "depth3": ("1280 720 3 8 0", {}, ["n_slots", "write_mip", "lvl"]),
    "band_rows8": ("1280 720 2 8 0", {"TINYORB_BAND_ROWS": "8"}, ["band_rows", "band_rows"]),
    "y8": ("1280 720 2 8 16", {}, ["input_y8", "input_y8"]),
    "max_batch1": ("1280 720 2 1 0", {}, ["band_rows", "band_rows"]),
}


@pytest.mark.parametrize("name", sorted(NEAR_MISSES))
def test_near_miss_takes_the_generic_instances(plan_dump, name):
    case, env, why = NEAR_MISSES[name]
    assert instances(plan_dump, case, env) == [("generic", w) for w in why]
