"""CPU-only: csrc/search_plan.h -- the beam search's point layout, the LDS layouts of its three kernel families and the plan of a
launch -- compiled on its own by the host compiler under AddressSanitizer and UBSan and run as a stand-alone program
(tests/search_plan_check.cpp) over tests/golden/search_plans_v1.txt, the decisions recorded from the commit before the plan
became a header (tests/golden/make_search_plans.py): no GPU, no libpann.so, nothing loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "search_plans_v1.txt")


def test_plans_and_layouts_stand_alone(tmp_path):
    exe = str(tmp_path / "search_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "search_plan_check.cpp")])
    r = subprocess.run([exe, TABLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = sum(1 for l in open(TABLE) if not l.startswith("#"))
    assert 1000 <= rows <= 3000 and os.path.getsize(TABLE) < 1 << 20
    assert r.stdout.strip() == f"search_plan: ok, {rows} rows"


def test_header_needs_no_hip():
    src = open(os.path.join(ROOT, "parlayann_amd", "csrc", "search_plan.h")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or "pann_internal" in i or "pann_device" in i], includes
