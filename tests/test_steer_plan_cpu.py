"""CPU-only: the steered plans of csrc/search_plan.h (DESIGN.md "Steered masked search") -- compiled on their own by the host
compiler under AddressSanitizer and UBSan and run as a stand-alone program (tests/steer_plan_check.cpp): no GPU, no libpann.so,
nothing loaded into this interpreter.  That the plans of every existing call are unchanged is tests/test_search_plan_cpu.py's."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steered_plans_and_layouts_stand_alone(tmp_path):
    exe = str(tmp_path / "steer_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "steer_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"steer_plan: ok, (\d+) plans \((\d+) with the table in LDS, (\d+) in HBM\)", r.stdout.strip())
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
