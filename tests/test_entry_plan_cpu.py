"""CPU-only: the host arithmetic of the medoid form in csrc/grouped_plan.h (DESIGN.md "Entry points") -- the pieces of a list and
of a chunk, the sums a piece leaves, the scratch layout -- compiled on its own by the host compiler under AddressSanitizer and
UBSan and run as a stand-alone program (tests/entry_plan_check.cpp): no GPU, no libpann.so, nothing loaded into this interpreter.
The kernels count a list's pieces with the header's own function, and the option the tests size their lists by is the constant."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pieces_and_scratch_stand_alone(tmp_path):
    exe = str(tmp_path / "entry_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "entry_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "entry_plan: ok"


def test_the_piece_constant_is_the_cases():
    import entry_cases as ec
    src = open(os.path.join(ROOT, "parlayann_amd", "csrc", "grouped_plan.h")).read()
    assert int(re.search(r"constexpr uint32_t CENTROID_PIECE_IDS = (\d+);", src).group(1)) == ec.P
    kernels = open(os.path.join(ROOT, "parlayann_amd", "csrc", "entry_points.hip")).read()
    assert "centroid_pieces_of(" in kernels and '#include "grouped_plan.h"' in kernels      # one definition for host and device
