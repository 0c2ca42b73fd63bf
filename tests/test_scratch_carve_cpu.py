"""CPU-only: csrc/scratch_carve.h -- the one way a device buffer is cut into several arrays (Carve, carve_into) -- compiled on its
own by the host compiler under AddressSanitizer and UBSan and run as a stand-alone program (tests/scratch_carve_check.cpp) against a
malloc-backed stand-in for the Workspace: no GPU, no libpann.so, nothing loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_layouts_stand_alone(tmp_path):
    exe = str(tmp_path / "scratch_carve_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "scratch_carve_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "scratch_carve: ok"


def test_header_needs_no_hip():
    src = open(os.path.join(ROOT, "parlayann_amd", "csrc", "scratch_carve.h")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or "pann_internal" in i or "pann_device" in i], includes
