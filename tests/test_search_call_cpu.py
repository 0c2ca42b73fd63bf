"""CPU-only: csrc/search_call.h -- the request descriptors of the search family and slice(), the one function that turns a request
into the launch arguments of a range of its queries -- compiled on its own by the host compiler under AddressSanitizer and UBSan and
run as a stand-alone program (tests/search_call_check.cpp): no GPU, no libpann.so, nothing loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slices_stand_alone(tmp_path):
    exe = str(tmp_path / "search_call_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "search_call_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "search_call: ok"


def test_header_needs_no_hip():
    src = open(os.path.join(ROOT, "parlayann_amd", "csrc", "search_call.h")).read()
    includes = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or "pann_internal" in i or "pann_device" in i], includes
