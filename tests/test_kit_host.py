"""The pure helpers of csrc/kc_kit.hpp on the host, against the definitions the kernel headers carried before the kit:
tests/cpp/test_kit.cpp, a program of its own (host build of the header, as tests/cpp/test_encode.cpp is of kc_encode.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kit_helpers_equal_the_definitions_they_replaced(tmp_path):
    """base code and complement on all 256 bytes; digit count and BCD at 0, 9, 10, 10^k - 1 and 10^k up to sixteen digits,
    65535 and 2^32 - 1, against the old chains and loops and against snprintf; the search on every [lo, hi] of strictly
    increasing arrays of 1 to 9 items for every x from a[lo] to one past a[hi], against a linear scan, for "a[lo] <= x is
    given" and for the writers' "first segment that starts behind x"; built with the address and undefined-behaviour
    sanitizers"""
    exe = os.path.join(str(tmp_path), "test_kit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_kit.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("bad=0"), out.stdout + out.stderr
    assert int(out.stdout.split("cases=")[1].split()[0]) > 100000
