"""The word-parallel staging of a sixteen-byte group (csrc/kc_encode.hpp) on the host, against the byte-by-byte form:
tests/cpp/test_encode.cpp, a program of its own (host build of the header, as tests/cpp/test_mix.cpp is of kc_common.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_parallel_encode_equals_the_byte_by_byte_one(tmp_path):
    """all 256 base bytes x all 256 quality bytes in each of the 16 positions of a group, the quality cuts 33, 53 and 128,
    ASCII reads, the case-masked block and the read-cache bytes: codes, ok bits, separator bits and `bad`, bit for bit;
    built with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(str(tmp_path), "test_encode")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_encode.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("bad=0"), out.stdout + out.stderr
    assert int(out.stdout.split("cases=")[1].split()[0]) > 9000000
