"""The parser of KC_DEBUG_FILL (csrc/kc_debug_fill.hpp) on the host: tests/cpp/test_debug_fill.cpp, a program of its own
(host build of the header, as tests/cpp/test_kit.cpp is of kc_kit.hpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_debug_fill_parser_takes_a_byte_and_nothing_else(tmp_path):
    """"", "0", "255", "256", "0xA5", "0x5a", "-1", "12x" and their neighbours (signs, blanks, a bare 0x, digits past any
    integer's range); every spelling of 0..300 in decimal and hexadecimal; every one- and two-byte string against the
    grammar restated with strspn and strtoul; the environment reader set, unset and unparsable; built with the address and
    undefined-behaviour sanitizers"""
    exe = os.path.join(str(tmp_path), "test_debug_fill")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_debug_fill.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("bad=0"), out.stdout + out.stderr
    assert int(out.stdout.split("cases=")[1].split()[0]) > 100000


def test_the_python_side_reads_the_variable_as_the_library_does(tmp_path, monkeypatch):
    """kcount._debug_fill restates the grammar of csrc/kc_debug_fill.hpp: the issue's strings and their neighbours through
    it, and a sample of strings through both -- the C parser's verdict comes from a small program built here"""
    from mhm2_kmer_analysis_v2_amd.kcount import _debug_fill
    cases = {"": None, "0": 0, "255": 255, "256": None, "0xA5": 0xA5, "0x5a": 0x5A, "-1": None, "12x": None, "0x": None, "0X5A": 0x5A, " 1": None,
             "1 ": None, "+1": None, "0x100": None, "017": 17, "9" * 30: None, "0x" + "F" * 30: None, "1_0": None, "\u0663": None, "0b1": None, "1e1": None}
    for s, want in cases.items():
        monkeypatch.setenv("KC_DEBUG_FILL", s)
        assert _debug_fill() == want, s
    monkeypatch.delenv("KC_DEBUG_FILL")
    assert _debug_fill() is None
    src = os.path.join(str(tmp_path), "p.cpp")
    open(src, "w").write('#include <cstdio>\n#include "%s"\nint main(int c, char **v) { for (int i = 1; i < c; i++) std::printf("%%d\\n", '
                         'kc::parse_debug_fill(v[i])); }\n' % os.path.join(ROOT, "mhm2_kmer_analysis_v2_amd", "csrc", "kc_debug_fill.hpp"))
    exe = os.path.join(str(tmp_path), "p")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    sample = [s for s in cases if s and s.isascii()] + ["%d" % v for v in range(0, 300, 7)] + ["0x%x" % v for v in range(0, 300, 7)] + ["0X%03X" % v for v in range(0, 300, 11)]
    got = [int(x) for x in subprocess.run([exe] + sample, capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(sample)
    for s, c in zip(sample, got):
        monkeypatch.setenv("KC_DEBUG_FILL", s)
        assert _debug_fill() == (None if c < 0 else c), s
