"""Which edge rows of a build-time fused BP instance keep their phi fast-path test: the census (csrc/bp_sat_census.hpp), the masks
the generator (tools/bp_spec_gen.cpp) writes from it, and what the end-case batch of tests/test_satrows_gpu.py drives the cleared
rows through, by the census model.  Host only."""
import os
import re
import subprocess

import pytest

from satrows_cases import END_FRAMES, END_SNR, end_case_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp")
DATA = os.path.join(ROOT, "data")
DEFAULT = (("H05", 32, 280), ("H", 64, 128), ("optimalH", 32, 280))  # the Makefile's SPEC_CODES: matrix, its width, n


def build(out, src, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), src, CODE, "-o", out])
    return out


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("satgen") / "bp_spec_gen"), os.path.join(ROOT, "tools", "bp_spec_gen.cpp"))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("satcheck") / "satrows_check"), os.path.join(ROOT, "tests", "satrows_check.cpp"))


def generated(gen, tmp_path, *opts, codes=("H05.txt:32",)):
    out = str(tmp_path / ("spec%s.inc" % "_".join(opts).replace("-", "m")))
    r = subprocess.run([gen, "-o", out, *opts, *[os.path.join(DATA, c) for c in codes]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(out).read()


def masks(text, fn):
    """the look-up fn of every policy of a generated include, in order"""
    return [[int(x.rstrip("u")) for x in m.split(",")]
            for m in re.findall(r"static constexpr unsigned %s\(int p\) \{\s*constexpr unsigned v\[\] = \{([0-9u,]+)\};" % fn, text)]


def test_census_and_thresholds(check):
    r = subprocess.run([check, os.path.join(DATA, "H05.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_census_and_thresholds_sanitized(tmp_path):
    """the same stand-alone host program under AddressSanitizer and UBSan (runtimes linked statically: the program needs nothing
    from its environment)"""
    exe = build(str(tmp_path / "satrows_check_san"), os.path.join(ROOT, "tests", "satrows_check.cpp"), "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")
    r = subprocess.run([exe, os.path.join(DATA, "H05.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_generated_masks(gen, tmp_path):
    ALL = 0xFFFFFFFF
    t0 = generated(gen, tmp_path, "-t", "0")
    assert masks(t0, "c_sat_rows") == [[ALL] * 5] and masks(t0, "v_sat_rows") == [[ALL] * 7]
    assert "census at -2dB, threshold 0 per cent" in t0 and "@-2dB,t0\"" in t0
    for t in ("0.01", "3", "10", "20"):
        text = generated(gen, tmp_path, "-t", t)
        (c,), (v,) = masks(text, "c_sat_rows"), masks(text, "v_sat_rows")
        assert c[2] & 0xF == 0 and v[6] & 1 == 0, (t, c, v)              # the rows that never fire
        assert c[3] & 0x1F == 0x1F and c[4] & 0xF == 0xF, (t, c)        # the absorbed passes keep every row
        assert "census at -2dB, threshold %s per cent" % t in text and ("@-2dB,t%s\"" % t) in text
    t101 = generated(gen, tmp_path, "-t", "101")
    (c,), (v,) = masks(t101, "c_sat_rows"), masks(t101, "v_sat_rows")
    cdeg, vdeg = (7, 6, 6, 5, 4), (6, 6, 5, 3, 3, 2, 2)  # the rows the passes of H05 have (tests/test_bp_spec.py)
    assert [m & ((1 << d) - 1) for m, d in zip(c, cdeg)] == [0] * 5 and [m & ((1 << d) - 1) for m, d in zip(v, vdeg)] == [0] * 7
    s2 = generated(gen, tmp_path, "-s", "2", "-t", "10")
    assert "census at 2dB, threshold 10 per cent" in s2 and "@2dB,t10\"" in s2
    # the default: -2 dB, and a threshold that is written down with the masks
    d = generated(gen, tmp_path)
    assert re.search(r"census at -2dB, threshold [0-9.]+ per cent", d)
    # a Makefile variable passes both options
    mk = open(os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "Makefile")).read()
    assert "-t $(SPEC_SAT_T)" in mk and "-s $(SPEC_SAT_SNR)" in mk and "$(SPECOPTS) $(SPEC_CODES)" in mk


def test_end_case_batch_reaches_the_cleared_rows(gen, check, tmp_path):
    """the batch of tests/test_satrows_gpu.py, by the census model: on either side a row that a -t 10 build leaves without its
    test (H05: the message rows of check passes 0-2 and four variable rows) meets an input of exactly +0, one of magnitude >= 66
    and +inf (and NaN); a -t 101 build clears these rows and all others"""
    text = generated(gen, tmp_path, "-t", "10", codes=[m + ".txt" for m, _, _ in DEFAULT])
    rows = re.findall(r'"(c:[0-9a-f,]+/v:[0-9a-f,]+@[^"]*)"', text)
    assert len(rows) == len(DEFAULT), rows
    for (matrix, L, n), r in zip(DEFAULT, rows):
        y = end_case_batch(n)
        path = str(tmp_path / (matrix + ".f64"))
        y.tofile(path)
        p = subprocess.run([check, "probe", os.path.join(DATA, matrix + ".txt"), str(L), str(END_SNR), path, str(END_FRAMES), r],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.startswith("probe c "), p.stdout + p.stderr
        w = p.stdout.split()
        c, v = [int(x) for x in w[2:6]], [int(x) for x in w[7:11]]
        print(matrix, r, "check side: +0, >= 66, +inf, NaN =", c, " variable side:", v)
        assert all(x > 0 for x in c) and all(x > 0 for x in v), (matrix, r, c, v)
