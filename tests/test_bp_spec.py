"""Build-time instances of the fused BP kernel with a code's pass structure constant: the generator (tools/bp_spec_gen.cpp) and
the signature match that selects an instance for a decoder handle (csrc/bp_spec.hpp).  Host only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp")
DATA = os.path.join(ROOT, "data")


def build(out, src, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), src, CODE, "-o", out])
    return out


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("specgen") / "bp_spec_gen"), os.path.join(ROOT, "tools", "bp_spec_gen.cpp"))


def printed(gen, *args):
    r = subprocess.run([gen, "--print", *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    entries = []
    for line in r.stdout.splitlines():
        key, val = [s.strip() for s in line.split("=", 1)]
        if key == "name":
            entries.append({"name": val})
        else:
            entries[-1][key] = [int(x) for x in val.split(",")] if "," in val else int(val)
    return entries, r.stderr


def test_h05_structure(gen):
    (e,), _ = printed(gen, os.path.join(DATA, "H05.txt") + ":32")
    assert e["name"] == "H05_L32" and e["L"] == 32
    assert e["c_pass"] == [7, 0, 6, 224, 6, 416, 5, 608, 4, 736]
    assert e["v_pass"] == [6, 0, 6, 192, 5, 384, 3, 544, 3, 640, 2, 736, 2, 800]
    assert e["c_cnt_ge"] == [160, 160, 160, 160, 160, 120, 80, 20, 0]
    assert e["v_cnt_ge"] == [216, 216, 200, 160, 80, 80, 60, 0]
    assert e["n_apass"] == 2


def test_default_codes_and_widths(gen, tmp_path):
    """the Makefile's default list: each matrix at the width the library picks; the include names one namespace, one kernel
    pair and one registry line per entry"""
    out = str(tmp_path / "spec.inc")
    entries, err = printed(gen, "-o", out, *[os.path.join(DATA, f) for f in ("H05.txt", "H.txt", "optimalH.txt")])
    assert [e["name"] for e in entries] == ["H05_L32", "H_L64", "optimalH_L32"], err
    text = open(out).read()
    for e in entries:
        assert text.count("namespace spec_%s {" % e["name"]) == 1
        assert text.count('{{"%s", %d, ' % (e["name"], e["L"])) == 1
        for mc in ("false", "true"):
            assert "spec_%s::bp_fused_kernel<float, 8, %d, 0, %s, true, BP_NVP>" % (e["name"], e["L"], mc) in text
    assert "#define ACG_BP_SPEC_ENTRIES" in text


def test_skips_what_the_kernel_does_not_take(gen, tmp_path):
    entries, err = printed(gen, os.path.join(DATA, "H05.txt") + ":256")
    assert entries == [] and "skipped" in err
    # a check of degree 9: not a degree <= 8 kernel
    p = tmp_path / "wide.txt"
    rows = [[1 if (j // 9 == i or j == (9 * i + 9) % 36) else 0 for j in range(36)] for i in range(4)]
    p.write_text("".join("".join("%d," % x for x in row) + "\n" for row in rows))
    entries, err = printed(gen, str(p))
    assert entries == [] and "degree > 8" in err


def test_signature_match(tmp_path):
    exe = build(str(tmp_path / "bp_spec_check"), os.path.join(ROOT, "tests", "bp_spec_check.cpp"))
    r = subprocess.run([exe, os.path.join(DATA, "H05.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_signature_match_sanitized(tmp_path):
    """the same stand-alone host program under AddressSanitizer and UBSan (runtimes linked statically: the program needs nothing
    from its environment)"""
    exe = build(str(tmp_path / "bp_spec_check_san"), os.path.join(ROOT, "tests", "bp_spec_check.cpp"), "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")
    r = subprocess.run([exe, os.path.join(DATA, "H05.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
