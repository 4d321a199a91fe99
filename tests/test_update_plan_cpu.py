"""The work plan of the MFMA update launches (plan_update_work, pangulu_amd/csrc/platform/pg_hip_update_plan.h) without a device: which
kernel runs each (group, tile) pair of a launch, and in which order.  tests/update_plan_check.cpp compiles the header as plain C++
behind tests/hip_emulation_shims.h and checks it two ways: properties of the plan over seeded random and hand-made inputs, and
equality, item by item and field by field, with the plans recorded in tests/golden/update_plan_expected.json (tests/golden/README.md
says where they come from)."""
import json
import os
import subprocess

import pytest

from .helpers import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("update_plan") / "update_plan_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "update_plan_check.cpp"), "-o", path], check=True)
    return path


def test_plan_properties(exe):
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-4000:]


def test_plan_equals_recorded(exe):
    """The recorded cases are inputs the program makes from fixed seeds; the file holds what the inline code made of them."""
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "update_plan_expected.json")))["cases"]
    assert len(cases) >= 6
    out = subprocess.run([exe, "plans"], stdout=subprocess.PIPE, text=True, timeout=300, check=True)
    tok = [int(x) for x in out.stdout.split()]
    at = 0
    for k, e in enumerate(cases):
        nw, nf, nfm = tok[at:at + 3]
        assert (nw, nf, nfm) == (e["nw"], e["nf"], e["nfm"]), "case %d" % k
        assert tok[at + 3:at + 3 + 7 * nw] == e["work"], "case %d: work" % k
        assert tok[at + 3 + 7 * nw:at + 3 + 7 * (nw + nf)] == e["work_f"], "case %d: work_f" % k
        at += 3 + 7 * (nw + nf)
    assert at == len(tok)
