"""No GPU: the layering of the C API's host files (csrc/capi*.hip) -- what the library exports, which file
includes what -- and the refusals of the entry points that need no simulator, held to the whole message and to which check speaks
first (tests/capi_refusal_cases.py, tests/golden/capi_refusals.json)."""
import glob
import json
import os
import re
import shutil
import subprocess

import pytest

import capi_refusal_cases as cases
from madrona_rl_envs_playground_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "madrona_rl_envs_playground_amd", "csrc")
CAPI = sorted(glob.glob(os.path.join(CSRC, "capi*")))


def test_the_library_exports_what_it_did_before_the_split(hip_lib):
    if not shutil.which("nm"):
        pytest.skip("nm is not installed")
    want = open(os.path.join(REPO, "tests", "golden", "capi_exports.txt")).read().split()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("mrl_"))
    assert got == want
    assert len(want) == 78 and set(_lib.SYMBOLS) <= set(want)


def test_includes_go_one_way():
    sources = [path for path in CAPI if path.endswith(".hip")]
    assert len(sources) >= 5 and os.path.join(CSRC, "capi_internal.hpp") in CAPI
    for path in sources:
        included = re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)
        assert "capi_internal.hpp" in included, path
        assert not [name for name in included if name.endswith(".hip")], path


def test_only_capi_hip_sees_the_source_hash():
    assert [os.path.basename(path) for path in CAPI if "MRL_SOURCE_HASH" in open(path).read()] == ["capi.hip"]


def test_no_cxx_island_in_a_c_block():
    for path in CAPI:
        assert 'extern "C++"' not in open(path).read(), path


def test_refusals_word_for_word(hip_lib):
    forms = cases.cpu_forms()
    want = cases.expected("cpu", forms)
    assert sorted(json.load(open(cases.GOLDEN))["cpu"]) == sorted(form.name for form in forms)
    got = cases.run(hip_lib, forms)
    assert sorted(got) == sorted(want)
    wrong = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not wrong, wrong
    assert all(rc != _lib.MRL_OK for rc, _ in want.values()), "every case is a refusal"
