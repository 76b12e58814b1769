"""The plan build on the host: tools/plan_digest.cpp linked with the plan sources alone (no GPU, no HIP call).

`--check` verifies the structural invariants of the fill tables (chunk boundaries and their maxima, row pointers of the reduced lists,
index bounds, the paired-table bijection, the slot permutation) for plans of every tree and of the chain trees; the environment
switches of the plan build must change what they are meant to change and nothing else.  No digests are pinned: they would pin the
last bits of the math library.
"""
import os
import re
import subprocess

import pytest

from biem_helmholtz_sphere_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SOURCES = ["plan.cpp", "plan_tree.cpp", "plan_fill.cpp"]
SWITCHES = ("BIEM_FILL_RED_WAVES", "BIEM_FILL_NC", "BIEM_FILL_LIST_ORDER", "BIEM_PLAN_STATS")


@pytest.fixture(scope="module")
def digest(tmp_path_factory):
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("plan_digest") / "plan_digest")
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tools", "plan_digest.cpp")]
    cmd += [os.path.join(_build.CSRC, f) for f in PLAN_SOURCES] + ["-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args, **env):
        base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        return subprocess.run([exe, *map(str, args)], env={**base, **env}, capture_output=True, text=True)
    return run


def _fields(line):
    """name -> text of the `name=value` items of a digest line (tables: `size:digest`)."""
    return dict(re.findall(r" (\w+)=(\"[^\"]*\"|\S+)", line))


def test_plan_sources_are_those_of_the_library():
    assert [f for f in _build.SOURCES if f.startswith("plan")] == PLAN_SOURCES


def test_invariants_hold_for_every_tree(digest):
    cases = "a 6 a 161 ba 7 ba 12 bba 4 bba 7 caa 3 caa 6 chain3 8 chain5 4 chain7 3".split()
    r = digest("--check", *cases)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) // 2
    for line in lines:
        f = _fields(line)
        assert f["rc"] == "0" and f["check"] == "ok", line
    a161 = _fields(lines[1])
    assert a161["lists_built"] == "0" and a161["coef"].startswith("0:")      # beyond kLists2dMax: no term lists


def test_unsupported_chain_plans_report_code_3(digest):
    r = digest("--check", "chain7", 8, "chain10", 5, "chain11", 2)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert [_fields(l)["rc"] for l in lines] == ["3", "3", "3"]
    assert "16-bit" in lines[0] and "projection matrix" in lines[1] and "unsupported" in lines[2]


def test_list_order_switch_changes_the_order_only(digest):
    default = _fields(digest("--check", "ba", 12).stdout)
    r = digest("--check", "ba", 12, BIEM_FILL_LIST_ORDER="natural")
    assert r.returncode == 0, r.stdout + r.stderr
    natural = _fields(r.stdout)
    assert natural["ridx"] != default["ridx"]
    for name in ("coef", "qcoef", "q2coef"):
        assert natural[name] == default[name]
    # the natural order of a lane's terms costs LDS bank conflicts in the table gather, the dealt order avoids most of them
    assert float(natural["red_gather_cycles"]) > float(default["red_gather_cycles"]) >= 1.0


def test_eight_wave_switch_cuts_more_reduced_chunks(digest):
    default = _fields(digest("--check", "ba", 12).stdout)
    r = digest("--check", "ba", 12, BIEM_FILL_RED_WAVES="8")
    assert r.returncode == 0, r.stdout + r.stderr
    eight = _fields(r.stdout)
    assert eight["check"] == "ok" and eight["red_waves"] == "8" and default["red_waves"] == "16"
    n_chunks = lambda f: int(f["rchunk"].split(":")[0]) - 1
    assert n_chunks(eight) > n_chunks(default) >= 1
