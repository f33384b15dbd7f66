"""Host only: the seven handle-free libraries answer every call of tests/golden/host_contract.json as the commit named in it did - plan
sizes at the boundaries of the 256-thread block and of VOX_TILE, the return code and exact error text of null arguments, range checks
and buffers one byte short (the message prints the needed size, which pins every call's layout) - and keep seven separate error
buffers.  The file is recorded by tools/capture_host_contract.py from a build of that commit, never from the code under test; every
call returns before its first HIP call, so this needs no GPU."""
import functools
import json
import pathlib

import pytest

import host_contract_cases as HC

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "host_contract.json"


@functools.lru_cache(maxsize=None)
def golden():
    return json.loads(GOLDEN.read_text())


@functools.lru_cache(maxsize=None)
def library(name):
    from vista_slam_amd import _lib, build
    build.build_lib()
    return getattr(_lib, "load_" + name)()


def call(name, fn, args):
    from vista_slam_amd import _lib
    return HC.call(_lib, library(name), name, fn, args)


@pytest.mark.parametrize("name", HC.LIBRARIES)
def test_every_recorded_call_answers_as_recorded(name):
    records = [r for r in golden()["records"] if r["lib"] == name]
    assert len(records) >= 16
    for r in records:
        got = call(name, r["fn"], r["args"])
        assert got == {"rc": r["rc"], "error": r["error"], "sizes": r["sizes"]}, (r["fn"], r["kind"], r["args"], got)


def test_the_record_covers_the_contract():
    """The file holds exactly the calls of host_contract_cases.cases(), whose byte counts come from the recorded plans; every plan is
    there at the eight counts for each of its count-like arguments, every entry point with a null argument, every workspace and index
    buffer one byte short."""
    from vista_slam_amd import _lib
    records = golden()["records"]
    assert len(golden()["commit"]) == 40
    plans = {(r["lib"], r["fn"], json.dumps(r["args"])): r["sizes"] for r in records if r["kind"] == "plan"}
    want = HC.cases(lambda name, fn, args: call(name, fn, args)["sizes"])
    assert [(r["lib"], r["kind"], r["fn"], r["args"]) for r in records] == [(n, k, f, json.loads(json.dumps(a))) for n, k, f, a in want]
    kinds = {}
    for r in records:
        kinds.setdefault((r["lib"], r["fn"]), set()).add(r["kind"])
        assert (r["rc"] == 0) == (r["kind"] == "plan") and (r["rc"] in (0, -1)) and (r["rc"] == 0) == (r["error"] is None), r
    for name in HC.LIBRARIES:
        fn, good, counts = HC.PLANS[name]
        assert {"plan", "range", "null"} <= kinds[(name, fn)]
        for pos in counts:
            for n in HC.COUNTS:
                assert (name, fn, json.dumps(good[:pos] + [n] + good[pos + 1:])) in plans
        for fn in HC.signatures(_lib, name):
            if fn != HC.LAST_ERROR[name]:
                assert "null" in kinds[(name, fn)], fn
    takes_work = {"sta_nn_build", "sta_nn_query", "sta_tsdf_blocks", "sta_tsdf_mesh", "sta_mesh_triangles", "sta_mesh_vertex_normals", "sta_surf_components",
                  "sta_surf_weights", "sta_simp_cells", "sta_simp_triangles", "sta_simp_place", "sta_tri_build"}
    assert {fn for (_n, fn), k in kinds.items() if "work_short" in k} == takes_work
    assert {fn for (_n, fn), k in kinds.items() if "index_short" in k} == {"sta_nn_build", "sta_tri_build"}
    for r in records:
        if r["kind"].endswith("_short"):
            assert " needed for " in r["error"] and " bytes, " in r["error"], r


def test_the_values_of_the_issue():
    """three answers written down independently of the recording"""
    assert call("dist", "sta_tri_plan", [6372, 3000, "out"])["sizes"] == [277504, 227584]
    assert call("simp", "sta_simp_plan", [1, 1, "out"])["sizes"] == [3584, 4608, 6144]
    assert call("dist", "sta_tri_plan", [0, 5, "out"]) == {"rc": -1, "error": "tri_plan: nt must be in [1, 2^27) (got 0)", "sizes": []}


def test_the_error_buffers_are_separate():
    """a failing call in one library leaves the last error of every other library as it was"""
    fail = {name: (HC.PLANS[name][0], HC.PLANS[name][1][:-1] + ["null"]) for name in HC.LIBRARIES}
    text = {}
    for name, (fn, args) in fail.items():
        r = call(name, fn, args)
        assert r["rc"] == -1
        text[name] = r["error"]
    assert len({t for t in text.values() if t != "null argument"}) == 6          # libsta_cloud.so does not name the call
    for a in HC.LIBRARIES:
        # a different message in a, so that a write into another buffer would show
        fn, good, _counts = HC.PLANS[a]
        pos, v = HC.RANGES[a][0]
        before = {b: getattr(library(b), HC.LAST_ERROR[b])() for b in HC.LIBRARIES}
        r = call(a, fn, good[:pos] + [v] + good[pos + 1:])
        assert r["rc"] == -1 and r["error"] != text[a]
        for b in HC.LIBRARIES:
            now = getattr(library(b), HC.LAST_ERROR[b])()
            assert now == (r["error"].encode() if b == a else before[b]), (a, b, now)
        assert call(a, *fail[a])["error"] == text[a]
