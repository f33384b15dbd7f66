"""Host only: every product entry point that runs on a stream's scratch context has a row in tests/workspace_cases.py, and every
entry point named there is one - so an entry point added later without a row in the workspace-independence matrix
(tests/test_workspace_gpu.py) fails here, without a GPU.

The parser is deliberately simple.  A function starts at a line that begins with `extern "C"` or `static` and ends in `(...) {`
(possibly some lines later); a lambda or a struct inside it does not start a new one.  A function TAKES the scratch when its body
calls plan_and_run( - the planned route - or cur_bump( - phase B of a split-phase scheduler call, which goes on in the workspace its
phase A planned.  The entry points are the functions of the product ABI (vista_slam_amd/_lib.py SIGNATURES = include/sta_mi355.h;
the sta_debug_* / sta_bench_* hooks of the test library are not in it) that take the scratch themselves or call, through any chain
of functions of csrc, one that does.
"""
import pathlib
import re

import workspace_cases as WC
from vista_slam_amd import _lib

CSRC = pathlib.Path(__file__).resolve().parents[1] / "vista_slam_amd" / "csrc"
START = re.compile(r'^(?:extern "C"|static|template\s*<[^>]*>\s*static)\s[^;(]*?\b([A-Za-z_]\w*)\s*\(')
TAKES = re.compile(r"\b(?:plan_and_run|cur_bump)\s*\(")
CALL = re.compile(r"\b([A-Za-z_]\w*)\s*\(")


def functions(root=CSRC):
    """-> {name: body text} of every top-level function of the .hip / .inc files under root (comments stripped)."""
    found = {}
    for f in sorted(root.iterdir()):
        if f.suffix not in (".hip", ".inc"):
            continue
        cur, depth, pending = None, 0, None
        for line in f.read_text().splitlines():
            code = line.split("//")[0]
            if depth == 0 and cur is None:
                m = START.match(code)
                if m and pending is None:
                    pending = m.group(1)
                    if pending in ("int", "void", "inline"):      # (the regex landed on a qualifier: no function here)
                        pending = None
            if pending is not None and depth == 0:
                if "{" in code:
                    cur, pending = pending, None
                    found[cur] = ""
                elif ";" in code:
                    pending = None          # a declaration
            if cur is not None:
                found[cur] += code + "\n"
            depth += code.count("{") - code.count("}")
            if depth <= 0:
                depth = 0
                if cur is not None and "{" in found[cur]:
                    cur = None
    return found


def scratch_entry_points(root=CSRC, abi=None):
    """-> {entry point: the function through which it takes the scratch} for the functions of `abi` (default: the product ABI)."""
    abi = set(_lib.SIGNATURES) if abi is None else set(abi)
    fns = functions(root)
    takers = {n: n for n, body in fns.items() if n not in ("plan_and_run", "cur_bump") and TAKES.search(body)}
    grew = True
    while grew:                      # callers of takers are takers
        grew = False
        for n, body in fns.items():
            if n in takers:
                continue
            hit = next((c for c in CALL.findall(body) if c in takers and c != n), None)
            if hit:
                takers[n] = hit
                grew = True
    return {n: via for n, via in takers.items() if n in abi}


def test_parser_sees_the_known_shapes_of_a_call_site(tmp_path):
    """A direct call, a call through a static helper, through a template helper with a lambda, through another entry point, phase B's
    cur_bump, a multi-line signature; and what is none: a comment, a test hook, a function that only declares."""
    (tmp_path / "a.hip").write_text(
        "template <class F>\n"
        "static int plan_and_run(sta_handle* h, hipStream_t st, F&& body) { return body(ws); }\n"
        "static Bump cur_bump(sta_handle* h) { return Bump{}; }\n"
        'extern "C" int sta_direct(sta_handle* h, void* stream) {\n'
        "    return plan_and_run(h, st, [&](Bump& ws) { return impl(h, ws); });\n"
        "}\n"
        "static int helper_any(sta_handle* h, const void* img,\n"
        "                      void* stream) {\n"
        "    struct Guard { sta_handle* h; ~Guard() { } } g{h};\n"
        "    return plan_and_run(h, st, [&](Bump& ws) {\n"
        "        return impl(h, ws);\n"
        "    });\n"
        "}\n"
        'extern "C" int sta_via_helper(sta_handle* h, void* stream) { return helper_any(h, nullptr, stream); }\n'
        'extern "C" int sta_via_entry(sta_handle* h, void* stream) {\n'
        "    CHK(sta_direct(h, stream));\n"
        "    return 0;\n"
        "}\n"
        'extern "C" int sta_phase_b(sta_handle* h, void* stream) {\n'
        "    Bump ws = cur_bump(h);\n"
        "    return 0;\n"
        "}\n"
        'extern "C" int sta_plain(sta_handle* h) {   // would call plan_and_run( if it needed scratch\n'
        "    return 0;\n"
        "}\n"
        'extern "C" int sta_debug_hook(sta_handle* h, void* stream) { return plan_and_run(h, st, [&](Bump& ws) { return 0; }); }\n')
    (tmp_path / "b.inc").write_text('extern "C" int sta_in_inc(sta_handle* h, void* stream) { return helper_any(h, nullptr, stream); }\n')
    abi = {"sta_direct", "sta_via_helper", "sta_via_entry", "sta_phase_b", "sta_plain", "sta_in_inc"}
    assert scratch_entry_points(tmp_path, abi) == {"sta_direct": "sta_direct", "sta_via_helper": "helper_any", "sta_via_entry": "sta_direct",
                                                   "sta_phase_b": "sta_phase_b", "sta_in_inc": "helper_any"}


def test_every_scratch_entry_point_has_a_row():
    found = scratch_entry_points()
    named = WC.named_entries()
    assert not (named & set(WC.EXEMPT)), sorted(named & set(WC.EXEMPT))
    missing = {k: v for k, v in found.items() if k not in named and k not in WC.EXEMPT}
    stale = (named | set(WC.EXEMPT)) - set(found)
    assert not missing, f"entry points that take a stream's scratch (through the function named) without a row in tests/workspace_cases.py: {missing}"
    assert not stale, f"tests/workspace_cases.py names entry points that do not take a stream's scratch (any more): {sorted(stale)}"
    assert len(found) >= 25, found          # the parser itself went blind
    for name, reason in {**WC.EXEMPT, **WC.NO_SCRATCH}.items():
        assert reason.strip(), name
    assert set(WC.NO_SCRATCH) <= set(_lib.SIGNATURES) and not (set(WC.NO_SCRATCH) & set(found)), sorted(set(WC.NO_SCRATCH) & set(found))


def test_the_matrix_is_well_formed():
    names = [c.name for c in WC.CASES]
    assert len(names) == len(set(names))
    for c in WC.CASES:
        assert c.entries and c.shapes and callable(c.make) and callable(c.run), c.name
        assert set(c.no_prec) <= set(WC.PRECISIONS), c.name
    assert set(WC.SPLIT_PHASE) <= set(names)
    for fam in WC.TRANSITION_FAMILIES:
        big, small = WC.family_extremes(fam)
        assert big.name != small.name and big.rank > small.rank, fam
    assert WC.FILLS == (0x00, 0xFF, 0x3C, 0x7B) and WC.MIN_TAIL == 64 << 10
    # the ctypes table knows the three hooks the GPU test drives
    assert {"sta_debug_workspace_fill", "sta_debug_workspace_info", "sta_debug_workspace_tail"} <= set(_lib.TEST_SIGNATURES)
