"""Host only: every fp16 plane writer of vista_slam_amd/csrc is classified in tests/range_cases.py - as REPORTING, with at least one
test of tests/test_range_gpu.py that drives it, or as EXEMPT, with the reason.  A writer added later without being classified fails
here, without a GPU.

The parser is deliberately simple: the enclosing function of a line is the last `__global__` / `__device__` signature above it, its
name the first identifier followed by `(` behind the qualifiers.  A writer is a function that declares a RangeAcc, hands a range
pointer (`rng`, `p.rng`, `p.range`) to split_f16 / to_f16_sat / split_mx4 / store_mx1, or does atomicAdd(p.range, ...).
"""
import pathlib
import re

import range_cases as RC

CSRC = pathlib.Path(__file__).resolve().parents[1] / "vista_slam_amd" / "csrc"
SIG = re.compile(r"__(?:global|device)__")
NAME = re.compile(r"\b([A-Za-z_]\w*)\s*\(")
USE = re.compile(r"\bRangeAcc\s+\w+\s*;"
                 r"|\b(?:split_f16|to_f16_sat|split_mx4(?:<\w+>)?|store_mx1(?:<\w+>)?)\s*\([^;]*?\b(?:rng|p\.rng|p\.range)\s*\)"
                 r"|atomicAdd\(\s*p\.range")


def find_writers(root=CSRC):
    """-> {function name: ["file:line", ...]} of every writer in the .h / .inc files under root."""
    found = {}
    for f in sorted(root.iterdir()):
        if f.suffix not in (".h", ".inc"):
            continue
        cur = None
        for i, line in enumerate(f.read_text().splitlines(), 1):
            code = line.split("//")[0]
            sig = SIG.search(code)
            if sig:
                m = NAME.search(re.sub(r"__launch_bounds__\s*\([^)]*\)", "", code[sig.end():]))
                if m:
                    cur = m.group(1)
            if USE.search(code) and cur not in RC.HELPERS:
                found.setdefault(cur, []).append(f"{f.name}:{i}")
    return found


def test_parser_sees_the_known_shapes_of_a_writer(tmp_path):
    """The three ways a writer shows up, a multi-line signature, a launch bound, and a helper definition that is not one."""
    (tmp_path / "k.h").write_text(
        "template <bool SPLIT>\n"
        "__global__ __launch_bounds__(256) void a_kernel(const P p) {\n"
        "    RangeAcc ra;   // a comment that names b_kernel( does not count\n"
        "}\n"
        "__global__ void b_kernel(const float* x,\n"
        "                         unsigned long long* rng) {\n"
        "    f16 h, l; split_f16(x[0], h, l, rng);\n"
        "}\n"
        "__device__ __forceinline__ void c_tile(const P& p) { if (bad) atomicAdd(p.range, 1ull); }\n"
        "template <bool W> __device__ __forceinline__ void d_tile(const P& p) { store_mx1<false>(p.C, o, v, p.range); }\n"
        "__device__ __forceinline__ f16 to_f16_sat(float x, unsigned long long* rng) { RangeAcc ra; return (f16)x; }\n"
        "__device__ void e_reader(const P& p) { float v = load(p.range); }\n")
    assert set(find_writers(tmp_path)) == {"a_kernel", "b_kernel", "c_tile", "d_tile"}


def test_every_plane_writer_is_classified():
    found = find_writers()
    classified = {RC.base(k) for k in RC.REPORTING} | {RC.base(k) for k in RC.EXEMPT}
    missing = {k: v for k, v in found.items() if k not in classified}
    stale = classified - set(found)
    assert not missing, f"plane writers that tests/range_cases.py does not classify (REPORTING with a GPU case, or EXEMPT with the reason): {missing}"
    assert not stale, f"tests/range_cases.py classifies functions that are no plane writers (any more): {sorted(stale)}"
    assert len(found) >= 20, found          # the parser itself went blind


def test_every_reporting_writer_names_a_case_that_exists():
    src = (pathlib.Path(__file__).parent / "test_range_gpu.py").read_text()
    defined = set(re.findall(r"^def (test_\w+)\(", src, re.M))
    for name, (counters, cases) in RC.REPORTING.items():
        assert cases, f"{name}: a reporting writer needs at least one GPU case"
        assert set(counters.replace(" ", "").split(",")) <= {"0", "1"}, name
    for name in RC.EXEMPT:
        assert RC.EXEMPT[name].strip(), name
        assert name in RC.EXEMPT_CASES, f"{name}: no test pins the value this exempt writer stores"
    assert set(RC.EXEMPT_CASES) == set(RC.EXEMPT)
    unknown = RC.all_case_names() - defined
    assert not unknown, f"cases named in tests/range_cases.py that tests/test_range_gpu.py does not define: {sorted(unknown)}"


def test_hot_table_follows_the_thresholds():
    """The expected classes of range_cases.HOT are the rule (> 65504; > 57344 on f16mx rows), and every value is built as it says."""
    for v, ((a, w, d), planes, mx) in RC.HOT.items():
        assert a * w + d == v and abs(a) < RC.E5M2_MAX and abs(w) <= RC.E4M3_W_MAX, v
        assert planes == RC.class_of(v, False) and mx == RC.class_of(v, True), v
