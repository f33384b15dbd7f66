"""Host only: the skew points of csrc/sta_skew.h stand where tests/test_skew_gpu.py needs them.

Over the twelve kernel headers of the main translation unit: every __syncthreads(), __syncthreads_or / _and / _count() and every raw s_barrier statement of a kernel with
more than one wave per workgroup is followed, on its line, by STA_SKEW(id); ids are unique over all files; and every file holds
exactly the points counted here - its barrier sites, its kernel entries (STA_SKEW_ENTRY: the kernels and kernel bodies that reach a
barrier) and its epilogue points (STA_SKEW_EPI).  The barriers of one-wave kernels (__launch_bounds__(64)) carry none: nothing can be
skewed there.  Without -DSTA_WAVE_SKEW the three macros expand to nothing, and no other header uses them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vista_slam_amd", "csrc")

# header -> (barrier sites of multi-wave kernels, entry points, epilogue points, barrier sites of one-wave kernels)
POINTS = {
    "gemm.h": (3, 2, 1, 0),           # qkv_finish_kernel, gemm_kernel; the epilogue of gemm_kernel
    "gemm2.h": (13, 1, 2, 0),         # 8 __syncthreads + 5 counted-wait barriers of the ring; gemm2_body; the epilogues of the body and of gemm2_tail
    "conv3h.h": (4, 2, 2, 0),         # the kernel and its varlen body, an epilogue each
    "attention.h": (7, 3, 1, 0),      # attn_kernel, attn_mixed_kernel, attn_varlen_kernel; the output stage
    "elementwise.h": (10, 7, 0, 0),
    "select.h": (9, 1, 0, 0),         # sel_block_scan's barrier is reached from voxel.h's kernels as well
    "voxel.h": (14, 10, 0, 0),
    "geo.h": (5, 5, 0, 0),
    "flow.h": (8, 4, 0, 5),           # flow_track_kernel is one wave
    "loop.h": (10, 4, 0, 0),
    "pgo.h": (14, 3, 0, 0),          # 13 __syncthreads() + the __syncthreads_or() in front of the first product
    "graph.h": (1, 1, 0, 1),          # graph_link_kernel is one wave
}
BARRIER = re.compile(r"__syncthreads(?:_or|_and|_count)?\([^;]*\);|asm volatile\(\"[^\"]*s_barrier\"[^;]*\);")


def code_lines(name):
    """(line number, code without the // comment) of a header."""
    out = []
    for i, ln in enumerate(open(os.path.join(CSRC, name)).read().split("\n"), 1):
        out.append((i, ln.split("//")[0]))
    return out


def scan(name):
    """-> (ids behind barriers, entry ids, epilogue ids, bare barrier sites [(line, one-wave kernel?)])"""
    behind, entries, epis, bare = [], [], [], []
    one_wave = False
    for i, code in code_lines(name):
        s = code.strip()
        if s.startswith("__global__"):
            m = re.search(r"__launch_bounds__\(([^)]*)\)", s)
            one_wave = bool(m and m.group(1).strip() == "64")
        elif s.startswith("__device__") and "(" in s:
            one_wave = False
        entries += [int(x) for x in re.findall(r"STA_SKEW_ENTRY\((\d+)\)", code)]
        epis += [int(x) for x in re.findall(r"STA_SKEW_EPI\((\d+)\)", code)]
        for m in BARRIER.finditer(code):
            follow = re.match(r"\s*STA_SKEW\((\d+)\);", code[m.end():])
            if follow:
                behind.append(int(follow.group(1)))
            else:
                bare.append((i, one_wave))
        # a skew point that follows no barrier on its line
        n_points = len(re.findall(r"STA_SKEW\(\d+\)", code))
        assert n_points == len([m for m in BARRIER.finditer(code) if re.match(r"\s*STA_SKEW\(\d+\);", code[m.end():])]), (name, i, code)
    return behind, entries, epis, bare


def test_every_barrier_of_a_multi_wave_kernel_is_followed_by_a_point():
    for name, (n_bar, _e, _p, n_one) in POINTS.items():
        behind, _entries, _epis, bare = scan(name)
        assert all(one for _line, one in bare), (name, [line for line, one in bare if not one])
        assert len(bare) == n_one, (name, bare)
        assert len(behind) == n_bar, (name, len(behind), n_bar)


def test_counts_per_file_and_unique_ids():
    seen = {}
    for name, (n_bar, n_entry, n_epi, _one) in POINTS.items():
        behind, entries, epis, _bare = scan(name)
        assert (len(behind), len(entries), len(epis)) == (n_bar, n_entry, n_epi), (name, len(behind), len(entries), len(epis))
        for i in behind + entries + epis:
            assert i not in seen, (i, name, seen[i])
            seen[i] = name
    assert len(seen) == sum(a + b + c for a, b, c, _ in POINTS.values())


def test_no_other_source_uses_the_macros_and_the_default_is_nothing():
    for f in sorted(os.listdir(CSRC)):
        if f in POINTS or f == "sta_skew.h":
            continue
        assert not re.search(r"STA_SKEW(_ENTRY|_EPI)?\(", open(os.path.join(CSRC, f)).read()), f
    src = open(os.path.join(CSRC, "sta_skew.h")).read()
    tail = src.split("#else")[1]
    assert re.findall(r"#define (STA_SKEW\w*)\(id\)[ \t]*\n", tail) == ["STA_SKEW", "STA_SKEW_ENTRY", "STA_SKEW_EPI"], tail
    assert "__syncthreads" not in src.split("#ifdef STA_WAVE_SKEW")[1] and "__shared__" not in src      # a point adds no barrier and no LDS


def test_only_the_skew_library_is_built_with_the_flag():
    from vista_slam_amd import build
    assert build.SKEW_FLAGS == ["-DSTA_TEST_HOOKS", "-DSTA_WAVE_SKEW"]
    assert "-DSTA_WAVE_SKEW" not in build.BASE_FLAGS + build.extra_flags()
    # the header enters the content hash of every library whose sources include it: the main translation unit and the users of voxel.h
    users = [n for n in list(build.SATELLITES) + list(build.ADDONS) if "voxel.h" in getattr(build, n.upper() + "_DEPS")]
    assert "sta_skew.h" in build.DEPS and users == ["cloud", "tsdf", "mesh", "simp", "dist"]
    for n in list(build.SATELLITES) + list(build.ADDONS):
        assert ("sta_skew.h" in getattr(build, n.upper() + "_DEPS")) == (n in users), n
    assert build.source_hash(None, build.SKEW_FLAGS) != build.source_hash()
