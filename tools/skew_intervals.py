"""The barrier-to-barrier intervals behind the repeat counts of tests/test_skew_gpu.py (profiles/r33_wave_skew.txt).

    python tools/skew_intervals.py [case id substring ...]

1. The in-kernel stamps of the test-hooks library (sta_bench_gemm_stamps: entry, first K tile landed, main loop done, epilogue
   acknowledged) on the dense GEMM shapes of the skew cases: entry -> first tile, main loop per K tile, epilogue.
2. Every case of tests/test_skew_gpu.py once on libsta_mi355_skew.so in its measuring mode (bit 16 of the wave mask: every skew point of
   every wave notes the 100 MHz clock, nothing is delayed): the largest distance between two consecutive points of one wave of one
   launch - the longest barrier-to-barrier interval, the wait at the barrier included.  This covers the kernels that have no stamps.
Prints, per group, the largest interval and ceil(4 x interval / 3.39 us): the s_sleep 127 per point that test_skew_gpu.py uses.
"""
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stamps():
    import torch
    from vista_slam_amd import _lib, weights as W
    from vista_slam_amd.sta_frontend import STAFrontend
    m = STAFrontend(W.TINY, "cuda:0", precision="f16x3", lib=_lib.load_test()).load_procedural()
    st = torch.cuda.current_stream().cuda_stream
    print("in-kernel stamps, test-hooks library, f16x3 (us; medians over the workgroups)")
    print(f"{'M':>6s} {'N':>5s} {'K':>5s} {'resid':>5s} {'WGs':>5s} {'ks':>3s} {'->tile0':>8s} {'loop':>8s} {'loop/Ktile':>10s} {'epilogue':>8s}")
    for M, N, K, r in ((6145, 768, 64, 1), (6160, 768, 256, 0), (6913, 768, 224, 0), (6928, 768, 192, 1), (100, 256, 1024, 0),
                       (513, 768, 128, 1), (3076, 2304, 768, 0), (196, 768, 768, 1)):
        out = (C.c_double * 10)()
        for _ in range(2):
            _lib.check(m.lib.sta_bench_gemm_stamps(m._h, M, N, K, r, out, None, 0, st))
        o = list(out)
        ks = max(1, int(o[8]))
        print(f"{M:6d} {N:5d} {K:5d} {r:5d} {int(o[0]):5d} {ks:3d} {o[2]:8.2f} {o[3]:8.2f} {o[3] / max(1, K // 32 // ks):10.3f} {o[4]:8.2f}", flush=True)
    del m


def measured(filters):
    import test_skew_gpu as TS
    c = TS.Ctx()
    worst = {}
    print("\nlargest interval between two skew points of one wave, skew library in measuring mode")
    print(f"{'case':32s} {'group':10s} {'interval us':>11s}")
    # (the largest system of tests/test_pgo_gpu.py bounds the solves of the file, which runs the two smallest)
    for cid, nw, group, call in TS.CASES + [("pgo_solve_slam120 (bound only)", 16, "pgo", TS._pgo_solve("slam120"))]:
        if filters and not any(f in cid for f in filters):
            continue
        _hits, gap, _seen = TS.run_skewed(c, call, 0x10000, 0)
        us = gap * 0.01
        worst[group] = max(worst.get(group, 0.0), us)
        print(f"{cid:32s} {group:10s} {us:11.2f}", flush=True)
    print(f"\n{'group':10s} {'interval us':>11s} {'sleeps (4 x interval / %.2f us)' % TS.SLEEP_US:>32s}")
    for group, us in worst.items():
        print(f"{group:10s} {us:11.2f} {max(1, math.ceil(4.0 * us / TS.SLEEP_US)):32d}")
    if not filters:
        print(f"\ncommitted in tests/test_skew_gpu.py (the largest of the measuring runs)\n{'group':10s} {'interval us':>11s} {'sleeps per point':>32s}")
        for group, us in TS.INTERVAL_US.items():
            print(f"{group:10s} {us:11.2f} {TS.repeat_of(group):32d}   {'(this run is above it)' if worst.get(group, 0.0) > us else ''}")
    print("\npoints hit with every wave selected and no delay (ids of csrc/*.h)")
    for cid, nw, group, call in TS.CASES:
        if filters and not any(f in cid for f in filters):
            continue
        _hits, _gap, seen = TS.run_skewed(c, call, 0xFFFF, 0)
        print(f"{cid:32s} {sorted(seen)}  missing of MUST: {TS.missing_points(cid, seen)}", flush=True)


if __name__ == "__main__":
    stamps()
    measured(sys.argv[1:])
