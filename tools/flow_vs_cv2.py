"""The restatement of the keyframe gate (tests/flow_cases.py, the yardstick of csrc/flow.h) next to OpenCV, where cv2 can be imported:
corner-set overlap and position differences of goodFeaturesToTrack, and the differences of calcOpticalFlowPyrLK's positions and
status on the restatement's corners.  No GPU.  The restatement is integer and float64 by contract and OpenCV is float32 with SIMD
paths, so small differences are expected; this tool prints them, it asserts nothing.

    python tools/flow_vs_cv2.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import flow_cases as F                                     # noqa: E402

try:
    import cv2
except ImportError:
    print("cv2 not available")
    sys.exit(0)

for H, W in ((96, 128), (224, 224)):
    a = F.blob_frame(H, W)
    ours = F.good_features(a)
    theirs = cv2.goodFeaturesToTrack(a, maxCorners=1000, qualityLevel=0.01, minDistance=8, blockSize=7)
    theirs = np.zeros((0, 2), np.float32) if theirs is None else theirs.reshape(-1, 2)
    so, st = {tuple(p) for p in ours.tolist()}, {tuple(p) for p in theirs.tolist()}
    same_rank = sum(1 for p, q in zip(ours.tolist(), theirs.tolist()) if p == q)
    print(f"{H} x {W}: corners {len(ours)} (restatement) / {len(theirs)} (cv2), {len(so & st)} in both sets, {same_rank} at the same rank")
    for shift in ((1.25, -0.5), (5.5, 3.25)):
        b = F.blob_frame(H, W, shift)
        o_pts, o_st = F.track(a, b, ours)
        c_pts, c_st, _ = cv2.calcOpticalFlowPyrLK(a, b, ours.reshape(-1, 1, 2), None, winSize=(21, 21), maxLevel=3,
                                                  criteria=(cv2.TERM_CRITERIA_EPS | cv2.TERM_CRITERIA_COUNT, 30, 0.01))
        c_pts, c_st = c_pts.reshape(-1, 2), c_st.reshape(-1)
        both = (o_st == 1) & (c_st == 1)
        d = np.hypot(*(o_pts[both] - c_pts[both]).T) if both.any() else np.zeros(1)
        mo = F.disparity(ours, o_pts, o_st)
        mc = float(np.mean(np.linalg.norm(c_pts[c_st == 1] - ours[c_st == 1], axis=1))) if (c_st == 1).any() else float("nan")
        print(f"    shift {shift}: status differs at {int((o_st != c_st).sum())} of {len(ours)} points; positions differ by median {np.median(d):.2e} px, "
              f"worst {d.max():.2e} px; mean displacement {mo[2] / max(mo[1], 1):.6f} (restatement) / {mc:.6f} (cv2)")
