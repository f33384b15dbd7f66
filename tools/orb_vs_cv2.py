"""The restatement of the ORB contract (tests/loop_cases.py, the yardstick of csrc/loop.h) next to OpenCV, where cv2 can be imported:
how many keypoints of cv2.ORB_create().detectAndCompute the restatement finds too (same level, same pixel), how their angles differ,
and - with cv2's learned comparison table unavailable to the restatement - how many descriptor bits differ on the common keypoints
under the procedural table (about half: the tables differ; with cv2's table passed as `pattern=` the figure is the real agreement).
No GPU.  The stated differences (1-degree angle bins, integer Harris order, the blur kernel, 11-bit bilinear resizing, no tie
extension at the second cut) make small differences expected; this tool prints them, it asserts nothing.

    python tools/orb_vs_cv2.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import flow_cases as F                                     # noqa: E402
import loop_cases as L                                     # noqa: E402

try:
    import cv2
except ImportError:
    print("cv2 not available")
    sys.exit(0)

for H, W in ((224, 224), (384, 512)):
    img = F.blob_frame(H, W, n_blobs=400)
    kp, resp, desc = L.extract(img)
    theirs, tdesc = cv2.ORB_create().detectAndCompute(img, None)
    tdesc = np.zeros((0, 32), np.uint8) if tdesc is None else tdesc
    scale = [1.2 ** l for l in range(8)]
    mine = {(int(l), int(x), int(y)): i for i, (x, y, l, _) in enumerate(kp)}
    common, dang, bits = 0, [], []
    for j, k in enumerate(theirs):
        key = (k.octave, int(round(k.pt[0] / scale[k.octave])), int(round(k.pt[1] / scale[k.octave])))
        if key in mine:
            i = mine[key]
            common += 1
            dang.append(abs((kp[i, 3] - k.angle + 180.0) % 360.0 - 180.0))
            bits.append(int(np.unpackbits(desc[i] ^ tdesc[j]).sum()))
    print(f"{H} x {W}: keypoints {len(kp)} (restatement) / {len(theirs)} (cv2), {common} at the same level and pixel; angle difference "
          f"median {np.median(dang) if dang else float('nan'):.2f} deg, worst {max(dang) if dang else float('nan'):.2f}; descriptor bits that differ "
          f"(procedural table against cv2's): median {np.median(bits) if bits else float('nan'):.0f} of 256")
