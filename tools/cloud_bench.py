"""libsta_cloud.so on the GPU: index build and nearest-neighbour query at 2 M and 20 M points, a whole `evaluate.eval_recon`, and a
chunked torch.cdist + min brute force on the same GPU for the same result.  Medians of `reps` runs (default 20) between device events;
eval_recon, which reads back on the host, is timed with a host clock around a synchronised call.

    python tools/cloud_bench.py [reps] [small]      # small: 2 M points only, and a 10-view eval_recon

The clouds are two samplings of the procedural room of tools/voxel_bench.py (16 x 12 x 4 m, 1 cm of noise): the reference and the
queries lie on the same surfaces, as a reconstruction and its ground truth do.  Two query settings: ICP's (radius = cell = 0.1 on
the clouds down-sampled to 0.05) and chamfer's (radius 0.5 on the full clouds) at several cells, with every query matched and - at
2 M - with 5 % of the queries moved beyond the radius, the worst case of a query (it walks every ring);
`cloud.CHAMFER_CELL_FRACTION` is chosen from those tables.  What cannot be measured here: the reference's CPU route (Open3D's ICP, pykdtree) - neither is installed."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from vista_slam_amd import cloud, evaluate, formats, weights as W   # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend             # noqa: E402

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 20
small = "small" in sys.argv[1:]
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)


def room(M, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    size = torch.tensor([16.0, 12.0, 4.0], device="cuda")
    p = torch.rand(M, 3, device="cuda", generator=g) * size
    face = torch.randint(0, 6, (M,), device="cuda", generator=g)
    axis, side = face // 2, (face % 2).float()
    p.scatter_(1, axis[:, None], (side * size[axis])[:, None])
    p += 0.01 * torch.randn(M, 3, device="cuda", generator=g)
    return p.contiguous()


def event_ms(fn, n):
    """median and spread of n runs between device events, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), max(out) - min(out)


def line(what, med, spread, extra=""):
    print(f"    {what:58s} median {med:9.3f} ms  spread {spread:8.3f}  {extra}", flush=True)


print(f"{torch.cuda.get_device_name(0)}; medians of {reps} runs between device events", flush=True)
for M in ((2_000_000,) if small else (2_000_000, 20_000_000)):
    ref, qry = room(M, 2500 + M // 1_000_000), room(M, 2600 + M // 1_000_000)
    print(f"{M} reference points, {M} queries", flush=True)
    # ICP's setting: both clouds down-sampled to 0.05, radius = cell = 0.1
    rd, _ = formats.voxel_downsample(m, ref, voxel_size=0.05)
    qd, _ = formats.voxel_downsample(m, qry, voxel_size=0.05)
    med, sp = event_ms(lambda: cloud.NNIndex.build(rd, 0.1), reps)
    ix = cloud.NNIndex.build(rd, 0.1)
    line(f"build  {len(rd)} down-sampled points, cell 0.1", med, sp, f"{ix.cells} cells")
    med, sp = event_ms(lambda: ix.query(qd, 0.1, want=("record",)), reps)
    rec = cloud.Record.from_array(ix.query(qd, 0.1, want=("record",))["record"].cpu().numpy())
    line(f"query  {len(qd)} down-sampled queries, radius 0.1, record only", med, sp, f"{rec.matched} matched (one ICP evaluation)")
    del ix, rd, qd
    # chamfer's setting: full clouds, radius 0.5
    for frac in (4, 8, 16, 32):
        cell = 0.5 / frac
        med, sp = event_ms(lambda: cloud.NNIndex.build(ref, cell), reps)
        ix = cloud.NNIndex.build(ref, cell)
        line(f"build  {M} points, cell 0.5/{frac}", med, sp, f"{ix.cells} cells, {M / ix.cells:.1f} points per cell")
        n = reps
        med, sp = event_ms(lambda: ix.query(qry, 0.5, want=("record",)), n)
        rec = cloud.Record.from_array(ix.query(qry, 0.5, want=("record",))["record"].cpu().numpy())
        line(f"query  {M} queries, radius 0.5, cell 0.5/{frac}, record only ({n} runs)", med, sp,
             f"{rec.matched} matched, rmse {np.sqrt(rec.sum_clipped / rec.finite):.5f}")
        del ix
    if M == 2_000_000:
        # the worst case of a query: nothing inside the radius, so every ring up to the last is walked (kmax = frac + 1 rings, about
        # 4/3 kmax^3 row visits with a binary search each), and the 63 other lanes of its wave wait for it.  5 % of the queries are
        # moved into the room's interior, at least 1 m from every surface: the outliers the metric clips at max_error.
        g = torch.Generator(device="cuda").manual_seed(2800)
        out = torch.rand(M, device="cuda", generator=g) < 0.05
        inside = torch.rand(M, 3, device="cuda", generator=g) * torch.tensor([14.0, 10.0, 2.0], device="cuda") + 1.0
        qo = torch.where(out[:, None], inside, qry).contiguous()
        for frac in (4, 8, 16, 32):
            ix = cloud.NNIndex.build(ref, 0.5 / frac)
            med, sp = event_ms(lambda: ix.query(qo, 0.5, want=("record",)), reps)
            rec = cloud.Record.from_array(ix.query(qo, 0.5, want=("record",))["record"].cpu().numpy())
            line(f"query  {M} queries, 5 % beyond the radius, cell 0.5/{frac} ({reps} runs)", med, sp,
                 f"{rec.finite - rec.matched} unmatched, rmse {np.sqrt(rec.sum_clipped / rec.finite):.5f}")
            del ix
        del qo, inside, out
    del ref, qry
    torch.cuda.empty_cache()

# brute force for the same result, alternating, at a size where it finishes: float64 distances in chunks, min over the reference
Mb = 100_000
ref, qry = room(Mb, 2701), room(Mb, 2702)
ix = cloud.NNIndex.build(ref, 0.5 / 16)


def brute():
    r64 = ref.double()
    best = torch.empty(Mb, dtype=torch.float64, device="cuda")
    arg = torch.empty(Mb, dtype=torch.int64, device="cuda")
    for s in range(0, Mb, 4096):
        d = torch.cdist(qry[s:s + 4096].double(), r64)
        best[s:s + 4096], arg[s:s + 4096] = d.min(dim=1)
    return best, arg


ours = lambda: ix.query(qry, 0.5, want=("d2", "idx"))           # noqa: E731
t = {"hip": [], "torch": []}
for f in (ours, brute):
    f()
for _ in range(reps):
    for k, f in (("hip", ours), ("torch", brute)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = f()
        b.record()
        torch.cuda.synchronize()
        t[k].append(a.elapsed_time(b))
o, (bd, ba) = ours(), brute()
same = int((o["idx"].long() == ba).sum())
print(f"brute force, {Mb} x {Mb}, float64 cdist in chunks of 4096 + min, alternating ({len(t['hip'])} runs each):", flush=True)
line("grid query (d2 and idx), cell 0.5/16", float(np.median(t["hip"])), max(t["hip"]) - min(t["hip"]))
line("torch.cdist + min", float(np.median(t["torch"])), max(t["torch"]) - min(t["torch"]),
     f"ratio {np.median(t['torch']) / np.median(t['hip']):.1f}; {same} of {Mb} indices equal, largest |d - d| {float((o['d2'].sqrt() - bd).abs().max()):.3g}")
del ref, qry, ix
torch.cuda.empty_cache()


# a whole eval_recon: N views of 224 x 224 looking at a stepped wall from a moving camera; the estimate is the ground truth in a
# Sim(3)-moved frame with 0.2 % depth noise
def scene(N, H=224, Wd=224):
    g = torch.Generator(device="cuda").manual_seed(77)
    K = torch.tensor([[200.0, 0, Wd / 2], [0, 200.0, H / 2], [0, 0, 1]], device="cuda")
    v, u = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(Wd, device="cuda").float(), indexing="ij")
    i = torch.arange(N, device="cuda").float()[:, None, None]
    gt_d = 2.0 + 0.002 * (u - Wd / 2) + 0.001 * (v - H / 2) + 0.3 * (u > Wd / 2 + 2 * i).float() + 0.01 * i
    gt_p = torch.eye(4, device="cuda").repeat(N, 1, 1)
    gt_p[:, 0, 3], gt_p[:, 1, 3], gt_p[:, 2, 3] = 0.1 * i[:, 0, 0], 0.05 * torch.sin(i[:, 0, 0]), 0.02 * i[:, 0, 0]
    s = 1.25
    th = 0.15
    R = torch.tensor([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], device="cuda", dtype=torch.float32)
    t = torch.tensor([0.3, -0.2, 0.5], device="cuda")
    est_p = gt_p.clone()
    est_p[:, :3, :3] = R.T @ gt_p[:, :3, :3]
    est_p[:, :3, 3] = ((gt_p[:, :3, 3] - t) @ R) / s
    est_d = gt_d / s * (1 + 0.002 * torch.randn(N, H, Wd, device="cuda", generator=g))
    mask = (torch.rand(N, H, Wd, device="cuda", generator=g) > 0.1).float()
    return dict(gt_depths=gt_d, gt_poses=gt_p, gt_intri=K, est_depths=est_d, est_poses=est_p, est_intris=K.repeat(N, 1, 1), est_masks=mask,
                rel_R=R.double().cpu().numpy(), rel_t=t.double().cpu().numpy(), rel_s=s)


N = 10 if small else 40
sc = scene(N)
evaluate.eval_recon(m, **sc)
ts = []
for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate.eval_recon(m, **sc, return_stages=True)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
reg = out[5]["icp"]
print(f"eval_recon, {N} views of 224 x 224 ({len(out[3])} gt points, {len(out[4])} est points; {len(out[5]['gt_down'])} / {len(out[5]['est_down'])} after "
      f"0.05 down-sampling), host clock around a synchronised call, {len(ts)} runs:", flush=True)
line(f"eval_recon (ICP: {reg.iterations} iterations, {reg.status})", float(np.median(ts)), max(ts) - min(ts),
     f"acc {out[0]:.5f} comp {out[1]:.5f} chamfer {out[2]:.5f}")
