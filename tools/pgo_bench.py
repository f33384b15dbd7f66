"""The Sim(3) pose graph (vista_slam_amd.pgo) timed on the GPU: `sta_pgo_index`, `sta_pgo_linearize` (full and cost-only) and
`sta_pgo_solve` on their own (device events around one call; the solve also as microseconds per PCG iteration), a whole
`pgo.optimize` call with its readbacks (host wall-clock), and - alongside, for scale - a torch float64 dense solve of the same damped
system on the same GPU: the Gauss-Newton matrix scattered into a dense [7n, 7n] tensor from the per-edge blocks (cheaper than forming
J and J^T W J, which the reference's autograd path does), `torch.linalg.cholesky` and `torch.cholesky_solve`.

    python tools/pgo_bench.py [reps]              # default 20 repetitions per row after 3 warm-up calls (5 for the dense solve)

Sizes: tests/pgo_cases.slam_graph(100) - live mode, pgo_every = 50, a window of 100 views - and slam_graph(400), all nodes free,
measurement noise 0.01.  Nobody has measured this stage on this hardware before and no target is set; the reference's pypose LM cannot
be run where pypose is absent.  The numpy restatement is a yardstick for results, not a baseline."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402
import pgo_cases as P                                      # noqa: E402
from vista_slam_amd import pgo, weights as W               # noqa: E402
from vista_slam_amd.sta_frontend import STAFrontend        # noqa: E402

nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
reps = nums[0] if nums else 20
m = STAFrontend(W.TINY, "cuda:0").load_procedural(seed=43)


def events(fn, reps=reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return float(np.median(t)), min(t), max(t)


def wall(fn, reps=reps):
    for _ in range(2):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), min(t), max(t)


def row(name, r, extra=""):
    print(f"    {name:58s} median {r[0]:11.1f} us   min {r[1]:11.1f}   max {r[2]:11.1f}{extra}", flush=True)


def dense(graph, lin, radius=1e4, dmin=1e-6, dmax=1e32):
    """(H + D / radius) d = -g with torch: H scattered from the per-edge blocks, Cholesky, two triangular solves"""
    n, e = graph.n, graph.edges.long()
    a, b, S = e[:, 0], e[:, 1], lin["S"]
    H = torch.zeros(n, n, 7, 7, device=S.device, dtype=torch.float64)
    H.index_put_((a, a), S, accumulate=True)
    H.index_put_((b, b), S, accumulate=True)
    H.index_put_((a, b), -S, accumulate=True)
    H.index_put_((b, a), -S, accumulate=True)
    H = H.permute(0, 2, 1, 3).reshape(7 * n, 7 * n)
    D = torch.diagonal(lin["blocks"], dim1=1, dim2=2).clamp(dmin, dmax).reshape(-1) / radius
    H.diagonal().add_(D)
    L = torch.linalg.cholesky(H)
    return torch.cholesky_solve(-lin["g"].reshape(-1, 1), L).reshape(n, 7)


print(f"{torch.cuda.get_device_name(0)}; {reps} repetitions per row after 3 warm-up calls")
for V in (100, 400):
    g = P.slam_graph(V)
    graph = pgo.Graph(m, len(g["nodes"]), g["edges"], g["poses"], g["confs"])
    nodes = torch.from_numpy(g["nodes"]).cuda()
    graph.index()
    lin = pgo.linearize(graph, nodes)
    d, stats = pgo.solve(graph, lin)
    st = stats.tolist()
    print(f"slam_graph({V}): {graph.n} nodes, {graph.E} edges, all free; workspace {graph.plan.workspace_bytes} B; f = {float(lin['rec'][0]):.4f}")
    print("  device events around one library call:")
    row("sta_pgo_index", events(graph.index))
    row("sta_pgo_linearize (r, S, v, f, g, diagonal blocks)", events(lambda: pgo.linearize(graph, nodes)))
    row("sta_pgo_linearize, cost only", events(lambda: pgo.linearize(graph, nodes, full=False)))
    for rtol in (1e-4, 1e-8):
        d, stats = pgo.solve(graph, lin, rtol=rtol)
        it = int(stats[0].item())
        r = events(lambda: pgo.solve(graph, lin, rtol=rtol))
        row(f"sta_pgo_solve, rtol {rtol:g}: {it} iterations", r, f"   {r[0] / max(it, 1):7.2f} us per iteration")
    try:
        x = dense(graph, lin)
        d8, _ = pgo.solve(graph, lin, rtol=1e-10)
        print(f"    (dense solve against PCG at rtol 1e-10: max |difference| {float((x - d8).abs().max()):.2e} of max |d| {float(x.abs().max()):.2e})")
        row("torch float64: dense H, linalg.cholesky, cholesky_solve", events(lambda: dense(graph, lin), reps=5))
    except Exception as exc:                               # (a torch build without a float64 Cholesky on this device)
        print(f"    torch dense solve unavailable: {type(exc).__name__}: {exc}")
    print("  host wall-clock around one synchronised call:")
    out, info = pgo.optimize(m, nodes, g["edges"], g["poses"], g["confs"], return_info=True)
    row(f"pgo.optimize, defaults: {len(info['f'])} trials, {sum(info['pcg_iterations'])} PCG iterations", wall(lambda: pgo.optimize(m, nodes, g["edges"], g["poses"], g["confs"])),
        f"   f {info['f'][0]:.4f} -> {info['f_new'][-1]:.6f}")
    del graph, lin
    torch.cuda.empty_cache()
