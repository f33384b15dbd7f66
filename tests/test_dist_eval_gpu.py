"""GPU: evaluate.eval_mesh(mode="surface") - the samples of the default mode scored against the other MESH with the exact point-to-triangle
distances of vista_slam_amd/meshdist.py - against tests/dist_cases.py.  Counts and ratios are compared exactly; the float64 means are
torch device sums in another order and are compared at 1e-12 relative, as tests/test_surf_gpu.py does for the default mode."""
import numpy as np
import pytest

import cloud_cases as CC
import dist_cases as D
import surf_cases as SF

pytestmark = pytest.mark.gpu
N = 600


def _mesh_of(v, t, col=None):
    import torch
    from vista_slam_amd import tsdf
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    return tsdf.Mesh(up(v), up(col), up(t))


def _clipped(verts, tris, points, max_error):
    return np.sqrt(np.minimum(D.brute(D.Index(verts, tris), points, max_error)[0], float(max_error) * float(max_error)))


def _score(d_est, d_gt, threshold):
    acc, comp = float(d_est.sum() / len(d_est)), float(d_gt.sum() / len(d_gt))
    n_precise, n_complete = int((d_est <= threshold).sum()), int((d_gt <= threshold).sum())
    p, r = n_precise / len(d_est), n_complete / len(d_gt)
    return {"accuracy": acc, "completion": comp, "completion_ratio": r, "precision": p, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0,
            "chamfer": (acc + comp) / 2.0, "n_precise": n_precise, "n_complete": n_complete}


def _assert_score(got, want):
    assert (got.n_precise, got.n_complete) == (want["n_precise"], want["n_complete"])
    assert got.precision == want["precision"] and got.completion_ratio == want["completion_ratio"] and got.fscore == want["fscore"]
    for k in ("accuracy", "completion", "chamfer"):
        assert abs(getattr(got, k) - want[k]) <= 1e-12 * want[k], (k, getattr(got, k), want[k])


def test_a_mesh_against_itself_scores_the_float32_step_not_the_sample_spacing():
    import torch
    from vista_slam_amd import evaluate
    v, t, col = SF.sphere()
    mesh = _mesh_of(v, t, col)
    surf = evaluate.eval_mesh("cuda:0", mesh, mesh, n_samples=N, threshold=0.05, max_error=0.5, seed=3, mode="surface")
    dflt = evaluate.eval_mesh("cuda:0", mesh, mesh, n_samples=N, threshold=0.05, max_error=0.5, seed=3)
    assert torch.equal(surf.est_points, dflt.est_points) and torch.equal(surf.gt_points, dflt.gt_points)
    # A sample is float(p) of a point p of its triangle: per axis at most half a float32 step of the largest coordinate away from it, so at
    # most sqrt(3) / 2 < 1 steps from the surface (the float64 rounding of p itself is 2^-29 of that).  The bound asserted is ONE step.
    step = float(np.spacing(np.float32(np.abs(v).max())))
    print(f"[dist eval] self score, {N} samples: surface accuracy {surf.accuracy:.3e} completion {surf.completion:.3e} (float32 step {step:.3e}); "
          f"samples accuracy {dflt.accuracy:.4f} completion {dflt.completion:.4f}")
    assert 0.0 <= surf.accuracy <= step and 0.0 <= surf.completion <= step
    assert surf.precision == 1.0 and surf.completion_ratio == 1.0 and surf.fscore == 1.0 and surf.n_precise == N
    # the default mode reports the spacing of the samples: the mean nearest-neighbour distance of n uniform points on an area A is about
    # 0.5 sqrt(A / n); half of that is asserted
    area = float(SF.prefix(SF.tri_weights(v, t))[1] * 0.5)
    spacing = 0.5 * np.sqrt(area / N)
    assert dflt.accuracy >= 0.5 * spacing and dflt.completion >= 0.5 * spacing, (dflt.accuracy, dflt.completion, spacing)
    assert dflt.accuracy > 1e4 * step


def test_a_dyadic_offset_shifts_the_score_as_the_restatement_computes_it():
    from vista_slam_amd import evaluate
    v, t, col = SF.sphere()
    d = np.array([0.0625, 0.0, 0.0], dtype=np.float32)
    ve = v + d
    est = SF.sample(ve, t, N, seed=3)["points"]
    gt = SF.sample(v, t, N, seed=4)["points"]
    for T in (None, np.concatenate([np.eye(3), np.array([[-0.03125], [0.0], [0.0]])], axis=1)):
        e = est if T is None else CC.transform(est, T)
        vt = ve if T is None else CC.transform(ve, T)
        want = _score(_clipped(v, t, e, 0.5), _clipped(vt, t, gt, 0.5), 0.05)
        got = evaluate.eval_mesh("cuda:0", _mesh_of(ve, t, col), _mesh_of(v, t), n_samples=N, threshold=0.05, max_error=0.5, T=T, seed=3, mode="surface")
        assert np.array_equal(got.est_points.cpu().numpy(), e) and np.array_equal(got.gt_points.cpu().numpy(), gt)
        _assert_score(got, want)
        shift = 0.0625 if T is None else 0.03125
        assert 0.3 * shift < got.accuracy <= shift and 0.3 * shift < got.completion <= shift + 1e-6
        print(f"[dist eval] offset {shift}: accuracy {got.accuracy:.5f} completion {got.completion:.5f} fscore {got.fscore:.4f}")
    with pytest.raises(ValueError, match="mode must be"):
        evaluate.eval_mesh("cuda:0", _mesh_of(v, t), _mesh_of(v, t), mode="mesh")


def test_a_cloud_as_ground_truth_scores_completion_against_the_estimates_mesh():
    from vista_slam_amd import evaluate
    v, t, _col = SF.sphere()
    d = np.array([0.0, 0.03125, 0.0], dtype=np.float32)
    gt = SF.sample(v, t, N, seed=9)["points"]
    est = SF.sample(v + d, t, N, seed=5)["points"]
    got = evaluate.eval_mesh("cuda:0", _mesh_of(v + d, t), gt, n_samples=N, threshold=0.05, max_error=0.5, seed=5, mode="surface")
    dflt = evaluate.eval_mesh("cuda:0", _mesh_of(v + d, t), gt, n_samples=N, threshold=0.05, max_error=0.5, seed=5)
    assert np.array_equal(got.gt_points.cpu().numpy(), gt) and np.array_equal(got.est_points.cpu().numpy(), est)
    assert (got.accuracy, got.precision, got.n_precise) == (dflt.accuracy, dflt.precision, dflt.n_precise), "accuracy stays cloud against cloud"
    d_est = SF.eval_points(est, gt, threshold=0.05, max_error=0.5)["d_est"]
    _assert_score(got, _score(d_est, _clipped(v + d, t, gt, 0.5), 0.05))
    assert got.completion <= 0.03125 < dflt.completion
