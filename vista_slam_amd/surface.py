"""Clean and sample a fused mesh: connected components of a `tsdf.Mesh` on the GPU (so that floaters - small blobs and shell fragments in
free space - can be dropped by size before the mesh is shown or scored) and points drawn uniformly by area from its surface (so that a
mesh can be scored samples against samples: `evaluate.eval_mesh`).

The library is libsta_surf.so (include/sta_surf.h holds the contract, tests/surf_cases.py restates it in numpy): a lock-free union-find
whose root is the component's smallest vertex index whatever the interleaving, and a stratified sampler made of a counter-based integer
generator (splitmix64) and float64 operations in a written order - labels, counts and samples are defined bit for bit by their inputs.

    mesh = surface.clean_mesh(mesh, min_triangles=100)
    s = surface.sample_surface(mesh, 200000, seed=0)

Not here: components by shared EDGE (Open3D's cluster_connected_triangles; here a shared vertex connects), component areas, point-to-triangle
distances (mesh simplification: vista_slam_amd/simplify.py).  DESIGN.md section 9.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib, tsdf

CHUNK = 1024
STATUS_BOUND = 1
PLAN_SIZES = 3


class Plan(NamedTuple):
    components_work_bytes: int
    weights_work_bytes: int
    sample_work_bytes: int       # always 0


class Samples(NamedTuple):
    points: torch.Tensor                # [n,3] f32
    triangles: torch.Tensor             # [n] int32, -1 (and NaN points) when the mesh has no area
    colors: Optional[torch.Tensor]      # [n,3] f32
    normals: Optional[torch.Tensor]     # [n,3] f32, unit face normals


def _check(rc):
    try:
        _lib.check_surf(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("surf_") else e) from None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def plan(nt: int, nv: int, ns: int = 0) -> Plan:
    """Host only (no GPU): the byte counts of sta_surf_plan, its refusals as ValueError."""
    out = (C.c_int64 * PLAN_SIZES)()
    _check(_lib.load_surf().sta_surf_plan(int(nt), int(nv), int(ns), out))
    return Plan(*[int(v) for v in out])


def _arrays(mesh):
    verts, tris = mesh.vertices.to(torch.float32).contiguous(), mesh.triangles.to(torch.int32).contiguous()
    if verts.dim() != 2 or verts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError(f"a mesh is vertices [nv,3] and triangles [nt,3] (got {tuple(verts.shape)}, {tuple(tris.shape)})")
    return verts, tris.to(verts.device)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _components(mesh):
    verts, tris = _arrays(mesh)
    dev, nv, nt = verts.device, len(verts), len(tris)
    p = plan(nt, nv)
    work = torch.empty(p.components_work_bytes, dtype=torch.uint8, device=dev)
    vlabel = torch.empty(nv, dtype=torch.int32, device=dev)
    tlabel = torch.empty(nt, dtype=torch.int32, device=dev)
    tcount = torch.empty(nv, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.load_surf().sta_surf_components(_ptr(tris), nt, nv, _ptr(vlabel), _ptr(tlabel), _ptr(tcount), status.data_ptr(), _ptr(work),
                                                    work.numel(), _stream(dev)))
    return vlabel, tlabel, tcount, status


def components(mesh, return_status: bool = False):
    """(vlabel [nv], tlabel [nt], tcount [nv]) int32 device tensors of sta_surf_components: per vertex the smallest vertex index of its
    component (-1: no triangle names it), per triangle the label of its first vertex (-1: an index outside [0, nv)), and at each
    component's smallest index its number of triangles.  Two triangles that share a vertex are connected.  The call does not wait for the
    stream; return_status adds the device status word (non-zero: a loop bound was hit and the arrays mean nothing)."""
    vlabel, tlabel, tcount, status = _components(mesh)
    return (vlabel, tlabel, tcount, status) if return_status else (vlabel, tlabel, tcount)


def clean_mesh(mesh, min_triangles: Optional[int] = None, keep_largest: Optional[int] = None) -> tsdf.Mesh:
    """The mesh without its small components: keeps the components of at least `min_triangles` triangles and, of those, the `keep_largest`
    with the most triangles (among equal counts the one with the lower smallest vertex index wins); triangles with an index outside
    [0, nv) go.  The mask is built on the device from tcount[tlabel] and handed to `tsdf.cull_mesh`.  Reads the status word (which waits
    for the stream) and raises if a loop bound was hit."""
    if min_triangles is None and keep_largest is None:
        raise ValueError("clean_mesh: give min_triangles, keep_largest or both")
    if min_triangles is not None and int(min_triangles) < 0:
        raise ValueError(f"clean_mesh: min_triangles must be >= 0 (got {min_triangles})")
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError(f"clean_mesh: keep_largest must be >= 0 (got {keep_largest})")
    _vlabel, tlabel, tcount, status = _components(mesh)
    nv = len(tcount)
    good = tcount > 0                                                # the roots
    if min_triangles is not None:
        good &= tcount >= int(min_triangles)
    if keep_largest is not None:
        # rank the roots by (count descending, index ascending): one int64 key per vertex, larger is better
        key = torch.where(good, tcount.to(torch.int64) * (1 << 31) + (nv - 1 - torch.arange(nv, device=tcount.device)), -1)
        k = min(int(keep_largest), nv)
        best = torch.topk(key, k).indices if k else key[:0]
        top = torch.zeros(nv, dtype=torch.bool, device=tcount.device)
        top[best] = True
        good &= top
    valid = tlabel >= 0
    keep = valid & good[tlabel.clamp(min=0).to(torch.int64)] if nv else valid
    if int(status.item()) != 0:
        raise RuntimeError(f"sta_surf_components reached a loop bound (status {int(status.item())}): the labels are not defined")
    return tsdf.cull_mesh(mesh, keep)


def _weights(verts, tris, tri_keep):
    dev, nv, nt = verts.device, len(verts), len(tris)
    if tri_keep is not None:
        tri_keep = torch.as_tensor(tri_keep, device=dev).to(torch.bool).to(torch.uint8).contiguous()
        if tri_keep.shape != (nt,):
            raise ValueError(f"tri_keep must be [{nt}] (got {tuple(tri_keep.shape)})")
    p = plan(nt, nv)
    work = torch.empty(p.weights_work_bytes, dtype=torch.uint8, device=dev)
    P = torch.empty(nt, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.load_surf().sta_surf_weights(_ptr(verts), nv, _ptr(tris), nt, _ptr(tri_keep), _ptr(P), total.data_ptr(), _ptr(work), work.numel(),
                                                 _stream(dev)))
    return P, total


def weights(mesh, tri_keep=None):
    """(P [nt] float64, total [1] float64) of sta_surf_weights: the inclusive prefix, in the header's order, of twice the triangle areas
    (0 for a triangle that is not valid, not kept or not finite).  Does not wait for the stream."""
    verts, tris = _arrays(mesh)
    return _weights(verts, tris, tri_keep)


def area(mesh, tri_keep=None) -> torch.Tensor:
    """The surface area as a 0-d float64 device tensor: total / 2 of `weights` (exact: a halving).  Does not wait for the stream."""
    return weights(mesh, tri_keep)[1][0] * 0.5


def sample_surface(mesh, n: int, seed: int = 0, tri_keep=None, colors: bool = False, normals: bool = False) -> Samples:
    """n points uniformly by area from the surface (sta_surf_weights + sta_surf_sample): stratified over the cumulative area, so triangle
    t gets within 2 of n * area_t / area samples; `seed` is any integer (taken modulo 2^64).  colors: the vertex colours interpolated;
    normals: the unit face normals.  A mesh without area gives triangles of -1 and NaN points.  Does not wait for the stream."""
    verts, tris = _arrays(mesh)
    dev, nv, nt, n = verts.device, len(verts), len(tris), int(n)
    plan(nt, nv, n)
    cols = None
    if colors:
        if mesh.colors is None:
            raise ValueError("sample_surface: colors=True but the mesh has none")
        cols = mesh.colors.to(torch.float32).contiguous()
        if cols.shape != verts.shape:
            raise ValueError(f"{nv} vertices but colors of shape {tuple(cols.shape)}")
    P, total = _weights(verts, tris, tri_keep)
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    cout = torch.empty(n, 3, dtype=torch.float32, device=dev) if colors else None
    nout = torch.empty(n, 3, dtype=torch.float32, device=dev) if normals else None
    with torch.cuda.device(dev):
        _check(_lib.load_surf().sta_surf_sample(_ptr(verts), nv, _ptr(tris), nt, _ptr(P), total.data_ptr(), _ptr(cols) if colors else None, n,
                                                int(seed) % (1 << 64), _ptr(points), _ptr(tri), _ptr(cout), _ptr(nout), _stream(dev)))
    return Samples(points, tri, cout, nout)
