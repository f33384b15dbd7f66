"""Simplify a fused mesh on the GPU: uniform-grid vertex clustering (Rossignac-Borrel) with quadric-error placement of each cell's
vertex (Lindstrom's out-of-core form of the Garland-Heckbert quadrics).  A `tsdf.Mesh` of millions of marching-tetrahedra triangles
becomes one whose vertices are the occupied cells of a lattice of `cell_size`; a flat wall no longer costs what a chair costs.

The library is libsta_simp.so (include/sta_simp.h holds the contract, tests/simp_cases.py restates it in numpy): three stages - cells,
triangles, placement - made of the stable radix sort, ordered compactions and one lane per cell that sums, rotates (cyclic Jacobi on the
3x3 quadric) and solves in float64 in a written order.  Cells, triangles and maps are integers and the positions are defined bit for bit.

    small = simplify.simplify_mesh(mesh, 4 * voxel_size)
    small, maps = simplify.simplify_mesh(mesh, 0.2, placement="mean", return_maps=True)

What it is not: iterative edge collapse.  There is no target triangle count - `cell_size` is the control.  Nothing guarantees a manifold:
two sheets closer than a cell merge, a fan can fold onto an edge, thin features can vanish.  No boundary or colour quadrics.  Normals are
not carried as an attribute: recompute them with `tsdf.vertex_normals`.  Not compared with Open3D's simplify_vertex_clustering or MeshLab.
DESIGN.md section 9.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib, tsdf

SWEEPS = 8
INDEX_BITS = 21
PLAN_SIZES = 3
COUNTERS = ("cells", "vertices", "triangles", "dropped_vertices", "invalid_triangles", "collapsed", "duplicates", "fallbacks")
PLACEMENTS = {"mean": 0, "quadric": 1}


class Plan(NamedTuple):
    cells_work_bytes: int
    triangles_work_bytes: int
    place_work_bytes: int


class Counters(NamedTuple):
    cells: int
    vertices: int
    triangles: int
    dropped_vertices: int
    invalid_triangles: int
    collapsed: int
    duplicates: int
    fallbacks: int


class Maps(NamedTuple):
    vmap: torch.Tensor          # [nv] int32: the output vertex of every input vertex, -1 for a dropped one or one whose cell is not used
    tri_src: torch.Tensor       # [n_out] int32: the input triangle of every output triangle, ascending
    counters: Counters


class Clusters(NamedTuple):
    triangles: torch.Tensor     # [nt,3] int32, rows at and beyond counters[2] are -1
    tri_src: torch.Tensor       # [nt] int32, likewise
    cell_out: torch.Tensor      # [nv] int32
    vmap: torch.Tensor          # [nv] int32
    vcell: torch.Tensor         # [nv] int32
    counters: torch.Tensor      # [8] int64 on the device


def _check(rc):
    try:
        _lib.check_simp(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("simp_") else e) from None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def plan(nt: int, nv: int) -> Plan:
    """Host only (no GPU): the byte counts of sta_simp_plan, its refusals as ValueError."""
    out = (C.c_int64 * PLAN_SIZES)()
    _check(_lib.load_simp().sta_simp_plan(int(nt), int(nv), out))
    return Plan(*[int(v) for v in out])


def _arrays(mesh):
    verts, tris = mesh.vertices.to(torch.float32).contiguous(), mesh.triangles.to(torch.int32).contiguous()
    if verts.dim() != 2 or verts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError(f"a mesh is vertices [nv,3] and triangles [nt,3] (got {tuple(verts.shape)}, {tuple(tris.shape)})")
    return verts, tris.to(verts.device)


def _grid(cell_size, origin):
    cell = float(cell_size)
    o = (0.0, 0.0, 0.0) if origin is None else tuple(float(v) for v in origin)
    if len(o) != 3:
        raise ValueError(f"origin must have three components (got {len(o)})")
    return cell, o


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _cells(verts, cell, o, counters, p):
    dev, nv = verts.device, len(verts)
    work = torch.empty(p.cells_work_bytes, dtype=torch.uint8, device=dev)
    vcell = torch.empty(nv, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.load_simp().sta_simp_cells(_ptr(verts), nv, cell, o[0], o[1], o[2], _ptr(vcell), counters.data_ptr(), _ptr(work), work.numel(),
                                               _stream(dev)))
    return vcell


def _triangles(tris, nv, vcell, counters, p):
    dev, nt = tris.device, len(tris)
    work = torch.empty(p.triangles_work_bytes, dtype=torch.uint8, device=dev)
    tris_out = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    tri_src = torch.empty(nt, dtype=torch.int32, device=dev)
    cell_out = torch.empty(nv, dtype=torch.int32, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.load_simp().sta_simp_triangles(_ptr(tris), nt, nv, _ptr(vcell), _ptr(tris_out), _ptr(tri_src), _ptr(cell_out), _ptr(vmap),
                                                   counters.data_ptr(), _ptr(work), work.numel(), _stream(dev)))
    return tris_out, tri_src, cell_out, vmap


def cells(mesh, cell_size: float, origin=None):
    """(vcell [nv] int32, counters [8] int64) of sta_simp_cells, device tensors: per vertex the rank of its cell among the occupied cells
    in ascending (z, y, x) order, -1 for a vertex that is not finite or beyond 2^20 cells from the origin; counters[0] cells, counters[3]
    dropped vertices, the other six 0.  Does not wait for the stream."""
    verts, tris = _arrays(mesh)
    cell, o = _grid(cell_size, origin)
    counters = torch.zeros(8, dtype=torch.int64, device=verts.device)
    return _cells(verts, cell, o, counters, plan(len(tris), len(verts))), counters


def cluster_triangles(mesh, cell_size: float, origin=None) -> Clusters:
    """Stages 1 and 2 (sta_simp_cells, sta_simp_triangles): the surviving triangles in output indices, their sources, the output index of
    every cell and of every vertex, all at their worst-case sizes with the counts in the device counters.  Does not wait for the stream."""
    verts, tris = _arrays(mesh)
    cell, o = _grid(cell_size, origin)
    p = plan(len(tris), len(verts))
    counters = torch.zeros(8, dtype=torch.int64, device=verts.device)
    vcell = _cells(verts, cell, o, counters, p)
    tris_out, tri_src, cell_out, vmap = _triangles(tris, len(verts), vcell, counters, p)
    return Clusters(tris_out, tri_src, cell_out, vmap, vcell, counters)


def _colors(mesh, verts):
    if mesh.colors is None:
        return None
    cols = mesh.colors.to(torch.float32).contiguous()
    if cols.shape != verts.shape:
        raise ValueError(f"{len(verts)} vertices but colors of shape {tuple(cols.shape)}")
    return cols


def _place(verts, cols, tris, vcell, cell_out, cell, o, placement, sv_ratio, counters, p):
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be 'quadric' or 'mean' (got {placement!r})")
    dev, nv, nt = verts.device, len(verts), len(tris)
    work = torch.empty(p.place_work_bytes, dtype=torch.uint8, device=dev)
    verts_out = torch.zeros(nv, 3, dtype=torch.float32, device=dev)          # rows behind the output vertices are not written: zeros
    cols_out = torch.zeros(nv, 3, dtype=torch.float32, device=dev) if cols is not None else None
    with torch.cuda.device(dev):
        _check(_lib.load_simp().sta_simp_place(_ptr(verts), _ptr(cols) if nv else None, nv, _ptr(tris), nt, _ptr(vcell), _ptr(cell_out), cell, o[0], o[1], o[2],
                                               PLACEMENTS[placement], float(sv_ratio), _ptr(verts_out), _ptr(cols_out) if nv else None,
                                               counters.data_ptr(), _ptr(work), work.numel(), _stream(dev)))
    return verts_out, cols_out


def place_vertices(mesh, clusters: Clusters, cell_size: float, origin=None, placement: str = "quadric", sv_ratio: float = 1e-3):
    """Stage 3 (sta_simp_place) on the `Clusters` of the same mesh, cell_size and origin: (vertices [nv,3], colors [nv,3] or None) at their
    worst-case size - the rows at and beyond clusters.counters[1] are zeros - with the fallbacks in clusters.counters[7].  Does not wait
    for the stream."""
    verts, tris = _arrays(mesh)
    cell, o = _grid(cell_size, origin)
    return _place(verts, _colors(mesh, verts), tris, clusters.vcell, clusters.cell_out, cell, o, placement, sv_ratio, clusters.counters,
                  plan(len(tris), len(verts)))


def simplify_mesh(mesh, cell_size: float, *, origin=None, placement: str = "quadric", sv_ratio: float = 1e-3, return_maps: bool = False):
    """The mesh clustered on a lattice of `cell_size` (sta_simp_cells, sta_simp_triangles, sta_simp_place) as a `tsdf.Mesh`: one vertex
    per cell that a surviving triangle names, triangles with corners in fewer than three cells gone, triangles of the same three cells
    merged (the first one stays, with its winding).  placement "quadric": the vertex minimises the summed plane quadrics of the triangles
    around the cell's vertices (so a cell on a crease gets a vertex on the crease), restricted to the eigen-directions above
    sv_ratio * the largest eigenvalue, and falls back to the mean when it would leave the cell; "mean": the mean of the cell's vertices.
    Colours are the cell's means.  origin=None is (0, 0, 0): no bounds pass.  Reads the eight counters once - the one wait for the stream -
    to cut the worst-case buffers to size; return_maps adds `Maps`."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be 'quadric' or 'mean' (got {placement!r})")
    verts, tris = _arrays(mesh)
    cell, o = _grid(cell_size, origin)
    cols = _colors(mesh, verts)
    p = plan(len(tris), len(verts))
    counters = torch.zeros(8, dtype=torch.int64, device=verts.device)
    vcell = _cells(verts, cell, o, counters, p)
    tris_out, tri_src, cell_out, vmap = _triangles(tris, len(verts), vcell, counters, p)
    verts_out, cols_out = _place(verts, cols, tris, vcell, cell_out, cell, o, placement, sv_ratio, counters, p)
    c = Counters(*[int(v) for v in counters.tolist()])          # the one synchronisation
    out = tsdf.Mesh(verts_out[:c.vertices], cols_out[:c.vertices] if cols_out is not None else None, tris_out[:c.triangles])
    return (out, Maps(vmap, tri_src[:c.triangles], c)) if return_maps else out
