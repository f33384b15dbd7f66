"""Fuse the map into a surface: a sparse truncated signed distance volume integrated from the keyframes' depth maps on the GPU, and its
zero level set as a triangle mesh by marching tetrahedra.

The library is libsta_tsdf.so (include/sta_tsdf.h holds the contract, tests/tsdf_cases.py restates it in numpy): blocks of 8^3 lattice
points under sorted 63-bit keys (no hash table), float64 arithmetic in a written order, views folded in ascending order per lattice
point, no floating-point atomics - a volume and a mesh are defined bit for bit by their inputs.  The inputs are exactly what
`PoseGraph.export` / `formats.world_pointcloud` take.

    mesh = tsdf.mesh_from_slam(slam, voxel_size=0.05)
    tsdf.write_mesh_ply("mesh.ply", mesh)

Not here: growing a volume's block set after `allocate` (poses move under the optimiser, so fusion is a pass over an export, as
`world_pointcloud` is); trilinear depth lookup (the nearest pixel is used); ray casting; marching cubes;
Open3D's ScalableTSDFVolume bit for bit - this is a contract of its own.  DESIGN.md section 9.

On top of a mesh, through libsta_mesh.so (include/sta_mesh.h): `vertex_normals` (area-weighted, summed in ascending triangle order, no
floating-point atomics), `write_mesh_ply(normals=)`, `visible_triangles` (the triangles whose id survives in a camera's id image) and
`cull_mesh`.  `render.Canvas.mesh` draws a Mesh.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

BLOCK = 8
BLOCK_POINTS = 512
MAX_TRUNC_VOXELS = 4
MAX_BLOCKS = 1 << 24
MAX_PIXELS = 1 << 28
PLAN_SIZES = 8
FIRST_MAX_BLOCKS = 1 << 16        # the capacity `allocate` tries first; a scene of more blocks costs a second sta_tsdf_blocks call


class Plan(NamedTuple):
    blocks_work_bytes: int
    keys_bytes: int
    tsdf_bytes: int          # = weight
    rgb_bytes: int
    mesh_work_bytes: int
    verts_bytes: int         # = cols
    tris_bytes: int
    key_slots: int


class Views(NamedTuple):
    """The per-view tables of include/sta_tsdf.h on the device."""
    depths: torch.Tensor     # [V,H,W] f32
    scales: torch.Tensor     # [V] f32
    K: torch.Tensor          # [V,4] f64: fx, fy, cx, cy
    c2w: torch.Tensor        # [V,12] f64
    w2c: torch.Tensor        # [V,12] f64
    obs: torch.Tensor        # [V,H,W] f32
    imgs: Optional[torch.Tensor]      # [V,3,H,W] f32 in [-1,1]


class Mesh(NamedTuple):
    vertices: torch.Tensor            # [nv,3] f32
    colors: Optional[torch.Tensor]    # [nv,3] f32 in [0,1]
    triangles: torch.Tensor           # [nt,3] int32, normals into free space


def _value_error(e: _lib.StaError):
    return ValueError(str(e)) if str(e).startswith("tsdf_") else e


def _check(rc):
    try:
        _lib.check_tsdf(rc)
    except _lib.StaError as e:
        raise _value_error(e) from None


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _origin(origin):
    if origin is None:
        return None
    o = (C.c_double * 3)(*[float(v) for v in origin])
    if not all(np.isfinite(v) for v in o):
        raise ValueError("origin must be finite")
    return o


def plan(V: int, H: int, W: int, voxel_size: float, trunc: Optional[float] = None, max_blocks: int = 1, max_vertices: int = 0,
         max_triangles: int = 0) -> Plan:
    """Host only (no GPU): the byte counts of sta_tsdf_plan, its refusals as ValueError."""
    vs = float(voxel_size)
    out = (C.c_int64 * PLAN_SIZES)()
    _check(_lib.load_tsdf().sta_tsdf_plan(int(V), int(H), int(W), vs, 3.0 * vs if trunc is None else float(trunc), int(max_blocks), int(max_vertices),
                                          int(max_triangles), out))
    return Plan(*[int(v) for v in out])


def case_table() -> np.ndarray:
    """Host only: the library's [6,16,7] int8 tetrahedron case table (sta_tsdf_table)."""
    buf = (C.c_int8 * (6 * 16 * 7))()
    _check(_lib.load_tsdf().sta_tsdf_table(buf))
    return np.frombuffer(buf, dtype=np.int8).reshape(6, 16, 7).copy()


def views(depths, scales, intrinsics, poses, confs, imgs=None, *, conf_thres: float, counts=None, min_views: int = 0, device="cuda:0") -> Views:
    """The tables of a fusion from exactly what `PoseGraph.export` / `formats.world_pointcloud` take: depths / confs [N,H,W], scales [N] or
    [N,1], intrinsics [N,3,3], poses [N,4,4] camera-to-world, imgs [N,3,H,W] in [-1,1] or None.  obs = 1.0 where conf > conf_thres (and
    counts >= min_views when counts is given and min_views > 0), else 0.  c2w is the float32 pose widened; w2c = [R^T | -R^T t] in host
    float64 from it.  A K with skew, or a last row other than (0, 0, 1), is refused."""
    dev = torch.device(device)
    depths = torch.as_tensor(depths).to(dev, torch.float32).contiguous()
    if depths.dim() != 3:
        raise ValueError(f"depths must be [N, H, W] (got {tuple(depths.shape)})")
    N, H, W = depths.shape
    scales = torch.as_tensor(scales).to(dev, torch.float32).reshape(N).contiguous()
    Km = torch.as_tensor(intrinsics).detach().cpu().to(torch.float32).reshape(N, 3, 3).numpy().astype(np.float64)
    if np.any(Km[:, 0, 1] != 0) or np.any(Km[:, 1, 0] != 0) or np.any(Km[:, 2] != np.array([0.0, 0.0, 1.0])):
        raise ValueError("intrinsics must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew or another last row is not supported")
    P = torch.as_tensor(poses).detach().cpu().to(torch.float32).reshape(N, 4, 4).numpy().astype(np.float64)
    R, t = P[:, :3, :3], P[:, :3, 3]
    Rt = np.transpose(R, (0, 2, 1))
    w2c = np.concatenate([Rt, -(Rt @ t[:, :, None])], axis=2).reshape(N, 12)
    confs = torch.as_tensor(confs).to(dev, torch.float32)
    if tuple(confs.shape) != (N, H, W):
        raise ValueError(f"confs must be {(N, H, W)} (got {tuple(confs.shape)})")
    keep = confs > float(conf_thres)
    if counts is not None and min_views > 0:
        counts = torch.as_tensor(counts).to(dev)
        if tuple(counts.shape) != (N, H, W):
            raise ValueError(f"counts must be {(N, H, W)} (got {tuple(counts.shape)})")
        keep = keep & (counts >= min_views)
    if imgs is not None:
        imgs = torch.as_tensor(imgs).to(dev, torch.float32).contiguous()
        if tuple(imgs.shape) != (N, 3, H, W):
            raise ValueError(f"imgs must be {(N, 3, H, W)} (got {tuple(imgs.shape)})")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    return Views(depths, scales, up(np.stack([Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2]], axis=1)), up(P[:, :3, :].reshape(N, 12)), up(w2c),
                 keep.to(torch.float32).contiguous(), imgs)


class TSDFVolume:
    """A sparse TSDF volume on one device.  `allocate(views)` finds the blocks the views touch and clears them; `integrate(views)` folds
    views in (in ascending order; successive ranges give the bits of one call); `mesh()` extracts the surface.  The tensors keys [nb]
    int64 (the bits of the uint64 keys), tsdf / weight [nb,512] float32 and rgb [nb,512,3] float32 (None for a volume without colour)
    are the library's layout.  allocate and mesh wait for the stream once each (their counts come back); integrate does not."""

    def __init__(self, device="cuda:0", voxel_size: float = 0.05, trunc: Optional[float] = None, origin=None, max_weight: float = 64.0,
                 depth_max: float = float("inf")):
        self.device = torch.device(device)
        self.voxel_size = float(voxel_size)
        self.trunc = 3.0 * self.voxel_size if trunc is None else float(trunc)
        self.origin = None if origin is None else tuple(float(v) for v in origin)
        self.max_weight, self.depth_max = float(max_weight), float(depth_max)
        plan(1, 1, 1, self.voxel_size, self.trunc)                # the refusals of a bad voxel_size / trunc
        self._o = _origin(self.origin)
        self.lib = _lib.load_tsdf()
        self.keys = self.tsdf = self.weight = self.rgb = None
        self.n_observed = self.n_dropped = 0

    @property
    def n_blocks(self) -> int:
        return 0 if self.keys is None else int(self.keys.shape[0])

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.keys, self.tsdf, self.weight, self.rgb) if t is not None)

    def _blocks(self, v: Views, max_blocks: int):
        V, H, W = v.depths.shape
        p = plan(V, H, W, self.voxel_size, self.trunc, max_blocks)
        keys = torch.empty(max_blocks, dtype=torch.int64, device=self.device)
        work = torch.empty(p.blocks_work_bytes, dtype=torch.uint8, device=self.device)
        cnt = (C.c_int64 * 3)()
        rc = self.lib.sta_tsdf_blocks(v.depths.data_ptr(), v.scales.data_ptr(), v.K.data_ptr(), v.c2w.data_ptr(), v.obs.data_ptr(), V, H, W, self.voxel_size,
                                      self.trunc, self._o, self.depth_max, keys.data_ptr(), max_blocks, work.data_ptr(), work.numel(), cnt, _stream(self.device))
        return rc, keys, [int(c) for c in cnt]

    def allocate(self, v: Views, colour: Optional[bool] = None, max_blocks: Optional[int] = None) -> "TSDFVolume":
        """The block set of the views (sta_tsdf_blocks), cleared (sta_tsdf_clear).  colour None: a colour volume iff the views have images."""
        V, H, W = v.depths.shape
        first = min(8 * V * H * W, FIRST_MAX_BLOCKS) if max_blocks is None else int(max_blocks)
        rc, keys, cnt = self._blocks(v, first)
        if rc != 0 and max_blocks is None and first < cnt[0] < MAX_BLOCKS:
            rc, keys, cnt = self._blocks(v, cnt[0])
        _check(rc)
        nb, self.n_observed, self.n_dropped = cnt
        self.keys = keys[:nb].clone()
        self.tsdf = torch.empty(nb, 512, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(nb, 512, dtype=torch.float32, device=self.device)
        self.rgb = torch.empty(nb, 512, 3, dtype=torch.float32, device=self.device) if (v.imgs is not None if colour is None else colour) else None
        return self.clear()

    def clear(self) -> "TSDFVolume":
        _check(self.lib.sta_tsdf_clear(self.tsdf.data_ptr(), self.weight.data_ptr(), self.rgb.data_ptr() if self.rgb is not None else None, self.n_blocks,
                                       _stream(self.device)))
        return self

    def integrate(self, v: Views, start: int = 0, stop: Optional[int] = None) -> "TSDFVolume":
        """Folds the views [start, stop) in (sta_tsdf_integrate); does not wait."""
        if self.keys is None:
            raise ValueError("integrate: allocate the volume first")
        V, H, W = v.depths.shape
        stop = V if stop is None else int(stop)
        _check(self.lib.sta_tsdf_integrate(self.keys.data_ptr(), self.n_blocks, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                           self.rgb.data_ptr() if self.rgb is not None else None, v.depths.data_ptr(), v.scales.data_ptr(), v.K.data_ptr(),
                                           v.w2c.data_ptr(), v.obs.data_ptr(), v.imgs.data_ptr() if v.imgs is not None else None, V, H, W, int(start), stop,
                                           self.voxel_size, self.trunc, self._o, self.depth_max, self.max_weight, _stream(self.device)))
        return self

    def mesh(self, min_weight: float = 1.0) -> Mesh:
        """The zero level set among the lattice points of weight >= min_weight (sta_tsdf_mesh): a counting call, then one into buffers of
        exactly that size."""
        if self.keys is None:
            raise ValueError("mesh: allocate the volume first")
        nb, dev = self.n_blocks, self.device
        empty = Mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev) if self.rgb is not None else None,
                     torch.zeros(0, 3, dtype=torch.int32, device=dev))
        if nb == 0:
            return empty
        p = plan(1, 1, 1, self.voxel_size, self.trunc, nb)
        work = torch.empty(p.mesh_work_bytes, dtype=torch.uint8, device=dev)
        cnt = (C.c_int64 * 2)()
        rgb = self.rgb.data_ptr() if self.rgb is not None else None

        def call(verts, cols, tris, nv, nt):
            _check(self.lib.sta_tsdf_mesh(self.keys.data_ptr(), nb, self.tsdf.data_ptr(), self.weight.data_ptr(), rgb, self.voxel_size, self._o,
                                          float(min_weight), verts, cols, tris, nv, nt, work.data_ptr(), work.numel(), cnt, _stream(dev)))
        call(None, None, None, 0, 0)
        nv, nt = int(cnt[0]), int(cnt[1])
        if nv == 0:
            return empty
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=dev) if self.rgb is not None else None
        tris = torch.empty(nt, 3, dtype=torch.int32, device=dev)
        call(verts.data_ptr(), cols.data_ptr() if cols is not None else None, tris.data_ptr(), nv, nt)
        return Mesh(verts, cols, tris)


def fuse(frontend_or_device, *, depths, scales, intrinsics, poses, confs, imgs=None, conf_thres: float, counts=None, min_views: int = 0,
         voxel_size: float, trunc: Optional[float] = None, origin=None, max_weight: float = 64.0, depth_max: float = float("inf"),
         min_weight: float = 1.0, return_volume: bool = False):
    """views -> allocate -> integrate -> mesh of exactly the arguments `PoseGraph.export` returns (plus the images).  -> Mesh (and the
    volume with return_volume)."""
    dev = getattr(frontend_or_device, "device", frontend_or_device)
    v = views(depths, scales, intrinsics, poses, confs, imgs, conf_thres=conf_thres, counts=counts, min_views=min_views, device=dev)
    vol = TSDFVolume(dev, voxel_size, trunc, origin, max_weight, depth_max).allocate(v).integrate(v)
    m = vol.mesh(min_weight)
    return (m, vol) if return_volume else m


def mesh_from_slam(slam, voxel_size: float, **kw) -> Mesh:
    """The surface of a live OnlineSLAM: `fuse` of its `PoseGraph.export`."""
    n = slam.view_num
    ex = slam.pose_graph.export(view_num=n)
    return fuse(slam.frontend, depths=ex.depths, scales=ex.scales, intrinsics=ex.intrinsics, poses=ex.poses, confs=ex.confs,
                imgs=torch.stack(slam.imgs[:n], dim=0), conf_thres=slam.conf_thres, voxel_size=voxel_size, **kw)


def mesh_from_folder(folder: str, voxel_size: float, device="cuda:0", **kw) -> Mesh:
    """The surface of a `save_data_all` folder (read with `evaluate.load_data`; images.npy gives the colours when it is there)."""
    import os
    from . import evaluate
    d = evaluate.load_data(folder, load_view_graph=False, load_gt_depths=False, load_gt_poses=False, load_gt_intrinsic=False)
    imgs = None
    if os.path.exists(os.path.join(folder, "images.npy")):
        imgs = torch.from_numpy(np.load(os.path.join(folder, "images.npy"))).permute(0, 3, 1, 2) * 2.0 - 1.0
    N = d.unscaled_depths.shape[0]
    return fuse(device, depths=d.unscaled_depths, scales=np.asarray(d.scales).reshape(N), intrinsics=d.intrinsics, poses=d.poses, confs=d.confs, imgs=imgs,
                conf_thres=d.conf_thres, voxel_size=voxel_size, **kw)


# ------------------------------------------------------------------------------------------ files
def _ply_header(nv: int, nt: int, normals: bool = False) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\ncomment Created by vista_slam_amd (Open3D layout)\n"
            f"element vertex {nv}\nproperty double x\nproperty double y\nproperty double z\n"
            + ("property double nx\nproperty double ny\nproperty double nz\n" if normals else "") +
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {nt}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


FACE_RECORD = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
assert FACE_RECORD.itemsize == 13
# a vertex with normals, in Open3D's order: coordinates, normals, colours
PLY_NORMAL_RECORD = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8"), ("red", "u1"), ("green", "u1"),
                              ("blue", "u1")])
assert PLY_NORMAL_RECORD.itemsize == 51


def write_mesh_ply(path: str, mesh: Mesh, normals=None):
    """Binary little-endian PLY: `formats.PLY_RECORD` vertices (double coordinates, uchar colours = rint(clamp(c, 0, 1) * 255); white
    without colours), then `property list uchar int vertex_indices` faces.  normals [nv,3] (`vertex_normals`): `property double nx, ny,
    nz` between the coordinates and the colours (PLY_NORMAL_RECORD); without them the file is what it always was."""
    from .formats import PLY_RECORD
    v = mesh.vertices.detach().cpu().numpy()
    rec = np.zeros(len(v), dtype=PLY_RECORD if normals is None else PLY_NORMAL_RECORD)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = normals.detach().cpu().numpy() if isinstance(normals, torch.Tensor) else np.asarray(normals)
        if n.shape != v.shape:
            raise ValueError(f"{len(v)} vertices but normals of shape {n.shape}")
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if mesh.colors is not None:
        c = np.rint(np.clip(np.nan_to_num(mesh.colors.detach().cpu().numpy(), nan=0.0), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    else:
        c = np.full((len(v), 3), 255, np.uint8)
    rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    t = mesh.triangles.detach().cpu().numpy()
    faces = np.zeros(len(t), dtype=FACE_RECORD)
    faces["n"], faces["v"] = 3, t
    with open(path, "wb") as f:
        f.write(_ply_header(len(v), len(t), normals is not None))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_mesh_ply(path: str):
    """-> (vertex records [nv] formats.PLY_RECORD - PLY_NORMAL_RECORD, with nx, ny, nz, when the file has normals -, triangles [nt,3]
    int32) of a file of `write_mesh_ply`"""
    from .formats import PLY_RECORD
    dtype = PLY_RECORD
    with open(path, "rb") as f:
        nv = nt = None
        while True:
            line = f.readline().decode("ascii").strip()
            if line == "property double nx":
                dtype = PLY_NORMAL_RECORD
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            if line.startswith("element face"):
                nt = int(line.split()[-1])
            if line == "end_header":
                break
        rec = np.frombuffer(f.read(nv * dtype.itemsize), dtype=dtype)
        faces = np.frombuffer(f.read(nt * FACE_RECORD.itemsize), dtype=FACE_RECORD)
    assert (faces["n"] == 3).all()
    return rec, faces["v"].astype(np.int32)


def mesh_from_ply(path: str, device="cuda:0") -> Mesh:
    """A file of `write_mesh_ply` as a Mesh on the device (coordinates rounded to float32, colours byte / 255)."""
    rec, tris = read_mesh_ply(path)
    v = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    c = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.float32) / np.float32(255.0)
    return Mesh(torch.from_numpy(v).to(device), torch.from_numpy(c).to(device), torch.from_numpy(np.ascontiguousarray(tris)).to(device))


# ------------------------------------------------------------------------------------------ on top of a mesh: libsta_mesh.so
def _check_mesh(rc):
    try:
        _lib.check_mesh(rc)
    except _lib.StaError as e:
        raise (ValueError(str(e)) if str(e).startswith("mesh_") else e) from None


def vertex_normals(mesh: Mesh) -> torch.Tensor:
    """[nv,3] float32: per vertex the sum of the un-normalised face normals of its triangles (so each face weighs by its area), in
    ascending triangle index in float64, normalised; (0, 0, 0) for a vertex of no triangle or of a zero sum (sta_mesh_vertex_normals).
    The call does not wait for the stream; its workspace is allocated here."""
    lib = _lib.load_mesh()
    verts, tris = mesh.vertices.to(torch.float32).contiguous(), mesh.triangles.to(torch.int32).contiguous()
    dev = verts.device
    nv, nt = len(verts), len(tris)
    sizes = (C.c_int64 * 2)()
    _check_mesh(lib.sta_mesh_plan(nt, nv, sizes))
    if sizes[1] < 0:
        raise ValueError(f"mesh_vertex_normals: 3 * nt must be below 2^31 (got nt = {nt})")
    work = torch.empty(int(sizes[1]), dtype=torch.uint8, device=dev)
    out = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    _check_mesh(lib.sta_mesh_vertex_normals(verts.data_ptr(), nv, tris.data_ptr(), nt, out.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return out


def visible_triangles(frontend, mesh: Mesh, cameras, H: int, W: int, ssaa: int = 1) -> torch.Tensor:
    """bool [nt]: the triangles whose id survives in the id image (`Canvas.ids`) of at least one of `cameras` (render.Camera) - the
    nearest surface at some pixel.  The triangle pass does the work; the union is torch plumbing."""
    from . import render
    dev = getattr(frontend, "device", frontend)
    nt = len(mesh.triangles)
    seen = torch.zeros(nt + 1, dtype=torch.bool, device=dev)          # the last slot takes the empty pixels
    cv = render.Canvas(dev, H, W, ssaa)
    for cam in cameras:
        cv.clear().mesh(cam, mesh, mode="id")
        ids = (cv.ids().reshape(-1).to(torch.int64) & 0xFFFFFFFF).clamp_(max=nt)      # an empty pixel's id is 2^32 - 1
        seen[ids] = True
    return seen[:nt]


def cull_mesh(mesh: Mesh, keep) -> Mesh:
    """The triangles of `keep` (bool [nt]) and the vertices they name, re-indexed in ascending order; the other vertices are dropped."""
    keep = torch.as_tensor(keep, dtype=torch.bool, device=mesh.triangles.device)
    tris = mesh.triangles[keep].to(torch.int64)
    used = torch.zeros(len(mesh.vertices), dtype=torch.bool, device=tris.device)
    used[tris.reshape(-1)] = True
    new = torch.cumsum(used.to(torch.int64), 0) - 1
    return Mesh(mesh.vertices[used], mesh.colors[used] if mesh.colors is not None else None, new[tris].to(torch.int32))
