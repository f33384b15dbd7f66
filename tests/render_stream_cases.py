"""The stream-order rows of libsta_raster.so and vista_slam_amd.render, in the shape of tests/stream_cases.py (its Row, its harness): every
call is ordered by its stream alone, also behind pending work.  tests/test_render_abi.py holds the entry points named here against the
declarations of include/sta_raster.h that take a `void* stream`, in both directions; tests/test_render_stream_gpu.py runs the rows.  The
poison of a floating-point input is NaN (a dropped point, a dropped segment), of a colour 0xFF, of a key buffer 0: values the kernels
take as data, never as a fault."""
from stream_cases import Row, _up

SYNCS = {}            # no entry point of include/sta_raster.h and no drawing method of render.Canvas waits for its stream
EXEMPT = {}
H, W = 17, 33


def _camera():
    import numpy as np
    import render_cases as RC
    from vista_slam_amd import render
    c = RC.view_camera(H, W)
    return render.Camera(np.asarray(c["K"], dtype=np.float64), c["T"])


def _canvas(ssaa=1):
    from vista_slam_amd import render
    return render.Canvas("cuda:0", H, W, ssaa)


def _mk_points(seed):
    def make(m):
        import numpy as np
        import render_cases as RC
        r = np.random.default_rng(60 + seed)
        return {"pts": _up(RC.random_points(300, 70 + seed, 0.8)), "col": _up(r.integers(0, 256, (300, 3), dtype=np.uint8)), "_canvas": _canvas(),
                "_camera": _camera()}
    return make


def _run_points(m, x, between=None):
    cv = x["_canvas"]
    cv.clear().points(x["_camera"], x["pts"], x["col"], point_size=2)
    return [("keys", cv.keys.clone()), ("counters", cv._counters.clone())]


def _mk_lines(seed):
    def make(m):
        import numpy as np
        import render_cases as RC
        r = np.random.default_rng(80 + seed)
        segs = np.stack([RC.random_points(40, 90 + seed, 0.8), RC.random_points(40, 95 + seed, 0.8)], axis=1)
        return {"segs": _up(segs), "col": _up(r.integers(0, 256, (40, 3), dtype=np.uint8)), "_canvas": _canvas(2), "_camera": _camera()}
    return make


def _run_lines(m, x, between=None):
    cv = x["_canvas"]
    cv.clear().lines(x["_camera"], x["segs"], x["col"], line_width=2)
    return [("keys", cv.keys.clone())]


def _mk_resolve(seed):
    def make(m):
        import numpy as np
        import render_cases as RC
        import torch
        case, exp = RC.expected_of("ssaa_2")
        keys = exp["keys"].copy()
        if seed:
            keys = np.roll(keys, 3, axis=1)
        return {"keys": torch.from_numpy(keys.view(np.int64)).cuda(), "_canvas": _canvas(2)}
    return make


def _run_resolve(m, x, between=None):
    cv = x["_canvas"]
    cv.keys.copy_(x["keys"])
    return [("rgba", cv.image((10, 20, 30, 40))), ("depth", cv.depth()), ("ids", cv.ids())]


def _seeded(name, entries, mk, run, shapes, layer=()):
    return Row(name, entries, mk(0), run, shapes, (), mk(1), layer)


ROWS = [
    _seeded("raster_points", ("sta_raster_clear", "sta_raster_points"), _mk_points, _run_points, "Canvas.clear + Canvas.points, 300 points of size 2 on 17x33",
            layer=("render.Canvas.points",)),
    _seeded("raster_lines", ("sta_raster_clear", "sta_raster_lines"), _mk_lines, _run_lines, "Canvas.clear + Canvas.lines, 40 segments of width 2 on 17x33 at ssaa 2",
            layer=("render.Canvas.lines",)),
    _seeded("raster_resolve", ("sta_raster_resolve",), _mk_resolve, _run_resolve, "Canvas.image / depth / ids of a 17x33 canvas at ssaa 2",
            layer=("render.Canvas.image",)),
]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def named_entries():
    return {e for r in ROWS for e in r.entries}


def named_layers():
    return {e for r in ROWS for e in r.layer}


def may_wait(row):
    return [k for k in row.entries + row.layer if k in SYNCS]
