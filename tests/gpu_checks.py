"""GPU parity checks, shared by the pytest suite (tests/test_gpu_*.py) and the diagnostic runner
(tests/gpu_diag.py).  Every check calls the HIP product kernels through the C ABI and compares
with a plain fp32 torch/numpy reference of the same op (or with reference-derived goldens) and
returns {metric_name: error}.  Nothing here runs the product on a CPU fallback: there is none."""
import ctypes as C

import numpy as np
import torch

import helpers as HP
from helpers import load_golden, rel_l2, max_rel, rope2d_ref, grid_pos
from range_cases import range_class
from vista_slam_amd import _lib
from vista_slam_amd import weights as W
from vista_slam_amd.sta_frontend import STAFrontend, rope2d_inplace

DEV = "cuda:0"
_models = {}
_hooks_lib = None        # on_library: the ONE library behind every model() / kernel_handle (None: the product / the test-hooks library)
last_range = (0, 0)      # (fp16 saturations, fp8 correction-byte saturations) counted during the last run_golden_case (sta_range_report)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def st():
    return torch.cuda.current_stream().cuda_stream


def model(cfg_name="tiny", qk_gain=1.0, precision="f16x3", seed=43, outlier=0, hooks=False):
    """Cached frontends (weights are procedural, so (cfg, gain, seed, outlier level) identifies them).  hooks=False: the PRODUCT
    library libsta_mi355.so (what every golden / parity test runs); hooks=True: the test-hooks build libsta_mi355_test.so (same
    translation unit + the kernel-level entry points and experiment switches of include/sta_mi355_debug.h)."""
    lib = _hooks_lib if _hooks_lib is not None else (_lib.load_test() if hooks else None)
    key = (cfg_name, qk_gain, seed, outlier, bool(hooks)) + ((id(lib),) if _hooks_lib is not None else ())
    if key not in _models:
        cfg = W.TINY if cfg_name == "tiny" else W.FULL
        m = STAFrontend(cfg, DEV, precision=precision, lib=lib)
        m.load_procedural(seed=seed, qk_gain=qk_gain, outlier=outlier)
        _models[key] = m
    m = _models[key]
    m.set_precision(precision)
    return m


class on_library:
    """`with on_library(_lib.load_skew()):` - every frontend that model() / kernel_handle hand out inside the block is one on `lib`, a
    build that exports the product ABI and the test hooks; what the checks compute and return is unchanged."""
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        global _hooks_lib
        self.prev, _hooks_lib = _hooks_lib, self.lib
        return self.lib

    def __exit__(self, *exc):
        global _hooks_lib
        _hooks_lib = self.prev


def drop_models():
    _models.clear()
    torch.cuda.empty_cache()


def kernel_handle(precision, variant=0):
    """precision "head_mx": the DPT head's arithmetic of the default policy (f16 main product + one block-scaled fp8 correction
    MFMA on f16mx rows) in the kernels that have it: the debug GEMM (plane epilogue), conv3x3, ConvT, bilinear."""
    # "mlp_mx": the MLP's f16mx path of precision f16x3m - mlp.fc1's GELU epilogue writing f16mx rows (via_f16 + GELU) and mlp.fc2
    # (fp32 / in-place-residual epilogues on f16mx rows and weights)
    m = model("tiny", 1.0, {"head_mx": "f16x3h", "mlp_mx": "f16x3m"}.get(precision, precision), hooks=True)
    _lib.check(m.lib.sta_set_gemm_variant(m._h, variant))
    _lib.check(m.lib.sta_debug_set_option(m._h, 4, {"head_mx": 1, "mlp_mx": 2}.get(precision, 0)))
    return m, m.lib, m._h


def has_hooks(m):
    return hasattr(m.lib, "sta_set_gemm_variant")


def set_variant(m, variant):
    """Force a GEMM tile family (test-hooks build only).  On a product-library frontend only `0` (= what it always does) is legal."""
    if not has_hooks(m):
        assert variant == 0, "forced tile families need a frontend on the test-hooks library (model(..., hooks=True))"
        return
    _lib.check(m.lib.sta_set_gemm_variant(m._h, variant))


# ------------------------------------------------------------------------------------------ kernels
def last_plan(lib, h):
    """The plan (sta_launch.inc: gemm_plan) of the handle's last GEMM launch: family, tile, row tail, tiles, K slices."""
    out = (C.c_int * 8)()
    _lib.check(lib.sta_debug_last_gemm_plan(h, out))
    return dict(zip(("family", "bm", "bn", "m_tail", "tiles_m", "tiles_n", "ksplit", "slab_ks"), out))


def check_gemm(precision, M=300, N=200, K=96, act=0, via_f16=0, resid=False, seed=0, variant=0, tail_rows=0):
    """tail_rows: also report the error of the last tail_rows rows alone (a wrong pose-token row among thousands of rows moves
    the whole-matrix error by less than any bar) and the plan the GEMM ran under."""
    m, lib, h = kernel_handle(precision, variant)
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * 1.3
    Wt = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if resid else None
    ref = A.double() @ Wt.double().T + b.double()
    if act == 1:
        ref = torch.nn.functional.gelu(ref)
    elif act == 2:
        ref = torch.relu(ref)
    if resid:
        ref = ref + R.double()
    out = torch.empty(M, N, device=DEV)
    Ad, Wd, bd = A.to(DEV), Wt.to(DEV), b.to(DEV)
    Rd = R.to(DEV) if resid else None
    _lib.check(lib.sta_debug_gemm(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K, act, via_f16,
                                  Rd.data_ptr() if resid else None, out.data_ptr(), st()))
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), ref.numpy()
    res = {"rel_l2": rel_l2(o, r), "max_rel": max_rel(o, r), "plan": last_plan(lib, h), "nan": int(np.isnan(o).sum())}
    if tail_rows:
        res.update(rel_l2_tail=rel_l2(o[M - tail_rows:], r[M - tail_rows:]), max_rel_tail=max_rel(o[M - tail_rows:], r[M - tail_rows:]))
    return res


def check_qkv_rope(precision, S=2, hp=3, wp=4, pose_tok=1, K=128, Cdim=128, seed=1, variant=0):
    m, lib, h = kernel_handle(precision, variant)
    g = torch.Generator().manual_seed(seed)
    ntok = hp * wp + pose_tok
    x = torch.randn(S * ntok, K, generator=g)
    Wt = torch.randn(3 * Cdim, K, generator=g) * 0.1
    b = torch.randn(3 * Cdim, generator=g) * 0.1
    heads = Cdim // 64
    npad = (ntok + 63) // 64 * 64
    q = torch.full((S, heads, ntok, 64), float("nan"), device=DEV)      # (an element no block writes stays NaN and fails every bar)
    k = torch.full_like(q, float("nan"))
    vt = torch.empty(S * heads * 64, npad, device=DEV)
    xd, Wd, bd = x.to(DEV), Wt.to(DEV), b.to(DEV)      # keep device inputs alive across the call
    _lib.check(lib.sta_debug_qkv_rope(h, xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), S, ntok, K, Cdim,
                                      wp, pose_tok, q.data_ptr(), k.data_ptr(), vt.data_ptr(), st()))
    torch.cuda.synchronize()
    y = (x.double() @ Wt.double().T + b.double()).float().reshape(S, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4).numpy()
    pos = grid_pos(S, hp, wp, pose_tok=bool(pose_tok))
    qr, kr, vr = rope2d_ref(y[0], pos), rope2d_ref(y[1], pos), y[2]
    v = vt.cpu().numpy().reshape(S, heads, 64, npad)[..., :ntok].transpose(0, 1, 3, 2)
    pad = vt.cpu().numpy().reshape(S, heads, 64, npad)[..., ntok:]
    return {"q": max_rel(q.cpu().numpy(), qr), "k": max_rel(k.cpu().numpy(), kr), "v": max_rel(v, vr),
            "vpad_abs": float(np.abs(pad).max()) if pad.size else 0.0, "plan": last_plan(lib, h),
            "nan": int(np.isnan(q.cpu().numpy()).sum() + np.isnan(k.cpu().numpy()).sum() + np.isnan(v).sum())}


def check_attention(precision, S=2, heads=2, nq=197, nk=197, kv_shift=0, sharp=1.0, seed=2):
    m, lib, h = kernel_handle(precision)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(S, heads, nq, 64, generator=g) * sharp
    k = torch.randn(S, heads, nk, 64, generator=g)
    v = torch.randn(S, heads, nk, 64, generator=g)
    idx = [(s + kv_shift) % S for s in range(S)]
    a = (q.double() @ k[idx].double().transpose(-1, -2)) * 0.125
    ref = (a.softmax(-1) @ v[idx].double()).permute(0, 2, 1, 3).reshape(S, nq, heads * 64)
    out = torch.empty(S, nq, heads * 64, device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    _lib.check(lib.sta_debug_attention(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, nq, nk,
                                       kv_shift, out.data_ptr(), st()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return {"rel_l2": rel_l2(o, ref.numpy()), "max_rel": max_rel(o, ref.numpy()), "nan": float(np.isnan(o).sum())}


def check_gemm_tail(precision, tiles_m=12, tail=16, N=2304, K=256, act=0, via_f16=0, resid=False, variant=0, seed=11, M=None):
    """Dense GEMM whose last `tail` rows are the decoder's pose-token rows (tail hint; GemmParams::m_tail): M = tiles_m x 192
    (or 256 under a forced 256-row family) + tail, unless M is given.  Returns the errors, those of the tail rows alone, and the
    plan the GEMM ran under (whether the tail blocks took the rows is for the caller to assert)."""
    m, lib, h = kernel_handle(precision, variant)
    bm = 256 if variant == 2 else 192
    M = tiles_m * bm + tail if M is None else M
    _lib.check(lib.sta_debug_set_tail_hint(h, tail))
    try:
        r = check_gemm(precision, M=M, N=N, K=K, act=act, via_f16=via_f16, resid=resid, seed=seed, variant=variant, tail_rows=tail)
    finally:
        _lib.check(lib.sta_debug_set_tail_hint(h, 0))
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    return r


def split_linear(seed, rows, N, K, precision, v_cols):
    """split_cases.linear_operands as float32 torch tensors: x [*rows, K], W [N, K], b [N], and the ONE right value of the columns
    v_cols [prod(rows), len(v_cols)] float64."""
    import split_cases as SC
    x, w, b, want = SC.linear_operands(seed, rows, N, K, precision, v_cols, HP.mm64)
    return torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), want


def check_qkv_rope_decoder_rows(precision, S=2, hp=3, wp=4, K=128, Cdim=128, seed=12, variant=0, ints=False):
    """QKV + RoPE epilogue on the decoder's row order: x = [S*N patch rows | S pose rows]; the buffers hold N + 1 tokens per
    sequence with the pose token (position -1) last.  ints: split operands with ONE right answer (split_linear) - the un-rotated V
    columns must come out EXACT, both parts ("v_exact_bad")."""
    m, lib, h = kernel_handle(precision, variant)
    g = torch.Generator().manual_seed(seed)
    N = hp * wp
    ntok = N + 1
    if ints:
        xs, Wt, b, v_want = split_linear(seed, (S, ntok), 3 * Cdim, K, precision, slice(2 * Cdim, 3 * Cdim))
    else:
        xs = torch.randn(S, ntok, K, generator=g)                 # reference order: pose token first
        Wt = torch.randn(3 * Cdim, K, generator=g) * 0.1
        b = torch.randn(3 * Cdim, generator=g) * 0.1
    heads = Cdim // 64
    npad = (ntok + 63) // 64 * 64
    x_dec = torch.cat([xs[:, 1:].reshape(S * N, K), xs[:, 0]], 0).contiguous()
    q = torch.empty(S, heads, ntok, 64, device=DEV)
    k = torch.empty_like(q)
    vt = torch.empty(S * heads * 64, npad, device=DEV)
    xd, Wd, bd = x_dec.to(DEV), Wt.to(DEV), b.to(DEV)
    _lib.check(lib.sta_debug_qkv_rope(h, xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), S, N, K, Cdim,
                                      wp, 2, q.data_ptr(), k.data_ptr(), vt.data_ptr(), st()))
    torch.cuda.synchronize()
    y = (xs.reshape(S * ntok, K).double() @ Wt.double().T + b.double()).float().reshape(S, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4).numpy()
    pos = grid_pos(S, hp, wp, pose_tok=True)
    qr, kr, vr = rope2d_ref(y[0], pos), rope2d_ref(y[1], pos), y[2]
    order = list(range(1, ntok)) + [0]                          # device token order: patches, then the pose token
    v = vt.cpu().numpy().reshape(S, heads, 64, npad)[..., :ntok].transpose(0, 1, 3, 2)
    pad = vt.cpu().numpy().reshape(S, heads, 64, npad)[..., ntok:]
    plan = last_plan(lib, h)
    _lib.check(lib.sta_set_gemm_variant(h, 0))
    qd_, kd_ = q.cpu().numpy(), k.cpu().numpy()
    res = {"q": max_rel(qd_, qr[:, :, order]), "k": max_rel(kd_, kr[:, :, order]), "v": max_rel(v, vr[:, :, order]),
           "q_pose": max_rel(qd_[:, :, -1:], qr[:, :, :1]), "k_pose": max_rel(kd_[:, :, -1:], kr[:, :, :1]),
           "v_pose": max_rel(v[:, :, -1:], vr[:, :, :1]),
           "vpad_abs": float(np.abs(pad).max()) if pad.size else 0.0, "plan": plan}
    if ints:
        want = v_want.reshape(S, ntok, heads, 64).transpose(0, 2, 1, 3)[:, :, order]
        res["v_exact_bad"], res["v_first"] = HP.first_wrong(v, want, np.rint(want), ("sequence", "head", "token", "column"))
    return res


def check_qkv_pair(precision, S=4, hp=24, wp=32, Cdim=768, K=768, ints=False, seed=14):
    """The decoder's paired launch (gemm_qkv_pair): a = attn.qkv (q | k | v) and b = cross_attn.projk|projv (k | v, nq = 0) on
    two inputs in the decoder's row order [S*N patch rows | S pose rows], pose-token tail hint S.  Against an fp64 reference +
    RoPE (pose token at position -1).  ints: operands hi + q 2^-12 with ONE right answer (split_linear), so that V (not rotated) must
    come out EXACT for both halves, hi and lo plane - any column offset of the second GEMM in the one-grid launch, and any dropped or
    misplaced correction product, shows up as a wrong value."""
    m, lib, h = kernel_handle(precision)
    g = torch.Generator().manual_seed(seed)
    N = hp * wp
    nt = N + 1
    heads = Cdim // 64
    npad = (nt + 63) // 64 * 64

    def operand(*shape, scale):
        return torch.randn(*shape, generator=g) * scale
    if ints:      # split operands (hi + q 2^-12, both parts non-zero) with ONE right answer: split_linear
        xa, Wa, ba, va_want = split_linear(seed, (S, nt), 3 * Cdim, K, precision, slice(2 * Cdim, 3 * Cdim))
        xb, Wb, bb, vb_want = split_linear(seed + 1, (S, nt), 2 * Cdim, K, precision, slice(Cdim, 2 * Cdim))
    else:
        xa, xb = operand(S, nt, K, scale=1.0), operand(S, nt, K, scale=1.0)        # reference order: pose token first
        Wa, Wb = operand(3 * Cdim, K, scale=0.05), operand(2 * Cdim, K, scale=0.05)
        ba, bb = operand(3 * Cdim, scale=0.1), operand(2 * Cdim, scale=0.1)

    def dec(x):
        return torch.cat([x[:, 1:].reshape(S * N, K), x[:, 0]], 0).contiguous()
    q_a = torch.empty(S, heads, nt, 64, device=DEV)
    k_a, k_b = torch.empty_like(q_a), torch.empty_like(q_a)
    vt_a = torch.empty(S * heads * 64, npad, device=DEV)
    vt_b = torch.empty_like(vt_a)
    ins = [dev(t.numpy()) for t in (dec(xa), Wa, ba, dec(xb), Wb, bb)]
    _lib.check(lib.sta_debug_set_tail_hint(h, 0))
    _lib.check(lib.sta_debug_qkv_pair(h, *[t.data_ptr() for t in ins], S, N, K, Cdim, wp, q_a.data_ptr(), k_a.data_ptr(),
                                      vt_a.data_ptr(), k_b.data_ptr(), vt_b.data_ptr(), st()))
    torch.cuda.synchronize()
    plan = last_plan(lib, h)
    ya = (xa.reshape(S * nt, K).double() @ Wa.double().T + ba.double()).reshape(S, nt, 3, heads, 64).permute(2, 0, 3, 1, 4).numpy()
    yb = (xb.reshape(S * nt, K).double() @ Wb.double().T + bb.double()).reshape(S, nt, 2, heads, 64).permute(2, 0, 3, 1, 4).numpy()
    pos = grid_pos(S, hp, wp, pose_tok=True)
    order = list(range(1, nt)) + [0]                             # device token order: patches, then the pose token
    ref = {"q_a": rope2d_ref(ya[0], pos)[:, :, order], "k_a": rope2d_ref(ya[1], pos)[:, :, order], "v_a": ya[2][:, :, order],
           "k_b": rope2d_ref(yb[0], pos)[:, :, order], "v_b": yb[1][:, :, order]}
    got = {"q_a": q_a.cpu().numpy(), "k_a": k_a.cpu().numpy(), "k_b": k_b.cpu().numpy()}
    res = {"plan": plan}
    for name, vt in (("v_a", vt_a), ("v_b", vt_b)):
        full = vt.cpu().numpy().reshape(S, heads, 64, npad)
        got[name] = full[..., :nt].transpose(0, 1, 3, 2)
        res[name + "_pad_abs"] = float(np.abs(full[..., nt:]).max()) if npad > nt else 0.0
    for name in ref:
        res[name] = max_rel(got[name], ref[name])
        res[name + "_pose"] = max_rel(got[name][:, :, -1:], ref[name][:, :, -1:])
    if ints:
        res["v_exact_bad"], res["v_first"] = 0, ""
        for n, w_ in (("v_a", va_want), ("v_b", vb_want)):
            want = w_.reshape(S, nt, heads, 64).transpose(0, 2, 1, 3)[:, :, order]
            bad, first = HP.first_wrong(got[n], want, np.rint(want), ("sequence", "head", "token", "column"))
            res["v_exact_bad"] += bad
            res["v_first"] += f"{n}: {first} " if bad else ""
    return res


def check_attention_pose(precision, S=2, heads=2, n=196, kv_shift=0, sharp=1.0, seed=13):
    """Decoder form of the attention kernel: n patch tokens + the pose token (last): as a key it is folded into the initial
    softmax state; as a query it rides in the last query block's spare rows (n % 128 != 0) or is served by the pose blocks."""
    m, lib, h = kernel_handle(precision)
    g = torch.Generator().manual_seed(seed)
    nt = n + 1
    q = torch.randn(S, heads, nt, 64, generator=g) * sharp
    k = torch.randn(S, heads, nt, 64, generator=g)
    v = torch.randn(S, heads, nt, 64, generator=g)
    idx = [(s + kv_shift) % S for s in range(S)]
    a = (q.double() @ k[idx].double().transpose(-1, -2)) * 0.125
    ref = (a.softmax(-1) @ v[idx].double()).permute(0, 2, 1, 3).reshape(S, nt, heads * 64)
    ref = torch.cat([ref[:, :n].reshape(S * n, heads * 64), ref[:, n]], 0)       # decoder row order
    out = torch.empty(S * n + S, heads * 64, device=DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    _lib.check(lib.sta_debug_attention_pose(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, n, kv_shift, out.data_ptr(), st()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return {"rel_l2": rel_l2(o, ref.numpy()), "rel_l2_pose": rel_l2(o[S * n:], ref.numpy()[S * n:]),
            "max_rel": max_rel(o, ref.numpy()), "nan": float(np.isnan(o).sum())}


# ---- tests/test_attention_exact.py: one launch of a case of tests/attention_cases.py, and the four kinds of check on it
def last_attn_plan(lib, h):
    """The plan (sta_launch.inc: attn_plan) of the handle's last attention launch."""
    import attention_cases as AC
    out = (C.c_int * len(AC.FIELDS))()
    _lib.check(lib.sta_debug_last_attn_plan(h, out))
    return dict(zip(AC.FIELDS, out))


def attn_launch(precision, case, q, k, v):
    """Run the case's launch on numpy q, k, v (token layout of helpers.py) -> (output per token [S, heads, nqt, 64] float32, the
    schedule class the launch ran under).  The output buffer starts as NaN and the debug entry poisons the planes the kernel writes
    to, so an element that no workgroup stored comes back as NaN."""
    import attention_cases as AC
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    m, lib, h = kernel_handle(precision)
    qd, kd, vd = dev(q), dev(k), dev(v)
    rows = S * nq + (S if form == "pose" else 0)
    out = torch.full((rows, heads * 64), float("nan"), device=DEV)
    _lib.check(lib.sta_debug_set_option(h, 5, opt5))
    try:
        if form == "pose":
            _lib.check(lib.sta_debug_attention_pose(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, nq, kv_shift, out.data_ptr(), st()))
        else:
            _lib.check(lib.sta_debug_attention(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, nq, nk, kv_shift, out.data_ptr(), st()))
        torch.cuda.synchronize()
        plan = last_attn_plan(lib, h)
    finally:
        _lib.check(lib.sta_debug_set_option(h, 5, 0))
    return HP.attn_rows_to_tokens(out.cpu().numpy(), form, S, heads, nq), AC.schedule_class(plan, nq)


def check_attention_selection(precision, case, pose_sel="self", seed=21, v_lo=False):
    """Every query selects one key with probability exactly 1 (helpers.attn_selection_inputs): the output must EQUAL V[pi(query)].
    v_lo: V = integer + lo (split_cases.attn_v_with_lo) - the output planes must hold BOTH parts of the selected row (f16: its hi).
    -> {"class", "margin", "nan", "wrong": number of wrong (sequence, head, query) rows, "first": text naming the first ones}."""
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    q, k, v, pi, margin = HP.attn_selection_inputs(form, S, heads, nq, nk, pose_sel, seed)
    assert margin > 160, (cid, margin)          # every other probability is exp2(-margin): exactly 0 in fp32
    vw = v
    if v_lo:
        import split_cases as SC
        v = SC.attn_v_with_lo(v, seed)
        assert SC.split_holds(v)
        vw = v.astype(np.float16).astype(np.float32) if precision == "f16" else v
    # q was built against its own sequence's keys: hand the kernel K / V rotated so that sequence (s + kv_shift) % S holds them
    idx = [(s - kv_shift) % S for s in range(S)]
    got, ran = attn_launch(precision, case, q, k[idx], v[idx])
    want = np.take_along_axis(vw, pi[..., None], 2)
    bad = np.argwhere((got != want).any(-1))
    first = []
    for s, h, t in bad[:6]:
        g = got[s, h, t]
        who = "pose query" if form == "pose" and t == nq else f"query {t}"
        first.append(f"(sequence {s}, head {h}, {who}): expected key {pi[s, h, t]} of (sequence {s}, head {h}), "
                     f"got columns 0..2 = (sequence {g[0]:g}, head {g[1]:g}, key {g[2]:g}), {int((g != want[s, h, t]).sum())} of 64 columns differ")
    return {"class": ran, "margin": margin, "nan": int(np.isnan(got).sum()), "wrong": len(bad), "first": "; ".join(first)}


def check_attention_decided(precision, case, seed=23):
    """Q K^T decided by the correction products alone (split_cases.attn_decided_inputs): every query has a selected key and a decoy
    that tie at exactly 0 in hi hi; f16x3 must return the selected V row (both parts), f16 - where the decoy ties - the mean of the
    hi parts of the two rows.  -> as check_attention_selection, with the family and the tiles of the first wrong rows."""
    import split_cases as SC
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    d = SC.attn_decided_inputs(form, S, heads, nq, nk, seed)
    m_dec, m_rest = SC.attn_decided_assert(d)
    idx = [(s - kv_shift) % S for s in range(S)]          # (q was built against its own sequence's keys)
    got, ran = attn_launch(precision, case, d["q"], d["k"][idx], d["v"][idx])
    want = SC.attn_decided_expected(d, precision)
    bad = np.argwhere((got != want).any(-1))
    first = []
    for s, h, t in bad[:6]:
        g, b, dk = got[s, h, t], d["pi"][s, h, t], d["dec"][s, h, t]
        first.append(f"(sequence {s}, head {h}, query {t}): selected key {b} (tile {b // 64}), decoy {dk} (tile {dk // 64}), separated by "
                     f"{'q_lo k_hi' if d['family'][s, h, t] else 'q_hi k_lo'}; got columns 0..2 = ({g[0]:g}, {g[1]:g}, {g[2]:g}), "
                     f"{int((g != want[s, h, t]).sum())} of 64 columns differ")
    return {"class": ran, "margin": (m_dec, m_rest), "nan": int(np.isnan(got).sum()), "wrong": len(bad), "first": "; ".join(first)}


def check_attention_uniform(precision, case, seed=22, v_lo=False):
    """q = 0: the output is the column mean of V over exactly nk (+ 1) keys.  -> max |error|, max |V|, the fp16 half-ulp of the
    largest mean (what the f16 form's single output rounding adds).  v_lo: V + lo of one sign per column
    (split_cases.attn_uniform_lo); the f16 form must return the mean of the hi parts."""
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    q, k, v = HP.attn_uniform_inputs(form, S, heads, nq, nk, seed)
    vw = v
    if v_lo:
        import split_cases as SC
        vw, v = v, SC.attn_uniform_lo(v, seed)[0]
        assert SC.split_is(v, (vw, np.rint((v.astype(np.float64) - vw) * 4096)))
        if precision != "f16":
            vw = v
    got, ran = attn_launch(precision, case, q, k, v)
    idx = [(s + kv_shift) % S for s in range(S)]
    ref = np.broadcast_to(vw[idx].astype(np.float64).mean(2, keepdims=True), got.shape)
    err = np.abs(got - ref)
    w = np.unravel_index(np.nanargmax(err), err.shape) if not np.isnan(err).all() else (0, 0, 0, 0)
    return {"class": ran, "nan": int(np.isnan(got).sum()), "max_abs": float(np.nanmax(err)) if not np.isnan(err).all() else float("nan"),
            "vmax": float(np.abs(v).max()), "half_ulp16": float(2.0 ** (np.floor(np.log2(np.abs(ref).max())) - 11)),
            "worst": f"(sequence {w[0]}, head {w[1]}, query {w[2]}, column {w[3]}): got {got[w]} want {ref[w]}"}


def _attn_rows(precision, case, q, k, v):
    cid, form, S, heads, nq, nk, kv_shift, opt5, cls = case
    got, ran = attn_launch(precision, case, q, k, v)
    rows, glob = HP.attn_row_errors(got, HP.attn_ref64(q, k, v, kv_shift))
    w = np.unravel_index(np.nanargmax(rows), rows.shape) if not np.isnan(rows).all() else (0, 0)
    return {"class": ran, "nan": int(np.isnan(got).sum()), "rel_l2": glob, "worst_row": float(np.nanmax(rows)) if not np.isnan(rows).all() else float("nan"),
            "worst": f"(sequence {w[0]}, query {w[1]})"}


def check_attention_ramp(precision, case, pattern, seed=101):
    """Scores that rise / fall tile by tile or peak in the last tile / at the pose key (helpers.attn_ramp_inputs) against the fp64
    softmax; per-row rel-L2."""
    cid, form, S, heads, nq, nk = case[:6]
    return _attn_rows(precision, case, *HP.attn_ramp_inputs(form, S, heads, nq, nk, pattern, seed))


def check_attention_rows(precision, case, sharp, seed=100):
    """Gaussian inputs, rel-L2 of every (sequence, query) row and of the whole output."""
    cid, form, S, heads, nq, nk = case[:6]
    return _attn_rows(precision, case, *HP.attn_gaussian_inputs(form, S, heads, nq, nk, sharp, seed))


def check_conv3(precision, n=2, H=7, W_=5, Cin=32, Co=48, stride=1, relu_in=0, act=0, resid=False, seed=3, variant=0):
    m, lib, h = kernel_handle(precision, variant)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, Cin, H, W_, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) * 0.1
    b = torch.randn(Co, generator=g)
    xin = torch.relu(x) if relu_in else x
    ref = torch.nn.functional.conv2d(xin.double(), w.double(), b.double(), stride=stride, padding=1)
    if act == 2:
        ref = torch.relu(ref)
    R = torch.randn(ref.shape, generator=g) if resid else None
    if resid:
        ref = ref + R.double()
    Ho, Wo = ref.shape[2], ref.shape[3]
    out = torch.empty(n, Ho, Wo, Co, device=DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    Rd = R.permute(0, 2, 3, 1).contiguous().to(DEV) if resid else None
    wd, bd = w.to(DEV), b.to(DEV)
    _lib.check(lib.sta_debug_conv3x3(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cin, Co, stride,
                                     relu_in, act, Rd.data_ptr() if resid else None, out.data_ptr(), st()))
    torch.cuda.synchronize()
    o = out.cpu().permute(0, 3, 1, 2).numpy()
    return {"rel_l2": rel_l2(o, ref.numpy()), "max_rel": max_rel(o, ref.numpy()), "plan": last_plan(lib, h), "nan": int(np.isnan(o).sum())}


def check_convt(precision, n=2, H=3, W_=5, Cdim=96, k=4, seed=4, variant=0):
    m, lib, h = kernel_handle(precision, variant)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, Cdim, H, W_, generator=g)
    w = torch.randn(Cdim, Cdim, k, k, generator=g) * 0.1
    b = torch.randn(Cdim, generator=g)
    ref = torch.nn.functional.conv_transpose2d(x.double(), w.double(), b.double(), stride=k)
    out = torch.empty(n, H * k, W_ * k, Cdim, device=DEV)
    xd, wd, bd = x.permute(0, 2, 3, 1).contiguous().to(DEV), w.to(DEV), b.to(DEV)
    _lib.check(lib.sta_debug_convt(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cdim, k, out.data_ptr(), st()))
    torch.cuda.synchronize()
    o = out.cpu().permute(0, 3, 1, 2).numpy()
    return {"rel_l2": rel_l2(o, ref.numpy()), "max_rel": max_rel(o, ref.numpy()), "plan": last_plan(lib, h), "nan": int(np.isnan(o).sum())}


def check_up2(precision, n=2, H=7, W_=5, Cdim=16, crop=None, seed=5, one_row=0, ints=False):
    """one_row: experiment switch 7 (one output row per workgroup where the product would run four).  ints: integer inputs.  Also
    the error of every border class (helpers.conv_pixel_classes, and the rows of the last, partly filled group of four)."""
    m, lib, h = kernel_handle(precision)
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1024, 1025, (n, Cdim, H, W_), generator=g).float() if ints else torch.randn(n, Cdim, H, W_, generator=g)
    ref = torch.nn.functional.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
    Hc, Wc = crop if crop else (2 * H, 2 * W_)
    ref = ref[:, :, :Hc, :Wc]
    out = torch.empty(n, Hc, Wc, Cdim, device=DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    _lib.check(lib.sta_debug_set_option(h, 7, one_row))
    try:
        _lib.check(lib.sta_debug_up2(h, xd.data_ptr(), n, H, W_, Cdim, Hc, Wc, out.data_ptr(), st()))
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.sta_debug_set_option(h, 7, 0))
    o = out.cpu().permute(0, 3, 1, 2).numpy()
    masks = HP.conv_pixel_classes(n, Hc, Wc, None, 1)
    if Hc % 4:
        masks["last_group_of_four_rows"] = np.broadcast_to((np.arange(Hc) >= 4 * ((Hc - 1) // 4))[None, :, None], (n, Hc, Wc))
    errs = HP.class_errors(out.cpu().numpy(), ref.permute(0, 2, 3, 1).numpy(), masks, channel_blocks=False)
    return {"rel_l2": rel_l2(o, ref.numpy()), "max_rel": max_rel(o, ref.numpy()), "nan": int(np.isnan(o).sum()),
            "worst": HP.worst_class(errs), "exact_bad": int((o.astype(np.float64) != ref.numpy()).sum())}


def check_layernorm(precision, M=37, Cdim=768, seed=6):
    m, lib, h = kernel_handle(precision)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Cdim, generator=g) * 3 + 0.7
    w = torch.randn(Cdim, generator=g)
    b = torch.randn(Cdim, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (Cdim,), w.double(), b.double(), eps=1e-6).numpy()
    o32 = torch.empty(M, Cdim, device=DEV)
    op = torch.empty(M, Cdim, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    _lib.check(lib.sta_debug_layernorm(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), M, Cdim, 1e-6,
                                       o32.data_ptr(), op.data_ptr(), st()))
    torch.cuda.synchronize()
    return {"f32": max_rel(o32.cpu().numpy(), ref), "planes": max_rel(op.cpu().numpy(), ref)}


def check_ops_golden(precision):
    """Single-op vectors produced by the reference's own modules (tests/golden/ops.npz)."""
    m, lib, h = kernel_handle(precision)
    g, _ = load_golden("ops")
    res = {}
    # RoPE2D in place (curope drop-in), tokens given as (B,H,N,D) -> kernel layout (B,N,H,D)
    tok = dev(g["rope_tok"]).permute(0, 2, 1, 3).contiguous()
    rpos = dev(g["rope_pos"])
    rope2d_inplace(tok, rpos, 100.0, 1.0)
    res["rope2d"] = max_rel(tok.permute(0, 2, 1, 3).cpu().numpy(), g["rope_out"])
    # inverse rotation (fwd = -1) restores the input (curope backward, curope2d.py:24-29)
    rope2d_inplace(tok, rpos, 100.0, -1.0)
    res["rope2d_roundtrip"] = max_rel(tok.permute(0, 2, 1, 3).cpu().numpy(), g["rope_tok"])
    # the other token dtypes curope dispatches on (kernels.cu:101): fp32 rotation of the stored value, result stored in that dtype
    for dt, name in ((torch.float16, "f16"), (torch.float64, "f64")):
        t0 = dev(g["rope_tok"]).permute(0, 2, 1, 3).contiguous().to(dt)
        want = torch.from_numpy(rope2d_ref(t0.float().permute(0, 2, 1, 3).cpu().numpy(), g["rope_pos"])).to(dt)
        rope2d_inplace(t0, rpos, 100.0, 1.0)
        res["rope2d_" + name] = max_rel(t0.permute(0, 2, 1, 3).cpu().double().numpy(), want.double().numpy())
    # LayerNorm eps 1e-6
    M, Cd = g["ln_x"].shape
    o32 = torch.empty(M, Cd, device=DEV); op = torch.empty(M, Cd, device=DEV)
    lx, lw, lb = dev(g["ln_x"]), dev(g["ln_w"]), dev(g["ln_b"])
    _lib.check(lib.sta_debug_layernorm(h, lx.data_ptr(), lw.data_ptr(), lb.data_ptr(),
                                       M, Cd, 1e-6, o32.data_ptr(), op.data_ptr(), st()))
    res["layernorm"] = max_rel(o32.cpu().numpy(), g["ln_out"])
    # SVD orthogonalisation incl. reflection / near-singular inputs
    B = g["svd_in"].shape[0]
    r = torch.empty(B, 3, 3, device=DEV)
    sv = dev(g["svd_in"])
    _lib.check(lib.sta_debug_svd_orthogonalize(h, sv.data_ptr(), r.data_ptr(), B, st()))
    res["svd_orth"] = float(np.abs(r.cpu().numpy() - g["svd_out"]).max())
    # bilinear x2 align_corners, odd size: channels padded to 8
    x = g["bilin_x"]
    xp = np.zeros((1, 8, x.shape[2], x.shape[3]), np.float32); xp[:, :3] = x
    out = torch.empty(1, 2 * x.shape[2], 2 * x.shape[3], 8, device=DEV)
    xpd = dev(xp.transpose(0, 2, 3, 1))
    _lib.check(lib.sta_debug_up2(h, xpd.data_ptr(), 1, x.shape[2], x.shape[3], 8,
                                 2 * x.shape[2], 2 * x.shape[3], out.data_ptr(), st()))
    res["bilinear"] = max_rel(out.cpu().numpy().transpose(0, 3, 1, 2)[:, :3], g["bilin_out"])
    # postprocess through head_final: weights = identity on the first 4 channels
    pin = g["post_in"]                       # [1,4,h,w]
    npix = pin.shape[2] * pin.shape[3]
    feat = np.zeros((npix, 128), np.float32); feat[:, :4] = pin[0].reshape(4, npix).T
    w4 = np.zeros((4, 128), np.float32); w4[np.arange(4), np.arange(4)] = 1.0
    pts = torch.empty(npix, 3, device=DEV); conf = torch.empty(npix, device=DEV)
    fd, w4d, b4d = dev(feat), dev(w4), dev(np.zeros(4, np.float32))
    _lib.check(lib.sta_debug_head_final(h, fd.data_ptr(), w4d.data_ptr(), b4d.data_ptr(),
                                        npix, pts.data_ptr(), conf.data_ptr(), st()))
    res["post_pts"] = max_rel(pts.cpu().numpy().reshape(pin.shape[2], pin.shape[3], 3), g["post_pts"][0])
    res["post_conf"] = max_rel(conf.cpu().numpy().reshape(pin.shape[2], pin.shape[3]), g["post_conf"][0])
    torch.cuda.synchronize()
    return res


# ------------------------------------------------------------------------------------------ end to end
def run_golden_case(name, precision, taps=True, variant=0, frontend=None):
    """HIP forward on the procedural inputs of a golden case; returns {key: rel-L2 error}.  frontend: a frontend that already holds
    the weights the fixture was generated with (the real-checkpoint kit: weights from a FILE) instead of the procedural ones."""
    g, meta = load_golden(name)
    cfg_name = "tiny" if int(meta["cfg_enc_embed_dim"]) == W.TINY.enc_embed_dim else "full"
    if frontend is not None:
        m = frontend
        m.set_precision(precision)
    else:
        m = model(cfg_name, float(meta["qk_gain"]), precision, int(meta["seed"]), int(meta.get("outlier", 0)), hooks=variant != 0)
    set_variant(m, variant)
    cfg = m.cfg
    m.range_report(reset=True)
    H, W_, B, sub = int(meta["H"]), int(meta["W"]), int(meta["B"]), int(meta["sub"])
    gen = W.smooth_images if int(meta["smooth"]) else W.synth_images
    imgs = gen(2 * B, H, W_, seed=int(meta["seed"]), tag=0)
    a, b = dev(imgs[:B]), dev(imgs[B:])
    res = {}
    main, supp = m.forward_pair(a, b)
    torch.cuda.synchronize()
    for side, o in (("main", main), ("supp", supp)):
        pts = o["pts3d_pred"].cpu().numpy(); conf = o["conf"].cpu().numpy()
        res[f"{side}_pts3d"] = rel_l2(pts[:, ::sub, ::sub], g[f"{side}_pts3d"])
        res[f"{side}_conf"] = rel_l2(conf[:, ::sub, ::sub], g[f"{side}_conf"])
        res[f"{side}_pose"] = rel_l2(o["relative_pose"].cpu().numpy(), g[f"{side}_pose"])
        res[f"{side}_pose_conf"] = rel_l2(o["relative_pose_conf"].cpu().numpy(), g[f"{side}_pose_conf"])
        # the same outputs in the max norm (max-abs error / max-abs value): an isolated bad pixel that rel-L2 averages away shows here
        res[f"{side}_pts3d_maxrel"] = max_rel(pts[:, ::sub, ::sub], g[f"{side}_pts3d"])
        res[f"{side}_conf_maxrel"] = max_rel(conf[:, ::sub, ::sub], g[f"{side}_conf"])
        res[f"{side}_pose_maxrel"] = max_rel(o["relative_pose"].cpu().numpy(), g[f"{side}_pose"])
        if "rand_idx" in g:      # off-lattice pixels of the sub-sampled fixtures: every pixel phase of the patch / conv tile / ConvT / bilinear grids
            ri = g["rand_idx"]
            pr, cr = pts.reshape(pts.shape[0], -1, 3)[:, ri], conf.reshape(conf.shape[0], -1)[:, ri]
            res[f"{side}_pts3d_rand"] = rel_l2(pr, g[f"{side}_pts3d_rand"]); res[f"{side}_pts3d_rand_maxrel"] = max_rel(pr, g[f"{side}_pts3d_rand"])
            res[f"{side}_conf_rand"] = rel_l2(cr, g[f"{side}_conf_rand"]); res[f"{side}_conf_rand_maxrel"] = max_rel(cr, g[f"{side}_conf_rand"])
        res[f"{side}_pts3d_norm"] = abs(float(np.sqrt((pts.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[0]) / float(g[f"{side}_pts3d_l2"][0]) - 1.0)
    # split entry points (what slam.py calls): encoder features + decoder hooks
    ts = torch.tensor([[H, W_]] * B)
    fa, pa = m._encode_image(a, ts, normalize=False)
    fb, pb = m._encode_image(b, ts, normalize=False)
    d1, d2 = m._decode_stereo(fa, fb, pa, pb)
    torch.cuda.synchronize()
    tsub = max(1, sub)
    # the integer output of _encode_image (PositionGetter, sta_blocks.py:241-247; slam.py:144 stores it per keyframe and feeds it
    # back at :162): bit-exact - dtype, shape and every entry (0.0 = identical, 1.0 = not; the callers compare with a tolerance)
    for key, got in (("pos_a", pa), ("pos_b", pb)):
        want = g[key]
        gotn = got.cpu().numpy()
        res[key] = 0.0 if (got.dtype == torch.int64 and gotn.shape == want.shape and want.dtype == np.int64 and np.array_equal(gotn, want)) else 1.0
    res["enc_feat_a"] = rel_l2(fa.cpu().numpy()[:, ::tsub], g["enc_feat_a"])
    res["enc_feat_b"] = rel_l2(fb.cpu().numpy()[:, ::tsub], g["enc_feat_b"])
    for hk in cfg.hooks[1:]:
        res[f"dec1_hook{hk - 1}"] = rel_l2(d1[hk - 1].cpu().numpy()[:, ::tsub], g[f"dec1_hook{hk - 1}"])
        res[f"dec2_hook{hk - 1}"] = rel_l2(d2[hk - 1].cpu().numpy()[:, ::tsub], g[f"dec2_hook{hk - 1}"])
    # split heads == monolithic forward
    pose = m.head_pose_s(d1[-1][:, 0, :])
    hp = m.head_pts([fa] + [t[:, 1:, :] for t in d1], ts)
    torch.cuda.synchronize()
    res["split_pose_vs_golden"] = rel_l2(pose["pose"].cpu().numpy(), g["main_pose"])
    res["split_pts_vs_golden"] = rel_l2(hp["pts3d"].cpu().numpy()[:, ::sub, ::sub], g["main_pts3d"])
    if taps and "dec1_in" in g:
        res["dec1_in"] = rel_l2(d1[0].cpu().numpy(), g["dec1_in"])
    global last_range
    last_range = m.range_report(reset=True)
    return res


# ---- tests/test_conv_exact.py: one launch of a case of tests/conv_cases.py, and the kinds of check on it.  Inputs and float64
# references are cached for the LAST case of each kind only: the parametrisation runs the three arithmetics of one case back to back.
_conv_cache = {}


def _cached(key, make):
    kind = key[0]
    if kind not in _conv_cache or _conv_cache[kind][0] != key:
        _conv_cache[kind] = (key, make())
    return _conv_cache[kind][1]


def conv_launch(precision, case, x, w, b, res, expect_range=(0, 0)):
    """Run the case's launch (sta_debug_conv3x3_r2) on numpy NHWC inputs -> (output [n, Ho, Wo, Co] float32, the class the launch ran
    under).  The output buffer starts as NaN and the entry poisons the output planes: an element no workgroup stored is a NaN.
    expect_range: which of the two range counters the launch must leave non-zero (range_class); default: none."""
    import conv_cases as CC
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case
    assert len(res) == nres
    m, lib, h = kernel_handle(precision, variant)
    Ho, Wo = CC.out_size(H, W_, stride)
    out = torch.full((n, Ho, Wo, Co), float("nan"), device=DEV)
    xd, wd, bd = dev(x), dev(w), dev(b)
    rd = [dev(r) for r in res]
    m.range_report(reset=True)
    try:
        _lib.check(lib.sta_debug_conv3x3_r2(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cin, Co, stride, relu_in, act,
                                            rd[0].data_ptr() if nres > 0 else None, rd[1].data_ptr() if nres > 1 else None,
                                            out.data_ptr(), st()))
        torch.cuda.synchronize()
        plan = last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    rng = tuple(m.range_report(reset=True))
    assert range_class(rng) == range_class(expect_range), f"{cid} {precision}: range events (fp16 saturations, fp8 correction saturations) = {rng}, expected class {range_class(expect_range)}"
    return out.cpu().numpy(), CC.conv_class(plan, Cin, stride, CC.EPI_NAME[(relu_in, act, nres)])


def check_conv_selection(precision, case):
    """One-hot weights on inputs that carry their own address (helpers.conv_selection_inputs): the output must EQUAL the shifted
    input planes.  Residual planes, where the case has them, are zero.  -> {"class", "nan", "wrong", "first"}."""
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case

    def make():
        x, w, tap, ci = HP.conv_selection_inputs(n, H, W_, Cin, Co, relu_in)
        return x, w, tap, ci, HP.conv_selection_expected(x, tap, ci, stride, relu_in)
    x, w, tap, ci, want = _cached(("sel", cid), make)
    if act == 2:
        want = np.maximum(want, 0)
    res = [np.zeros(want.shape, np.float32)] * nres
    got, ran = conv_launch(precision, case, x, w, np.zeros(Co, np.float32), res)
    wrong, first = HP.conv_selection_report(got, want, tap, ci, stride)
    return {"class": ran, "nan": int(np.isnan(got).sum()), "wrong": wrong, "first": first}


def check_conv_integers(precision, case, seed=31):
    """Small-integer inputs, weights, bias and residuals (helpers.conv_integer_inputs): every exact output is an integer of
    magnitude <= 2048 (asserted here in int64), so every arithmetic must return the integer itself."""
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case

    def make():
        x, w, b, res = HP.conv_integer_inputs(n, H, W_, Cin, Co, stride, nres, seed)
        ref = HP.conv_ref64(x, w, b, stride, relu_in, act, res)
        want = np.rint(ref).astype(np.int64)
        assert np.array_equal(want.astype(np.float64), ref) and np.abs(want).max() <= 2048, (cid, np.abs(ref).max())
        return x, w, b, res, want
    x, w, b, res, want = _cached(("int", cid), make)
    got, ran = conv_launch(precision, case, x, w, b, res)
    bad = np.argwhere(~(got.astype(np.float64) == want))
    first = "; ".join(f"output (image {i}, y {y}, x {xo}), channel {co}: want {want[i, y, xo, co]}, got {got[i, y, xo, co]:g}" for i, y, xo, co in bad[:6])
    return {"class": ran, "nan": int(np.isnan(got).sum()), "wrong": len(bad), "first": first, "max_abs": int(np.abs(want).max())}


def check_conv_classes(precision, case, seed=32):
    """Gaussian inputs against the float64 conv2d: rel-L2 of the whole tensor and of every class of helpers.conv_pixel_classes and
    every 32-channel block.  -> {"class", "nan", "rel_l2", "errs": {class: error}, "worst": (class, error)}."""
    import conv_cases as CC
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case

    def make():
        x, w, b, res = HP.conv_gaussian_inputs(n, H, W_, Cin, Co, stride, nres, seed)
        return x, w, b, res, HP.conv_ref64(x, w, b, stride, relu_in, act, res)
    x, w, b, res, ref = _cached(("gauss", cid), make)
    got, ran = conv_launch(precision, case, x, w, b, res)
    Ho, Wo = CC.out_size(H, W_, stride)
    bm = {2: 256, 3: 192, 5: 192, 6: 128, 8: 256}[ran[0]]
    errs = HP.class_errors(got, ref, HP.conv_pixel_classes(n, Ho, Wo, ran[0], bm))
    return {"class": ran, "nan": int(np.isnan(got).sum()), "rel_l2": rel_l2(got, ref), "errs": errs, "worst": HP.worst_class(errs)}


# ---- tests/test_split_exact_gpu.py: operands with a lo part that have ONE right answer (tests/split_cases.py)
def check_gemm_split(precision, M, N, K, variant, resid=False, via_f16=0, seed=0, tail=0, plan=None, wg_over=None):
    """sta_debug_gemm on split operands; arguments as _int_gemm of tests/test_gemm_mfma16.py (tail hint, plan and workgroup
    assertions, NaN / residual start of the output).  -> {"wrong", "first", "nan", "plan"}."""
    import split_cases as SC

    def make():
        ops = SC.gemm_operands(M, N, K, resid, seed)
        for name in ("A", "W"):
            SC.assert_split(SC.value(ops[name]), ops[name], name)
        return ops, SC.gemm_terms(ops, HP.mm64)
    ops, t = _cached(("gemm_split", M, N, K, resid, seed), make)
    want = SC.gemm_expected(ops, t, precision, bool(via_f16))
    hi_only = SC.gemm_expected(ops, t, "f16", False)
    m, lib, h = kernel_handle(precision, variant)
    Ad, Wd, bd = dev(SC.value(ops["A"])), dev(SC.value(ops["W"])), dev(ops["b"].astype(np.float32))
    out = dev(SC.value(ops["R"])) if resid else torch.full((M, N), float("nan"), device=DEV)
    _lib.check(lib.sta_debug_set_tail_hint(h, tail))
    try:
        _lib.check(lib.sta_debug_gemm(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K, 0, via_f16,
                                      out.data_ptr() if resid else None, out.data_ptr(), st()))
        torch.cuda.synchronize()
        got_plan = last_plan(lib, h)
    finally:
        _lib.check(lib.sta_debug_set_tail_hint(h, 0))
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    if plan is not None:
        assert (got_plan["family"], got_plan["m_tail"]) == tuple(plan), got_plan
    if wg_over is not None:
        assert got_plan["tiles_m"] * got_plan["tiles_n"] * got_plan["ksplit"] > wg_over, got_plan
    got = out.cpu().numpy()
    wrong, first = HP.first_wrong(got, want, hi_only, ("row", "col"))
    return {"wrong": wrong, "first": first, "nan": int(np.isnan(got).sum()), "plan": got_plan}


def check_conv_split(precision, case, seed=33):
    """A case of tests/conv_cases.py on split inputs, weights and residuals (split_cases.conv_operands).  -> as check_conv_integers."""
    import split_cases as SC
    cid, n, H, W_, Cin, Co, stride, relu_in, act, nres, variant, cls = case

    def make():
        ops = SC.conv_operands(case, seed)
        t = HP.split_conv_terms(ops, stride)
        b = SC.conv_bias(ops, t)
        SC.conv_window(ops, b)
        for name, p in [("x", ops["x"]), ("w", ops["w"])] + [(f"residual {i}", r) for i, r in enumerate(ops["res"])]:
            SC.assert_split(SC.value(p), p, f"{cid} {name}")
        return ops, t, b
    ops, t, b = _cached(("conv_split", cid), make)
    want = SC.conv_expected(ops, t, b, precision)
    hi_only = SC.conv_expected(ops, t, b, "f16x3", wrong="hi_only")
    got, ran = conv_launch(precision, case, SC.value(ops["x"]), SC.value(ops["w"]), b.astype(np.float32), [SC.value(r) for r in ops["res"]])
    wrong, first = HP.first_wrong(got, want, hi_only, ("image", "y", "x", "channel"))
    return {"class": ran, "nan": int(np.isnan(got).sum()), "wrong": wrong, "first": first, "max_abs": float(np.abs(want).max())}


def check_convt_split(precision, H, W_, Cdim, k, variant=0):
    """sta_debug_convt on split operands (the rows of test_convt_dispatch_rows_integer_exact).  -> {"wrong", "first", "nan", "plan"}."""
    import split_cases as SC

    def make():
        ops = SC.convt_operands(H, W_, Cdim, k)
        for name in ("x", "w"):
            SC.assert_split(SC.value(ops[name]), ops[name], name)
        return ops, SC.convt_terms(ops, HP.mm64)
    ops, t = _cached(("convt_split", H, W_, Cdim, k), make)
    want = SC.convt_expected(ops, t, precision)
    hi_only = SC.convt_expected(ops, t, "f16x3", wrong="hi_only")
    n = ops["x"][0].shape[0]
    m, lib, h = kernel_handle(precision, variant)
    out = torch.full((n, H * k, W_ * k, Cdim), float("nan"), device=DEV)
    xd, wd, bd = dev(SC.value(ops["x"])), dev(SC.value(ops["w"])), dev(ops["b"].astype(np.float32))
    try:
        _lib.check(lib.sta_debug_convt(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cdim, k, out.data_ptr(), st()))
        torch.cuda.synchronize()
        plan = last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    got = out.cpu().numpy()
    wrong, first = HP.first_wrong(got, want, hi_only, ("image", "y", "x", "channel"))
    return {"wrong": wrong, "first": first, "nan": int(np.isnan(got).sum()), "plan": plan}


def tail_launch(precision, hcase, nA, x, w2, b2, w4, b4, expect_range=(0, 0)):
    """sta_debug_conv3_head on numpy inputs -> (pts [n, H, W, 3], conf [n, H, W], class).  The two output pairs are separate
    allocations of exactly nA and n - nA images, NaN before the launch.  expect_range: as conv_launch."""
    import conv_cases as CC
    cid, n, H, W_, variant, w4scale, cls = hcase
    m, lib, h = kernel_handle(precision, variant)
    pa, ca = torch.full((nA, H, W_, 3), float("nan"), device=DEV), torch.full((nA, H, W_), float("nan"), device=DEV)
    pb, cb = torch.full((n - nA, H, W_, 3), float("nan"), device=DEV), torch.full((n - nA, H, W_), float("nan"), device=DEV)
    ins = [dev(t) for t in (x, w2, b2, w4, b4)]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    m.range_report(reset=True)
    try:
        _lib.check(lib.sta_debug_conv3_head(h, *[t.data_ptr() for t in ins], n, H, W_, nA, ptr(pa), ptr(ca), ptr(pb), ptr(cb), st()))
        torch.cuda.synchronize()
        plan = last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    rng = tuple(m.range_report(reset=True))
    assert range_class(rng) == range_class(expect_range), f"{cid} {precision}: range events (fp16 saturations, fp8 correction saturations) = {rng}, expected class {range_class(expect_range)}"
    return torch.cat([pa, pb]).cpu().numpy(), torch.cat([ca, cb]).cpu().numpy(), CC.conv_class(plan, 128, 1, "head")


def check_tail_classes(precision, hcase, nA):
    """The fused tail on Gaussian inputs against float64 (helpers.tail_ref64), per pixel class, for pts and conf."""
    cid, n, H, W_, variant, w4scale, cls = hcase

    def make():
        ins = HP.tail_gaussian_inputs(n, H, W_, w4scale)
        return ins, HP.tail_ref64(*ins)
    ins, (rp, rc) = _cached(("tail", cid), make)
    pts, conf, ran = tail_launch(precision, hcase, nA, *ins)
    masks = HP.conv_pixel_classes(n, H, W_, ran[0], 256 if ran[0] == 8 else 192)
    ep = HP.class_errors(pts, rp, masks, channel_blocks=False)
    ec = HP.class_errors(conf[..., None], rc[..., None], masks, channel_blocks=False)
    return {"class": ran, "nan": int(np.isnan(pts).sum() + np.isnan(conf).sum()), "pts": rel_l2(pts, rp), "conf": rel_l2(conf, rc),
            "worst_pts": HP.worst_class(ep), "worst_conf": HP.worst_class(ec)}


def tail_exact_inputs(hcase, seed=42):
    """One-hot head.2 on inputs in {0, 1}, head.4 with four weights of +-1 per row (two of each sign, one per 32-channel block of the
    tile's four waves), integer bias: the four pre-activation sums are integers in [-3, 3].  -> inputs, pre [n, H, W, 4] int64."""
    cid, n, H, W_, variant, w4scale, cls = hcase
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2, size=(n, H, W_, 128)).astype(np.float32)
    tap, ci = HP.conv_selection_map(128, 128)
    w2 = np.zeros((128, 128, 3, 3), np.float32)
    w2[np.arange(128), ci, tap // 3, tap % 3] = 1.0
    y = HP.conv_selection_expected(x, tap, ci, 1, 0)                      # relu(y) = y: the inputs are not negative
    w4 = np.zeros((4, 128), np.float32)
    for o in range(4):
        for blk in range(4):
            w4[o, 32 * blk + (7 * o + 11 * blk + 3) % 32] = 1.0 if blk < 2 else -1.0
    b4 = np.array([1, -1, 0, 1], np.float32)
    pre = np.rint(y.astype(np.float64) @ w4.T.astype(np.float64) + b4).astype(np.int64)
    assert np.abs(pre).max() <= 3
    return (x, w2, np.zeros(128, np.float32), w4, b4), pre


def check_tail_exact(precision, hcase, nA):
    """The fused tail on inputs whose four pre-activation sums are known integers: pts / conf against the float64 activations of
    those integers, in ulps of the fp32 result.  -> worst ulp errors and the pixels that hold them."""
    cid, n, H, W_, variant, w4scale, cls = hcase
    ins, pre = _cached(("tail_exact", cid), lambda: tail_exact_inputs(hcase))
    rp, rc = HP.tail_activations64(pre)
    pts, conf, ran = tail_launch(precision, hcase, nA, *ins)

    def ulps(got, ref):
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        e = np.abs(got.astype(np.float64) - ref) / ulp
        e[np.isnan(got)] = np.inf
        w = np.unravel_index(np.argmax(e), e.shape)
        return float(e[w]), f"(image {w[0]}, y {w[1]}, x {w[2]}): pre-activations {pre[w[0], w[1], w[2]].tolist()}, got {got[w]!r}, want {ref[w]!r}"
    up, wp = ulps(pts, rp)
    uc, wc = ulps(conf, rc)
    return {"class": ran, "nan": int(np.isnan(pts).sum() + np.isnan(conf).sum()), "pts_ulp": up, "pts_worst": wp, "conf_ulp": uc, "conf_worst": wc}


# ---- tests/test_range_gpu.py: one launch of a debug entry between two resets of the handle's range counters
def with_range(m, launch):
    """Reset the range counters, run launch(), synchronise -> (what launch returned, (fp16 events, fp8 events))."""
    m.range_report(reset=True)
    r = launch()
    torch.cuda.synchronize()
    return r, tuple(m.range_report(reset=True))


def range_gemm(precision, A, Wt, b, act=0, via_f16=1, variant=0):
    """sta_debug_gemm on numpy operands -> (out [M, N] float32, report, plan of the launch)."""
    m, lib, h = kernel_handle(precision, variant)
    M, K = A.shape
    N = Wt.shape[0]
    Ad, Wd, bd = dev(A), dev(Wt), dev(b)
    out = torch.full((M, N), float("nan"), device=DEV)
    try:
        _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_gemm(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K, act, via_f16,
                                                                     None, out.data_ptr(), st())))
        plan = last_plan(lib, h)
    finally:
        _lib.check(lib.sta_set_gemm_variant(h, 0))
    return out.cpu().numpy(), rng, plan


def range_convt(precision, x, w, b, k):
    """sta_debug_convt on numpy NHWC x, w [C, C, k, k], b [C] -> (out [n, kH, kW, C], report, plan)."""
    m, lib, h = kernel_handle(precision)
    n, H, W_, Cd = x.shape
    xd, wd, bd = dev(x), dev(w), dev(b)
    out = torch.full((n, H * k, W_ * k, Cd), float("nan"), device=DEV)
    _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_convt(h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), n, H, W_, Cd, k, out.data_ptr(), st())))
    return out.cpu().numpy(), rng, last_plan(lib, h)


def range_up2(precision, x, Hc, Wc):
    """sta_debug_up2 on numpy NHWC x -> (out [n, Hc, Wc, C], report)."""
    m, lib, h = kernel_handle(precision)
    n, H, W_, Cd = x.shape
    xd = dev(x)
    out = torch.full((n, Hc, Wc, Cd), float("nan"), device=DEV)
    _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_up2(h, xd.data_ptr(), n, H, W_, Cd, Hc, Wc, out.data_ptr(), st())))
    return out.cpu().numpy(), rng


def range_layernorm(precision, x, g, b, eps):
    """sta_debug_layernorm (ln_kernel) -> (fp32 output, value of the planes, report)."""
    m, lib, h = kernel_handle(precision)
    M, Cd = x.shape
    xd, gd, bd = dev(x), dev(g), dev(b)
    o32 = torch.zeros(M, Cd, device=DEV); op = torch.zeros(M, Cd, device=DEV)
    _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_layernorm(h, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), M, Cd, eps,
                                                                      o32.data_ptr(), op.data_ptr(), st())))
    return o32.cpu().numpy(), op.cpu().numpy(), rng


def range_resid_ln(precision, A, Wt, b, x, g1, b1, eps):
    """sta_debug_gemm_resid_ln with one affine set -> (x' [M, N], value of the planes, report, plan)."""
    m, lib, h = kernel_handle(precision)
    M, K = A.shape
    N = Wt.shape[0]
    Ad, Wd, bd, xd, gd, b1d = dev(A), dev(Wt), dev(b), dev(x.copy()), dev(g1), dev(b1)
    o1 = torch.zeros(M, N, device=DEV)
    _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_gemm_resid_ln(h, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), xd.data_ptr(), M, N, K,
                                                                          gd.data_ptr(), b1d.data_ptr(), None, None, eps, o1.data_ptr(), None, st())))
    return xd.cpu().numpy(), o1.cpu().numpy(), rng, last_plan(lib, h)


def range_qkv_rope(precision, x, Wt, b, S, ntok, Cdim, wp):
    """sta_debug_qkv_rope in the decoder's row order (x = [S*ntok patch rows | S pose rows]) -> (q, k [S, heads, ntok + 1, 64],
    v^T [S, heads, 64, npad], report, plan)."""
    m, lib, h = kernel_handle(precision)
    K = x.shape[1]
    heads, nt = Cdim // 64, ntok + 1
    npad = (nt + 63) // 64 * 64
    q = torch.full((S, heads, nt, 64), float("nan"), device=DEV)
    k = torch.full_like(q, float("nan"))
    vt = torch.full((S * heads * 64, npad), float("nan"), device=DEV)
    xd, Wd, bd = dev(x), dev(Wt), dev(b)
    _, rng = with_range(m, lambda: _lib.check(lib.sta_debug_qkv_rope(h, xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), S, ntok, K, Cdim, wp, 2,
                                                                     q.data_ptr(), k.data_ptr(), vt.data_ptr(), st())))
    return q.cpu().numpy(), k.cpu().numpy(), vt.cpu().numpy().reshape(S, heads, 64, npad), rng, last_plan(lib, h)


def range_attention(precision, q, k, v, pose=False):
    """sta_debug_attention (q [S, heads, nq, 64], k / v [S, heads, nk, 64] -> out [S, nq, heads*64]) or, pose=True,
    sta_debug_attention_pose (q, k, v [S, heads, n + 1, 64] -> out [S*n + S, heads*64]) -> (out, report)."""
    m, lib, h = kernel_handle(precision)
    S, heads, nq, _ = q.shape
    nk = k.shape[2]
    qd, kd, vd = dev(q), dev(k), dev(v)
    if pose:
        out = torch.full((S * nq, heads * 64), float("nan"), device=DEV)
        fn = lambda: _lib.check(lib.sta_debug_attention_pose(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, nq - 1, 0, out.data_ptr(), st()))
    else:
        out = torch.full((S, nq, heads * 64), float("nan"), device=DEV)
        fn = lambda: _lib.check(lib.sta_debug_attention(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), S, heads, nq, nk, 0, out.data_ptr(), st()))
    _, rng = with_range(m, fn)
    return out.cpu().numpy(), rng


def range_rope(precision, entry, bufs, pos, pos_max, **kw):
    """One of the three rotation entries on numpy buffers (rotated in place, returned as hi + lo) -> ([buffers], report).
    entry "tokens" (S1, S2, heads, na, nb, which), "enc" (S, heads, ntok), "varlen" (S, heads, n: list)."""
    m, lib, h = kernel_handle(precision)
    d = [dev(b) for b in bufs]
    table = dev(np.ascontiguousarray(pos, np.int32))
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in d])
    if entry == "tokens":
        fn = lambda: _lib.check(lib.sta_debug_rope_tokens(h, ptrs, len(d), kw["S1"], kw["S2"], kw["heads"], kw["na"], kw["nb"], table.data_ptr(),
                                                          pos_max, kw["which"], st()))
    elif entry == "enc":
        fn = lambda: _lib.check(lib.sta_debug_rope_enc_tokens(h, ptrs, len(d), kw["S"], kw["heads"], kw["ntok"], table.data_ptr(), pos_max, 0, st()))
    else:
        n = (C.c_int * len(kw["n"]))(*kw["n"])
        fn = lambda: _lib.check(lib.sta_debug_rope_varlen(h, ptrs, len(d), kw["S"], kw["heads"], n, table.data_ptr(), pos_max, st()))
    _, rng = with_range(m, fn)
    return [t.cpu().numpy() for t in d], rng


# ---- tests/test_workspace_gpu.py: the scratch of the CURRENT stream's context of a frontend on the test-hooks library
def workspace_fill_rc(m, byte):
    """sta_debug_workspace_fill on the current stream -> the return code (0, or -1 with the message in sta_last_error)."""
    return m.lib.sta_debug_workspace_fill(m._h, m._stream(), int(byte))


def workspace_fill(m, byte):
    _lib.check(workspace_fill_rc(m, byte))


def workspace_info(m):
    """-> {"ws_cap", "plan_peak", "skbuf", "slab", "side_skbuf" (bytes), "pending"} of the current stream's context."""
    out = (C.c_int64 * 8)()
    _lib.check(m.lib.sta_debug_workspace_info(m._h, m._stream(), out))
    return dict(zip(("ws_cap", "plan_peak", "skbuf", "slab", "side_skbuf", "pending"), (int(v) for v in out)))


def workspace_tail(m, byte):
    """-> (bytes of workspace [planned peak + 4096, capacity) that differ from `byte`, offset of the first or -1).  Synchronises."""
    n_bad, first = C.c_int64(0), C.c_int64(0)
    _lib.check(m.lib.sta_debug_workspace_tail(m._h, m._stream(), int(byte), C.byref(n_bad), C.byref(first)))
    return int(n_bad.value), int(first.value)
