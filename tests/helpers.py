"""Shared test helpers: golden loading, error metrics, plain fp32 reference ops (own restatements,
pinned against tests/golden/ops.npz in test_refops_cpu.py)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    meta = dict(zip([str(k) for k in d.pop("meta_keys")], d.pop("meta_vals").tolist())) if "meta_keys" in d else {}
    return d, meta


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def max_rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rope2d_ref(tok, pos, base=100.0):
    """tok (B,H,N,D) float32, pos (B,N,2) int -> rotated copy (pos_embed.py:169-185 semantics)."""
    tok = np.asarray(tok, np.float32)
    B, H, N, D = tok.shape
    Q = D // 4
    out = tok.copy()
    inv = (1.0 / (np.float32(base) ** (np.arange(Q, dtype=np.float32) / np.float32(Q)))).astype(np.float32)
    for xy in range(2):
        ang = pos[:, None, :, xy, None].astype(np.float32) * inv[None, None, None, :]
        c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        u = tok[..., xy * 2 * Q: xy * 2 * Q + Q]
        v = tok[..., xy * 2 * Q + Q: xy * 2 * Q + 2 * Q]
        out[..., xy * 2 * Q: xy * 2 * Q + Q] = u * c - v * s
        out[..., xy * 2 * Q + Q: xy * 2 * Q + 2 * Q] = v * c + u * s
    return out


def grid_pos(B, hp, wp, pose_tok=False):
    yy, xx = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
    p = np.stack([yy.ravel(), xx.ravel()], -1).astype(np.int64)
    if pose_tok:
        p = np.concatenate([np.full((1, 2), -1, np.int64), p], 0)
    return np.broadcast_to(p[None], (B,) + p.shape).copy()


# ---------------------------------------------------------------------------------------------------------
# keyframe-sequence goldens (tests/golden/seq_*.npz, oracle/gen_golden.py gen_seq): one record per candidate edge
def seq_meta(meta):
    return {k: int(meta[k]) for k in ("H", "W", "nkf", "neighbor_edge_num", "loop_edge_num", "loop_dist_min", "sub", "nrand", "seed", "tag")}


def compare_seq_edges(edges, g, meta, tol=1e-3):
    """`edges`: list of dicts {i, j, pose [4,4], conf float, accepted bool, confs [2,H,W] / None, intri, depths, scales [2] with
    NaN for 'no scale edge', scale_confs [2]} (numpy), in the reference's edge order.  Compares every field of every edge of the
    golden `g`: decisions and (i, j) exactly, numbers as rel-L2 AND max-abs / max-abs - both below `tol`.  -> worst errors."""
    m = seq_meta(meta)
    n = int(g["n_edges"])
    assert len(edges) == n, (len(edges), n)
    sub, rand_idx = m["sub"], g.get("rand_idx")
    worst = {}

    def note(key, got, want):
        e1, e2 = rel_l2(got, want), max_rel(got, want)
        worst[key] = max(worst.get(key, 0.0), e1)
        worst[key + "_max"] = max(worst.get(key + "_max", 0.0), e2)
        assert e1 < tol and e2 < tol, (key, e1, e2)

    for e in range(n):
        r = edges[e]
        assert (r["i"], r["j"]) == tuple(int(v) for v in g[f"e{e}_ij"]), (e, r["i"], r["j"], g[f"e{e}_ij"])
        assert bool(r["accepted"]) == bool(g[f"e{e}_accepted"]), (e, r["conf"], float(g["thres"]))          # decisions identical
        note("pose", r["pose"], g[f"e{e}_pose"])
        assert abs(float(r["conf"]) - float(g[f"e{e}_conf"])) < 0.1 * float(g["thres_margin"]), (e, r["conf"], float(g[f"e{e}_conf"]))
        note("pose_conf", np.array([r["conf"]]), np.array([float(g[f"e{e}_conf"])]))
        if not r["accepted"]:
            assert r["confs"] is None and r["intri"] is None and r["depths"] is None
            continue
        note("confs", r["confs"][:, ::sub, ::sub], g[f"e{e}_confs"])
        note("depths", r["depths"][:, ::sub, ::sub], g[f"e{e}_depths"])
        if rand_idx is not None:                                   # off-lattice pixels: every phase of the 16x16 patch / conv tiles
            note("confs_rand", r["confs"].reshape(2, -1)[:, rand_idx], g[f"e{e}_confs_rand"])
            note("depths_rand", r["depths"].reshape(2, -1)[:, rand_idx], g[f"e{e}_depths_rand"])
        note("intri", r["intri"], g[f"e{e}_intri"])
        worst["confs_norm"] = max(worst.get("confs_norm", 0.0), abs(float(np.sqrt((r["confs"].astype(np.float64) ** 2).sum())) / float(g[f"e{e}_confs_l2"]) - 1.0))
        worst["depths_norm"] = max(worst.get("depths_norm", 0.0), abs(float(np.sqrt((r["depths"].astype(np.float64) ** 2).sum())) / float(g[f"e{e}_depths_l2"]) - 1.0))
        for k in range(2):
            want = float(g[f"e{e}_scale"][k])
            got = r["scales"][k]
            assert np.isnan(want) == (got is None or np.isnan(got)), (e, k, want, got)        # the same views get scale edges
            if not np.isnan(want):
                # s = sum(w Di Dj) / sum(w Di Di): with procedural weights the depths have both signs and the numerator cancels
                # (|s| down to 0.06), so the error is judged against the same ratio with |Di Dj| (`scale_abs`, stored by the
                # generator from the reference's tensors) - the magnitude the rounding errors of the maps actually scale with
                sabs = float(g[f"e{e}_scale_abs"][k])
                ref_mag = max(abs(want), sabs)
                es = abs(float(got) - want) / ref_mag
                self_rel = abs(float(got) - want) / abs(want)
                worst["scale"] = max(worst.get("scale", 0.0), es)
                worst["scale_rel_to_itself"] = max(worst.get("scale_rel_to_itself", 0.0), self_rel)
                assert es < tol, ("scale", e, k, got, want, ref_mag)
                # WELL-CONDITIONED scale edges (|s| >= 0.5 x the same ratio without cancellation: every edge of the full-architecture
                # sequences) meet the bar relative to the value ITSELF; only an edge whose numerator cancels by more than half - tiny
                # configuration, random two-signed depths - is exempt from that second assertion
                if abs(want) >= 0.5 * sabs:
                    worst["scale_well_conditioned"] = max(worst.get("scale_well_conditioned", 0.0), self_rel)
                    worst["n_well_conditioned"] = worst.get("n_well_conditioned", 0.0) + 1.0
                    assert self_rel < tol, ("scale relative to itself (well-conditioned edge)", e, k, got, want, sabs)
                else:
                    worst["n_ill_conditioned"] = worst.get("n_ill_conditioned", 0.0) + 1.0
                note("scale_conf", np.array([r["scale_confs"][k]]), np.array([float(g[f"e{e}_scale_conf"][k])]))
    assert worst.get("confs_norm", 0.0) < tol and worst.get("depths_norm", 0.0) < tol, worst
    return worst


# ---------------------------------------------------------------------------------------------------------
# attention: inputs of tests/test_attention_exact.py, the fp64 reference and a numpy model of the kernel's documented arithmetic
# (csrc/attention.h).  Token layout everywhere: q [S, heads, nqt, 64], k / v [S, heads, nkt, 64]; the decoder ("pose") form has
# nqt = nkt = n + 1 with the pose token LAST.  Results are per token, [S, heads, nqt, 64] (attn_rows_to_tokens undoes the row order
# of the debug entry points).
ATT_SCALE_LOG2E = np.float32(0.125) * np.float32(1.44269504088896340736)


def attn_rows_to_tokens(out, form, S, heads, nq):
    """Output rows of sta_debug_attention ([S, nq, heads*64]) / sta_debug_attention_pose ([S*n + S, heads*64]: patch rows sequence-
    major, then the S pose rows) -> [S, heads, nqt, 64]."""
    out = np.asarray(out)
    if form == "plain":
        return out.reshape(S, nq, heads, 64).transpose(0, 2, 1, 3)
    o = np.concatenate([out[:S * nq].reshape(S, nq, heads, 64), out[S * nq:].reshape(S, 1, heads, 64)], 1)
    return o.transpose(0, 2, 1, 3)


def attn_ref64(q, k, v, kv_shift):
    """softmax(q k^T / 8) v in float64, K / V of sequence (s + kv_shift) % S."""
    S = q.shape[0]
    idx = [(s + kv_shift) % S for s in range(S)]
    a = (q.astype(np.float64) @ k[idx].astype(np.float64).transpose(0, 1, 3, 2)) * 0.125
    a -= a.max(-1, keepdims=True)
    p = np.exp(a)
    return (p / p.sum(-1, keepdims=True)) @ v[idx].astype(np.float64)


def _split16(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def attn_model(q, k, v, kv_shift, precision):
    """The documented arithmetic in numpy float32.  f16x3: operands and P as fp16 hi + lo, three products (hi hi + hi lo + lo hi),
    fp32 accumulation, fp32 exp2 softmax, output as hi + lo.  f16: single fp16 roundings of operands, P and output, fp32 row sum of
    the UNROUNDED p.  (Not modelled: the summation order of the MFMAs and the online rescaling, the hardware exp2 - the 4x margin
    of the bounds derived from this model is for those.)"""
    S = q.shape[0]
    idx = [(s + kv_shift) % S for s in range(S)]
    q, k, v = q.astype(np.float32), k[idx].astype(np.float32), v[idx].astype(np.float32)
    split = precision != "f16"
    qh, ql = _split16(q); kh, kl = _split16(k); vh, vl = _split16(v)
    kt = kh.transpose(0, 1, 3, 2)
    s = qh @ kt
    if split:
        s = s + (qh @ kl.transpose(0, 1, 3, 2) + ql @ kt)
    m = (s.max(-1, keepdims=True) * ATT_SCALE_LOG2E).astype(np.float32)                  # the kernel: m = max * scale, p = exp2(fma(s, scale, -m))
    t = (s.astype(np.float64) * np.float64(ATT_SCALE_LOG2E) - m.astype(np.float64)).astype(np.float32)
    p = np.exp2(t).astype(np.float32)
    l = p.sum(-1, keepdims=True, dtype=np.float32)
    ph, pl = _split16(p)
    o = ph @ vh
    if split:
        o = o + (ph @ vl + pl @ vh)
    o = (o * (np.float32(1.0) / l)).astype(np.float32)
    oh, ol = _split16(o)
    return (oh + ol if split else oh).astype(np.float64)


def attn_row_errors(got, ref):
    """got, ref [S, heads, nqt, 64] -> (rel-L2 of every (sequence, query) row over heads x 64 columns [S, nqt], global rel-L2)."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    num = ((got - ref) ** 2).sum((1, 3)); den = (ref ** 2).sum((1, 3))
    return np.sqrt(num / np.maximum(den, 1e-300)), float(np.sqrt(num.sum() / max(den.sum(), 1e-300)))


def attn_tokens(form, nq, nk):
    return (nq, nk) if form == "plain" else (nq + 1, nk + 1)


def attn_gaussian_inputs(form, S, heads, nq, nk, sharp, seed):
    rng = np.random.default_rng(seed)
    nqt, nkt = attn_tokens(form, nq, nk)
    q = (rng.standard_normal((S, heads, nqt, 64)) * sharp).astype(np.float32)
    k = rng.standard_normal((S, heads, nkt, 64)).astype(np.float32)
    v = rng.standard_normal((S, heads, nkt, 64)).astype(np.float32)
    return q, k, v


def attn_ramp_inputs(form, S, heads, nq, nk, pattern, seed):
    """Gaussian q, k, v whose score gets one more term r(key) (k[..., 0] = r, q[..., 0] = 8, so q0 k0 / 8 = r):
    "rise": r = 8 x tile index - the running maximum moves in every key tile, every tile rescales the accumulator;
    "fall": r = -8 x tile index - no score after the first tile reaches the running maximum (Gaussian part: |.| < 4 at these
            sizes), so the wave-uniform alpha == 1 skip is taken on every later tile;
    "peak": r = 12 on the keys of the LAST tile (the tail tile when nk % 64 != 0), in the pose form on the pose key instead."""
    q, k, v = attn_gaussian_inputs(form, S, heads, nq, nk, 0.35, seed)       # Gaussian part of the score: std 0.35
    tile = np.arange(k.shape[2]) // 64
    if pattern == "rise":
        r = 8.0 * tile
    elif pattern == "fall":
        r = -8.0 * tile
    else:
        assert pattern == "peak"
        r = np.zeros(k.shape[2])
        if form == "pose":
            r[nk] = 12.0
        else:
            r[tile == tile[nk - 1]] = 12.0
    if form == "pose" and pattern != "peak":
        r[nk] = r[nk - 1]                # the pose key (folded into the initial state) sits with the last tile
    k[..., 0] = r.astype(np.float32)
    q[..., 0] = 8.0
    return q, k, v


def attn_uniform_inputs(form, S, heads, nq, nk, seed):
    """q = 0: every score is 0, the output is the column mean of V over exactly nk (+ 1 with the pose token) keys.  V: integers
    1024 +- 64, and 2048 at key 0, key nk - 1 and the pose key - fp16-exact, every partial sum below 2^24 (exact in fp32)."""
    rng = np.random.default_rng(seed)
    nqt, nkt = attn_tokens(form, nq, nk)
    q = np.zeros((S, heads, nqt, 64), np.float32)
    k = rng.standard_normal((S, heads, nkt, 64)).astype(np.float32)
    v = (1024 + rng.integers(-64, 65, size=(S, heads, nkt, 64))).astype(np.float32)
    v[:, :, 0] = 2048; v[:, :, nk - 1] = 2048; v[:, :, nkt - 1] = 2048
    return q, k, v


def attn_selection_inputs(form, S, heads, nq, nk, pose_sel, seed):
    """Every query selects exactly one key.  Keys: random +-1 codes in 63 dimensions and a constant 1; query = 64 x [code of key
    pi(query), -63]: raw score 64 (dot - 63) = 0 for the selected key, <= 64 (dot_max - 63) for every other one.  V: integers,
    columns 0..2 = (sequence, head, key).  pi [S, heads, nqt]: a permutation when nq == nk, else a map that hits key 0, key nk - 1
    and the first and last key of every 64-key tile as far as there are queries; pose form: the pose query selects itself
    (pose_sel "self") or a patch key ("patch"), and up to three patch queries select the pose key.
    -> q, k, v, pi, margin (the smallest distance, in log2 units of the softmax, of a non-selected key below the selected one)."""
    rng = np.random.default_rng(seed)
    nqt, nkt = attn_tokens(form, nq, nk)
    code = (rng.integers(0, 2, size=(S, heads, nkt, 63)) * 2 - 1).astype(np.float32)
    k = np.concatenate([code, np.ones((S, heads, nkt, 1), np.float32)], -1)
    forced = [0, nk - 1] + [j for t in range((nk + 63) // 64) for j in (t * 64, min(t * 64 + 63, nk - 1))]
    forced = list(dict.fromkeys(forced))
    pi = np.zeros((S, heads, nqt), np.int64)
    for s in range(S):
        for h in range(heads):
            if nq == nk:
                p = rng.permutation(nk)
            else:
                p = rng.integers(0, nk, size=nq)
                slots = rng.permutation(nq)[:len(forced)]
                p[slots] = forced[:len(slots)]
            if form == "pose":
                free = [i for i in range(nq) if p[i] not in forced] or list(range(nq))
                to_pose = rng.permutation(free)[:3]
                p = np.concatenate([p, [nk if pose_sel == "self" else int(rng.integers(0, nk))]])
                p[to_pose] = nk
            pi[s, h] = p
    q = np.empty((S, heads, nqt, 64), np.float32)
    v = rng.integers(-1024, 1025, size=(S, heads, nkt, 64)).astype(np.float32)
    for s in range(S):
        for h in range(heads):
            q[s, h, :, :63] = 64.0 * code[s, h, pi[s, h]]
            v[s, h, :, 0] = s; v[s, h, :, 1] = h; v[s, h, :, 2] = np.arange(nkt)
    q[..., 63] = -63.0 * 64.0
    # the margin in float64: scores of the non-selected keys (each query's own key row masked out)
    dots = code.astype(np.float64) @ code.astype(np.float64).transpose(0, 1, 3, 2)         # [S, heads, key, key]
    dots[:, :, np.arange(nkt), np.arange(nkt)] = -np.inf
    margin = -64.0 * (dots.max() - 63.0) * float(ATT_SCALE_LOG2E) if nkt > 1 else np.inf
    return q, k, v, pi, margin


# ---------------------------------------------------------------------------------------------------------
# 3x3 convolutions of the DPT head: inputs of tests/test_conv_exact.py, the float64 reference, a model of the documented arithmetic
# and the pixel classes the errors are taken over.  Layout everywhere: x NHWC [n, H, W, Cin], w [Co, Cin, 3, 3] (reference layout),
# residuals and results NHWC [n, Ho, Wo, Co].
def _conv2d(x, w, stride, dtype, device="cpu"):
    """3x3, pad 1, as nine shifted matrix products in `dtype` (the same code for the float64 reference and the float32 model)."""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(device=device, dtype=dtype)
    n, H, W, Cin = xt.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.nn.functional.pad(xt, (0, 0, 1, 1, 1, 1))
    y = torch.zeros((n * Ho * Wo, wt.shape[0]), dtype=dtype, device=device)
    for ky in range(3):
        for kx in range(3):
            a = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride].reshape(n * Ho * Wo, Cin)
            y += a @ wt[:, :, ky, kx].T
    return y.reshape(n, Ho, Wo, -1).cpu().numpy()


def _ref_device():
    import torch
    return "cuda:0" if torch.cuda.is_available() else "cpu"


def conv_ref64(x, w, b, stride=1, relu_in=0, act=0, res=()):
    """act(conv3x3(relu?(x)) + b) + residuals in float64."""
    import torch
    x = np.asarray(x, np.float64)
    y = _conv2d(np.maximum(x, 0.0) if relu_in else x, np.asarray(w, np.float64), stride, torch.float64, _ref_device()) + np.asarray(b, np.float64)
    if act == 2:
        y = np.maximum(y, 0.0)
    for r in res:
        y = y + np.asarray(r, np.float64)
    return y


def conv_model(x, w, b, stride, relu_in, act, res, precision, round_out=True):
    """The documented arithmetic in float32.  f16x3: input, weights and residuals as fp16 hi + lo, three products (hi hi + hi lo +
    lo hi), fp32 accumulation, output as hi + lo; the input ReLU looks at the sign of hi.  f16: single fp16 roundings of input,
    weights, residuals and output.  round_out=False: the fp32 accumulator + bias (+ activation), what the fused tail keeps on chip.
    (Not modelled: the summation order of the MFMAs and of the K slices - the 4x margin of the bounds is for those.)"""
    import torch
    split = precision != "f16"
    xh, xl = _split16(np.asarray(x, np.float32))
    if relu_in:
        neg = xh < 0
        xh = np.where(neg, np.float32(0), xh); xl = np.where(neg, np.float32(0), xl)
    wh, wl = _split16(np.asarray(w, np.float32))
    acc = _conv2d(xh, wh, stride, torch.float32)
    if split:
        acc = acc + (_conv2d(xh, wl, stride, torch.float32) + _conv2d(xl, wh, stride, torch.float32))
    y = (acc + np.asarray(b, np.float32)).astype(np.float32)
    if act == 2:
        y = np.maximum(y, np.float32(0))
    if not round_out:
        return y
    for r in res:
        rh, rl = _split16(np.asarray(r, np.float32))
        y = (y + (rh + rl if split else rh)).astype(np.float32)
    oh, ol = _split16(y)
    return (oh + ol if split else oh).astype(np.float64)


def tail_activations64(pre):
    """pre [..., 4] float64 (x, y, z, c) -> pts [..., 3], conf [...]: pts = xyz expm1(d) / d, conf = 1 + exp(c) (postprocess.py:10-62)."""
    pre = np.asarray(pre, np.float64)
    xyz = pre[..., :3]
    d = np.sqrt((xyz ** 2).sum(-1, keepdims=True))
    return xyz * (np.expm1(d) / np.maximum(d, 1e-8)), 1.0 + np.exp(pre[..., 3])


def tail_ref64(x, w2, b2, w4, b4):
    """The fused DPT tail in float64: head.2 (3x3) + ReLU, head.4 (1x1 128 -> 4), activations."""
    y = conv_ref64(x, w2, b2, 1, 0, 2)
    return tail_activations64(y @ np.asarray(w4, np.float64).T + np.asarray(b4, np.float64))


def tail_model(x, w2, b2, w4, b4, precision):
    """head.2 in the arithmetic of conv_model with the accumulators kept in fp32; relu(acc + b2) and head.4's rows (scaled by a power of
    two into [0.5, 1), which is exact) enter the 128 -> 4 contraction as fp16 hi + lo with three products; fp32 activations."""
    y = conv_model(x, w2, b2, 1, 0, 2, (), precision, round_out=False)
    yh, yl = _split16(y)
    w4 = np.asarray(w4, np.float32)
    sc = np.ldexp(np.float32(1), -np.frexp(np.abs(w4).max(1, keepdims=True))[1]).astype(np.float32)      # as head4_row_scales (sta_api.hip)
    vh, vl = _split16(w4 * sc)
    pre = (yh @ vh.T + (yh @ vl.T + yl @ vh.T)).astype(np.float32) / sc.T + np.asarray(b4, np.float32)
    pre = pre.astype(np.float32)
    xyz = pre[..., :3]
    d = np.sqrt((xyz * xyz).sum(-1, keepdims=True, dtype=np.float32))
    s = (np.expm1(d) / np.maximum(d, np.float32(1e-8))).astype(np.float32)
    return (xyz * s).astype(np.float64), (np.float32(1) + np.exp(pre[..., 3])).astype(np.float64)


def tail_gaussian_inputs(n, H, W, w4scale, seed=41):
    """x [n, H, W, 128], head.2 (w2, b2), head.4 (w4, b4) with head.4 at `w4scale` times its ordinary size."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, H, W, 128)).astype(np.float32)
    w2 = (rng.standard_normal((128, 128, 3, 3)) * 0.03).astype(np.float32)
    b2 = (rng.standard_normal(128) * 0.5).astype(np.float32)
    w4 = (rng.standard_normal((4, 128)) * 0.05 * w4scale).astype(np.float32)
    b4 = (rng.standard_normal(4) * 0.3 * w4scale).astype(np.float32)
    return x, w2, b2, w4, b4


def conv_pixel_classes(n, Ho, Wo, family, bm):
    """{name: bool mask [n, Ho, Wo]} - the small sets of pixels where these kernels go wrong: the four corners, each border, the
    interior, the ragged last tile column / row (family 8: 8 x 32-pixel tiles of one image; None: no tiles; else the last bm-row
    tile of the FLATTENED pixels), the first and last row of every image after the first (tiles that span two images)."""
    yy, xx = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    top, bot, lef, rig = yy == 0, yy == Ho - 1, xx == 0, xx == Wo - 1
    one = {"corner_tl": top & lef, "corner_tr": top & rig, "corner_bl": bot & lef, "corner_br": bot & rig,
           "border_top": top & ~lef & ~rig, "border_bottom": bot & ~lef & ~rig, "border_left": lef & ~top & ~bot,
           "border_right": rig & ~top & ~bot, "interior": ~(top | bot | lef | rig)}
    m = {k: np.broadcast_to(v, (n, Ho, Wo)) for k, v in one.items()}
    if family == 8:
        if Wo % 32:
            m["ragged_tile_column"] = np.broadcast_to(xx >= 32 * ((Wo - 1) // 32), (n, Ho, Wo))
        if Ho % 8:
            m["ragged_tile_row"] = np.broadcast_to(yy >= 8 * ((Ho - 1) // 8), (n, Ho, Wo))
    elif family is not None and (n * Ho * Wo) % bm:
        flat = np.arange(n * Ho * Wo).reshape(n, Ho, Wo)
        m["ragged_last_tile"] = flat >= bm * ((n * Ho * Wo - 1) // bm)
    for i in range(1, n):
        for name, row in (("first_row", top), ("last_row", bot)):
            k = np.zeros((n, Ho, Wo), bool)
            k[i] = row
            m[f"image{i}_{name}"] = k
    return {k: v for k, v in m.items() if v.any()}


def class_errors(got, ref, masks, channel_blocks=True):
    """got, ref [n, Ho, Wo, C] -> {class: rel-L2 over the class}: the pixel classes of `masks`, and every 32-channel block over all
    pixels.  A NaN in a class makes its error NaN."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    e2, r2 = (got - ref) ** 2, ref ** 2
    pe, pr = e2.sum(-1), r2.sum(-1)
    out = {k: float(np.sqrt(pe[m].sum() / max(pr[m].sum(), 1e-300))) for k, m in masks.items()}
    if channel_blocks:
        C = got.shape[-1]
        for c0 in range(0, C, 32):
            out[f"channels_{c0}_{min(c0 + 32, C) - 1}"] = float(np.sqrt(e2[..., c0:c0 + 32].sum() / max(r2[..., c0:c0 + 32].sum(), 1e-300)))
    return out


def worst_class(errs):
    """-> (name, error) of the worst class; a NaN class wins."""
    return max(errs.items(), key=lambda kv: np.inf if np.isnan(kv[1]) else kv[1])


def conv_gaussian_inputs(n, H, W, Cin, Co, stride, nres, seed):
    rng = np.random.default_rng(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = rng.standard_normal((n, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Co, Cin, 3, 3)) * 0.1).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    res = [rng.standard_normal((n, Ho, Wo, Co)).astype(np.float32) for _ in range(nres)]
    return x, w, b, res


CONV_SEL_OFFSET = 40.0       # relu_in cases: subtracted from every second group of four planes, so that the input ReLU clamps


def conv_selection_map(Cin, Co):
    """Output channel co -> (tap, input channel): tap co % 9 of 32-channel block (co // 9) % (Cin / 32), so that with Co >= 9 Cin / 32
    EVERY (tap, input block) pair - every K tile of the loop, e.g. tap 8 of block b next to tap 0 of block b + 1 - is selected by
    some output channel (asserted), on planes of all four kinds."""
    co = np.arange(Co)
    nb = Cin // 32
    tap, blk = co % 9, (co // 9) % nb
    ci = 32 * blk + (7 * co + 3) % 32
    assert Co >= 9 * nb and len(set(zip(tap.tolist(), blk.tolist()))) == 9 * nb, "every (tap, input block) pair must be selected"
    assert set((ci % 4).tolist()) == {0, 1, 2, 3}
    return tap, ci


def conv_selection_inputs(n, H, W, Cin, Co, relu_in):
    """Inputs that carry their own address: plane 4j holds y, 4j + 1 holds x, 4j + 2 the image index, 4j + 3 the group j (all <= 2047:
    one fp16 holds them).  Weights one-hot by conv_selection_map.  -> x, w, tap [Co], ci [Co]."""
    assert max(H, W, n, Cin // 4) <= 2047
    x = np.empty((n, H, W, Cin), np.float32)
    x[..., 0::4] = np.arange(H, dtype=np.float32)[None, :, None, None]
    x[..., 1::4] = np.arange(W, dtype=np.float32)[None, None, :, None]
    x[..., 2::4] = np.arange(n, dtype=np.float32)[:, None, None, None]
    x[..., 3::4] = np.arange(Cin // 4, dtype=np.float32)
    if relu_in:
        g = (np.arange(Cin) // 4) % 2 == 1
        x[..., g] -= np.float32(CONV_SEL_OFFSET)
    tap, ci = conv_selection_map(Cin, Co)
    w = np.zeros((Co, Cin, 3, 3), np.float32)
    w[np.arange(Co), ci, tap // 3, tap % 3] = 1.0
    return x, w, tap, ci


def conv_selection_expected(x, tap, ci, stride, relu_in):
    """The shifted input planes, 0 outside the image (relu_in: of relu(x))."""
    n, H, W, _ = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((n, H + 2, W + 2, x.shape[3]), np.float32)
    xp[:, 1:-1, 1:-1] = np.maximum(x, 0) if relu_in else x
    out = np.empty((n, Ho, Wo, len(tap)), np.float32)
    for t in range(9):
        ky, kx = divmod(t, 3)
        sel = np.nonzero(tap == t)[0]
        out[..., sel] = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride][..., ci[sel]]
    return out


def conv_selection_report(got, want, tap, ci, stride, limit=6):
    """Text naming the first wrong elements: output pixel, channel, the source pixel expected and the value found."""
    bad = np.argwhere(~(got == want))
    names = ("y", "x", "image", "group")
    lines = []
    for i, y, xo, co in bad[:limit]:
        ky, kx = divmod(int(tap[co]), 3)
        kind = names[int(ci[co]) % 4]
        lines.append(f"output (image {i}, y {y}, x {xo}), channel {co}: expected input pixel (image {i}, y {y * stride + ky - 1}, "
                     f"x {xo * stride + kx - 1}) channel {ci[co]} (tap {tap[co]}, a plane of {kind}) = {want[i, y, xo, co]:g}, found {got[i, y, xo, co]:g}"
                     f" (the pixel actually read has {kind} = {got[i, y, xo, co]:g}, + {CONV_SEL_OFFSET:g} on an offset plane)")
    return len(bad), "; ".join(lines)


def conv_integer_inputs(n, H, W, Cin, Co, stride, nres, seed):
    """Small integers whose exact convolution is an integer of magnitude <= 2048 BY CONSTRUCTION: x in [-3, 3], every output channel
    has min(9 Cin, 512) weights of +-1 (the rest 0), bias in [-32, 32], residuals in [-100, 100]: |sum| <= 3 x 512 + 32 + 2 x 100 =
    1768.  fp16 holds every operand and every result, fp32 every partial sum."""
    rng = np.random.default_rng(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    K = 9 * Cin
    x = rng.integers(-3, 4, size=(n, H, W, Cin)).astype(np.float32)
    w = rng.integers(0, 2, size=(Co, K)).astype(np.float32) * 2 - 1
    if K > 512:
        keep = np.argsort(rng.random((Co, K)), axis=1)[:, :512]
        mask = np.zeros((Co, K), bool)
        np.put_along_axis(mask, keep, True, 1)
        w = w * mask
    b = rng.integers(-32, 33, size=Co).astype(np.float32)
    res = [rng.integers(-100, 101, size=(n, Ho, Wo, Co)).astype(np.float32) for _ in range(nres)]
    return x, w.reshape(Co, Cin, 3, 3).astype(np.float32), b, res


# ---------------------------------------------------------------------------------------------------------
# tests/test_split_exact_*.py: the integer sums of tests/split_cases.py on the float64 backends of this file (integer-valued arrays,
# every partial sum below 2^53: exact whatever the order)
def mm64(a, b):
    """a [M, K], b [N, K] integer-valued -> a b^T in float64, on the GPU where there is one."""
    import torch
    d = _ref_device()
    at = torch.from_numpy(np.ascontiguousarray(a)).to(d).double()
    bt = torch.from_numpy(np.ascontiguousarray(b)).to(d).double()
    return (at @ bt.T).cpu().numpy()


def split_conv_terms(ops, stride, lolo=False):
    """The sums of split_cases.conv_expected for the operands of split_cases.conv_operands: I, T1 = x_hi * w_q, T2 = x_q * w_hi
    (, L = x_q * w_q), NHWC float64, of the input after its ReLU."""
    import torch
    import split_cases as SC
    (xh, xq), (wh, wq) = (SC.conv_relu_in(ops["x"]) if ops["relu_in"] else ops["x"]), ops["w"]

    def f(a, w):
        return _conv2d(a.astype(np.float64), w.astype(np.float64), stride, torch.float64, _ref_device())
    t = {"I": f(xh, wh), "T1": f(xh, wq), "T2": f(xq, wh)}
    if lolo:
        t["L"] = f(xq, wq)
    return t


def first_wrong(got, want, hi_only, names, limit=4):
    """-> (count of wrong elements, text naming the first ones: index, got, want, the hi-only value - got == hi-only: a correction
    was dropped; neither: it was misplaced or applied twice)."""
    bad = np.argwhere(~(np.asarray(got, np.float64) == want))
    lines = []
    for ix in bad[:limit]:
        ix = tuple(ix)
        where = ", ".join(f"{n} {i}" for n, i in zip(names, ix))
        lines.append(f"({where}): got {float(got[ix])!r} want {float(want[ix])!r} hi-only {float(hi_only[ix])!r}")
    return len(bad), "; ".join(lines)


# ---------------------------------------------------------------------------------------------------------
# bit-level comparison of the outputs of two runs: tests/test_workspace_gpu.py and tests/test_stream_order_gpu.py
def snapshot(outs):
    """Outputs of a run, detached from the buffers the next run may reuse."""
    import torch
    torch.cuda.synchronize()
    return [(name, t.detach().clone()) for name, t in outs]


def bits(t):
    import torch
    t = t.contiguous().reshape(-1)
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16}
    return t.view(as_int[t.dtype]) if t.dtype in as_int else t


def first_difference(got, ref):
    """None when the two output lists are bit-identical, else text naming the first output that differs and where."""
    import torch
    if [n for n, _ in got] != [n for n, _ in ref]:
        return f"the outputs themselves differ: {[n for n, _ in got]} against {[n for n, _ in ref]}"
    for (name, a), (_n, b) in zip(got, ref):
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"output {name}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
        ne = bits(a) != bits(b)
        if bool(ne.any()):
            flat = int(torch.nonzero(ne)[0])
            idx = tuple(int(v) for v in np.unravel_index(flat, tuple(a.shape))) if a.dim() else ()
            return (f"output {name} {tuple(a.shape)}: {int(ne.sum())} of {ne.numel()} elements differ, first at index {idx}: "
                    f"got {a.contiguous().reshape(-1)[flat].item()!r}, reference {b.contiguous().reshape(-1)[flat].item()!r}")
    return None
