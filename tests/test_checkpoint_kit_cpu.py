"""CPU: the real-checkpoint acceptance kit of oracle/gen_golden.py end to end on a stand-in checkpoint FILE - torch.save({'model':
procedural tiny weights}) -> `--checkpoint` path -> fixtures - which must be bit-equal to what the generator writes for the same
weights handed over directly, carry the fingerprint of the file, and come with the activation-range table.  The generator's model
is a small weight-dependent stand-in with the reference's module layout and call signatures (below), so the kit's plumbing is
checked without the reference tree; the kit on the reference model itself is `python oracle/check_oracle_vs_ref.py ckpt`."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _standin_reference(cfg, sd):
    """A deterministic stand-in for the reference STA model: the module attributes the generator hooks (enc_blocks, dec_block,
    downstream_head_pts.dpt.{act_postprocess, scratch.layer_rn, scratch.refinenet1..4, head}) and the split entry points it calls
    (_encode_image, _decode_stereo, head_pose_s, head_pts, forward on a views dict).  Every output depends on every weight
    tensor: the patch embedding and decoder_embed are applied as they are, every other module scales by a gain drawn from its
    own tensors.  Loading is strict: a missing or foreign tensor name fails."""
    import torch
    from torch import nn
    from vista_slam_amd import weights as W
    want = set(W.state_dict(cfg, seed=0))
    assert set(sd) == want, (sorted(set(sd) ^ want))[:8]
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()}

    def gain(prefix):
        vals = [v.double().mean() for k, v in t.items() if k.startswith(prefix)]
        assert vals, prefix
        return 1.0 + 0.05 * float(torch.tanh(torch.stack(vals).sum()))

    class Scale(nn.Module):
        def __init__(self, prefix):
            super().__init__()
            self.g = gain(prefix)

        def forward(self, x):
            return x * self.g + 0.01 * torch.tanh(x)

    class Tokens2Map(nn.Module):                         # act_postprocess[i]: tokens [B, N, C] -> map [B, 1, hp, wp]
        def __init__(self, prefix):
            super().__init__()
            self.g = gain(prefix)

        def forward(self, x, hp, wp):
            return (self.g * x.mean(-1)).reshape(x.shape[0], 1, hp, wp)

    pre = "downstream_head_pts.dpt."
    model = nn.Module()
    model.patch_embed = Scale("patch_embed.")
    model.enc_blocks = nn.ModuleList(Scale(f"enc_blocks.{i}.") for i in range(cfg.enc_depth))
    model.dec_block = nn.ModuleList(Scale(f"dec_block.{i}.") for i in range(cfg.dec_depth))
    dpt = nn.Module()
    dpt.act_postprocess = nn.ModuleList(Tokens2Map(f"{pre}act_postprocess.{i}.") for i in range(4))
    dpt.scratch = nn.Module()
    dpt.scratch.layer_rn = nn.ModuleList(Scale(f"{pre}scratch.layer{i + 1}_rn.") for i in range(4))
    for r in (1, 2, 3, 4):
        setattr(dpt.scratch, f"refinenet{r}", Scale(f"{pre}scratch.refinenet{r}."))
    dpt.head = nn.ModuleList([Scale(f"{pre}head.0."), nn.ReLU(), Scale(f"{pre}head.2."), Scale(f"{pre}head.4.")])
    model.downstream_head_pts = nn.Module()
    model.downstream_head_pts.dpt = dpt
    g_pose, g_norm = gain("head_pose_s."), gain("enc_norm.") * gain("dec_norm.") * gain("init_pose_token")
    P = cfg.patch_size

    def encode(img, ts, normalize=False):
        B, _c, H, W_ = img.shape
        x = torch.nn.functional.conv2d(img, t["patch_embed.proj.weight"], t["patch_embed.proj.bias"], stride=P)
        x = model.patch_embed(x.flatten(2).transpose(1, 2))
        for blk in model.enc_blocks:
            x = blk(x)
        yy, xx = torch.meshgrid(torch.arange(H // P), torch.arange(W_ // P), indexing="ij")
        pos = torch.stack([yy.flatten(), xx.flatten()], -1)[None].expand(B, -1, -1).clone()
        return x * g_norm, pos

    def decode(f1, f2, p1, p2):
        def embed(f, p):
            x = f @ t["decoder_embed.weight"].T + t["decoder_embed.bias"]
            tok = x.mean(1, keepdim=True) + 1e-3 * p.double().mean().float()
            return torch.cat([tok, x], 1)
        x1, x2 = embed(f1, p1), embed(f2, p2)
        o1, o2 = [x1], [x2]
        for blk in model.dec_block:
            x1, x2 = blk(x1 + 0.1 * x2.mean(1, keepdim=True)), blk(x2 + 0.1 * x1.mean(1, keepdim=True))
            o1.append(x1); o2.append(x2)
        return o1, o2

    def head_pose_s(tok):
        s = torch.tanh(g_pose * tok.mean(-1))
        pose = torch.eye(4).repeat(tok.shape[0], 1, 1)
        pose[:, :3, 3] = torch.stack([s, 0.5 * s, -s], -1)
        return {"pose": pose, "conf": torch.sigmoid(s)}

    def head_pts(decout, ts):
        H, W_ = (int(v) for v in ts[0])
        hp, wp = H // P, W_ // P
        lay = [dpt.act_postprocess[k](decout[h], hp, wp) for k, h in enumerate(cfg.hooks)]
        lay = [dpt.scratch.layer_rn[k](x) for k, x in enumerate(lay)]
        path = dpt.scratch.refinenet4(lay[3])
        for r in (3, 2, 1):
            path = getattr(dpt.scratch, f"refinenet{r}")(path + lay[r - 1])
        x = path.repeat_interleave(P, 2).repeat_interleave(P, 3)
        x = torch.cat([x, -x, 0.5 * x, x * x], 1)
        for m in dpt.head:
            x = m(x)
        x = x.permute(0, 2, 3, 1)
        return {"pts3d": x[..., :3], "conf": 1.0 + torch.exp(-x[..., 3])}

    def forward(views):
        a, b = views["main_view"], views["neighbor_views"][0]
        fa, pa = encode(a["img"], a["true_shape"])
        fb, pb = encode(b["img"], b["true_shape"])
        d1, d2 = decode(fa, fb, pa, pb)
        res = []
        for f, d in ((fa, d1), (fb, d2)):
            pose = head_pose_s(d[-1][:, 0, :])
            pts = head_pts([f] + [x[:, 1:, :] for x in d], a["true_shape"])
            res.append({"pts3d_pred": pts["pts3d"], "conf": pts["conf"], "relative_pose": pose["pose"], "relative_pose_conf": pose["conf"]})
        return {"main_views": [res[0]], "support_views": [res[1]]}

    model._encode_image, model._decode_stereo, model.head_pose_s, model.head_pts = encode, decode, head_pose_s, head_pts
    model.forward = forward
    return model.eval()


def _standin_slam_utils():
    import types
    import torch

    def estimate_intrinsic_from_pts3d(pcls, confs, shared_intrinsic=True):
        f = (confs * pcls[..., 2].abs()).sum() / confs.sum()
        H, W_ = pcls.shape[1:3]
        return torch.tensor([[float(f), 0.0, W_ / 2.0], [0.0, float(f), H / 2.0], [0.0, 0.0, 1.0]])

    def estimate_scale_with_depth_and_confidence(d, d_other, c, c_other):
        w = c * c_other
        return (w * d * d_other).sum() / (w * d * d).sum()
    return types.SimpleNamespace(estimate_intrinsic_from_pts3d=estimate_intrinsic_from_pts3d,
                                 estimate_scale_with_depth_and_confidence=estimate_scale_with_depth_and_confidence)


def test_checkpoint_mode_reproduces_the_procedural_fixtures(tmp_path, monkeypatch):
    import sys
    import torch
    sys.path.insert(0, ROOT)
    from oracle import gen_golden as GG
    from vista_slam_amd import weights as W
    monkeypatch.setattr(GG, "OUT", str(tmp_path))
    monkeypatch.setattr(GG, "load_reference_model", _standin_reference)
    monkeypatch.setattr(GG, "_ref_slam_utils", _standin_slam_utils)
    sd = W.state_dict(W.TINY, seed=43)
    ck = tmp_path / "tiny_standin.pth"
    torch.save({"model": {k: torch.from_numpy(v.copy()) for k, v in sd.items()}, "epoch": 3}, str(ck))
    # the kit, restricted to its 224x224 forward fixture (+ the range table) ...
    GG.gen_checkpoint(str(ck), tag="ckpttest", cfg=W.TINY, only={"ckpttest_224_b1"})
    # ... and the same case / a short sequence with the weights handed over directly
    GG.run_case(name="direct_224_b1", cfg=W.TINY, H=224, W_=224, B=1, sub=8)
    a, b = np.load(tmp_path / "ckpttest_224_b1.npz"), np.load(tmp_path / "direct_224_b1.npz")
    shared = [k for k in b.files if not k.startswith("meta_")]
    assert len(shared) > 20
    for k in shared:
        assert np.array_equal(a[k], b[k]), k
    assert str(a["ckpt_fingerprint"]) == W.state_dict_fingerprint(sd) and int(a["ckpt_tensors"]) == len(sd)
    assert a["range_enc_absmax"].shape == (W.TINY.enc_depth,) and a["range_dec_absmax"].shape == (W.TINY.dec_depth,)
    assert np.all(a["range_enc_absmax"] > 0) and a["range_dpt_act_absmax"].shape == (4,)
    table = (tmp_path / "ckpttest_ranges.txt").read_text()
    assert "encoder residual stream" in table and "LayerNorm gains" in table
    seq = dict(cfg=W.TINY, H=48, W_=64, nkf=4, neighbor_edge_num=3, loop_edge_num=2, rel_pose_thres=0.75, sub=4)
    GG.gen_seq(name="seq_ck", sd=GG.load_checkpoint_sd(str(ck)), extra={"ckpt_fingerprint": np.array("x")}, **seq)
    GG.gen_seq(name="seq_direct", **seq)
    a, b = np.load(tmp_path / "seq_ck.npz"), np.load(tmp_path / "seq_direct.npz")
    for k in [k for k in b.files if not k.startswith("meta_")]:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_fingerprint_is_order_and_container_independent():
    import sys
    import torch
    sys.path.insert(0, ROOT)
    from vista_slam_amd import weights as W
    sd = W.state_dict(W.TINY, seed=43)
    fp = W.state_dict_fingerprint(sd)
    keys = list(sd)[::-1]
    assert W.state_dict_fingerprint({k: torch.from_numpy(sd[k].copy()) for k in keys}) == fp
    other = dict(sd); k0 = keys[0]; other[k0] = sd[k0] + np.float32(1e-3)
    assert W.state_dict_fingerprint(other) != fp
