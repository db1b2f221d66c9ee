"""The SimFeatUp 'resize_conv' upsampler (LayeredResizeConv, sg_jbu kind 3) and the GEMMs' ReLU epilogue on the GPU, and the sharded and
packed pipelines with the 'bilinear' kind: f64 per-element bounds in every precision, the fixture minted from the reference's own module,
the strict checkpoint rule, the drop-in classes against the oracle composed with the restated module, two ranks against one process."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsampler_alt_reference as UR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POTSDAM = os.path.join(ROOT, "configs", "cls_potsdam.txt")
PREC = ["f32", "f16x2", "bf16"]


# ---- ReLU epilogue: sg_op_linear act 3 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("M,N,K", [(300, 136, 67), (2048, 512, 256)])
def test_linear_relu_within_f64_bound(precision, M, N, K):
    from clip_decontamination_amd import _lib
    from clip_decontamination_amd.ops import precision_id, ptr, stream_ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    R = torch.randn(M, N, generator=g)
    dev = torch.device("cuda:0")
    out = torch.full((M, N), float("nan"), device=dev)
    scratch = torch.empty(8 * (M + N) * (K + 64) + 1024, dtype=torch.uint8, device=dev)
    Ad, Wd, bd, Rd = (t.to(dev) for t in (A, W, b, R))
    rc = lib.sg_op_linear(ptr(Ad), ptr(Wd), ptr(bd), ptr(Rd), ptr(out), M, N, K, 3, precision_id(precision), ptr(scratch), scratch.numel(),
                          stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    pre = A.double() @ W.double().T + b.double()
    ref = torch.clamp(pre, min=0) + R.double()
    eps = UR.EPS_OPERAND[precision]
    prod = A.double().abs() @ W.double().abs().T + b.double().abs()
    bound = (2 * eps + UR.gamma(K + 1)) * prod + 2 * UR.U * (ref.abs() + prod)
    err = (out.cpu().double() - ref).abs()
    assert (err <= bound).all(), f"max err/bound {(err / bound).max():.3g}"
    clearly_neg = pre < -bound
    assert clearly_neg.any() and torch.equal(out.cpu()[clearly_neg], R[clearly_neg])      # max(x, 0) then + residual: exactly the residual


def test_linear_refuses_unknown_act():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, 64, device="cuda:0")
    from clip_decontamination_amd.ops import ptr
    assert lib.sg_op_linear(ptr(x), ptr(x), None, None, ptr(x), 64, 64, 64, 4, 0, None, 0, None) != 0


# ---- resize_conv against f64 and the fixture ------------------------------------------------------------------------------------------
def _rc(C, precision="f32", seed=3):
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import get_upsampler
    up = get_upsampler("resize_conv", C, "cuda:0", precision)
    w = Wt.make_resize_conv_weights(C, seed=seed)
    up.load_state_dict(w)
    return up, w


# a statistical check beside the worst-case bound: the bound compounds |W| growth over four stages and is loose in bf16
REL = {"f32": 1e-5, "f16x2": 1e-5, "bf16": 3e-2}


@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("P", [16, 14])
def test_resize_conv_matches_fixture_and_f64(golden, precision, P):
    g = golden("upsampler_alt")
    key = f"resize_conv.g3x4.p{P}"
    src, guid = g["resize_conv.source"], g[key + ".guidance"]
    up, w = _rc(src.shape[1], precision)
    out = up(torch.from_numpy(src).cuda(), torch.from_numpy(guid).cuda()).cpu().numpy()
    assert out.shape == (1, src.shape[1], 48, 64)
    ref, bnd = UR.resize_conv_bound(src, guid, w, precision)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= bnd).all(), f"max err/bound {(err / bnd).max():.3g}"
    assert err.max() <= REL[precision] * np.abs(ref).max()
    fx = g[key + ".out"]
    sub = out[:, :, g[key + ".rows"]][:, :, :, g[key + ".cols"]]
    assert np.abs(sub - fx).max() <= max(REL[precision], 1e-5) * np.abs(fx).max()


@pytest.mark.parametrize("precision", PREC)
def test_resize_conv_wide_within_f64_bound(precision):
    """C = 256 over a 3 x 5 grid, B = 2: the 2-byte GEMMs at K = C + 3 padded to 320, the large-M kernels on the last stages."""
    rng = np.random.default_rng(9)
    C, B, gh, gw = 256, 2, 3, 5
    src = rng.standard_normal((B, C, gh, gw)).astype(np.float32)
    guid = rng.standard_normal((B, 3, 14 * gh, 14 * gw)).astype(np.float32)
    up, w = _rc(C, precision, seed=5)
    out = up(torch.from_numpy(src).cuda(), torch.from_numpy(guid).cuda()).cpu().numpy()
    ref, bnd = UR.resize_conv_bound(src, guid, w, precision)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= bnd).all(), f"max err/bound {(err / bnd).max():.3g}"
    assert err.max() <= REL[precision] * np.abs(ref).max()


def test_resize_conv_repeats_and_logits_refusal():
    up, _ = _rc(64, "bf16")
    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.standard_normal((1, 64, 3, 4)).astype(np.float32)).cuda()
    guid = torch.from_numpy(rng.standard_normal((1, 3, 42, 56)).astype(np.float32)).cuda()
    a, b = up(src, guid), up(src, guid)
    assert torch.equal(a, b)
    assert "resize_conv:gemm_bf16" in up.lib.sg_jbu_last_kernels().decode()
    from clip_decontamination_amd.ops import ptr, stream_ptr
    t = torch.zeros(64, device="cuda:0")
    lg = torch.zeros(1, 1, 48 * 64, device="cuda:0")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    assert up.lib.sg_jbu_logits(up._ctx, ptr(src), ptr(guid), 1, 3, 4, 42, 56, up.precision, ptr(t), 1, None, 0.0, ptr(lg), ptr(ws),
                                ws.numel(), stream_ptr(up.device)) != 0


def test_resize_conv_strict_checkpoint(tmp_path):
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.upsampler import HipJBU
    w = {"upsampler." + k: torch.from_numpy(v) for k, v in Wt.make_resize_conv_weights(32, seed=3).items()}
    good, missing, extra = tmp_path / "good.pth", tmp_path / "missing.pth", tmp_path / "extra.pth"
    torch.save({"state_dict": w}, good)
    torch.save({"state_dict": {k: v for k, v in w.items() if not k.endswith("conv4.bias")}}, missing)
    torch.save({"state_dict": {**w, "upsampler.conv5.bias": torch.zeros(32)}}, extra)
    assert HipJBU.from_config("resize_conv", 32, str(good), "cuda:0").is_resize_conv
    with pytest.raises(RuntimeError, match="missing key"):
        HipJBU.from_config("resize_conv", 32, str(missing), "cuda:0")
    with pytest.raises(RuntimeError, match=r"unexpected key\(s\) \['conv5.bias'\]"):
        HipJBU.from_config("resize_conv", 32, str(extra), "cuda:0")


# ---- drop-in classes with resize_conv against the oracle composed with the restated module ---------------------------------------------
def _torch_resize_conv(w):
    tw = {k: torch.from_numpy(v).double() for k, v in w.items()}

    def up(src, img):
        x = src.double()
        g = img.double()
        for k in range(1, 5):
            big = F.interpolate(x, scale_factor=2, mode="bilinear")
            sg = F.interpolate(g, big.shape[-2:], mode="bilinear")
            y = F.conv2d(torch.cat([big, sg], 1), tw[f"conv{k}.weight"], tw[f"conv{k}.bias"])
            x = big + (F.relu(y) if k < 4 else y)
        return x.float()
    return up


@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
def test_dropin_resize_conv_matches_oracle(cls_name, precision):
    import segmentor, segearth_segmentor
    from clip_decontamination_amd import weights as Wt
    from oracle import segment as OS, vit as OV, jbu as JO
    cfg = Wt.vit_config("tiny-16")
    words, qidx = segmentor.get_cls_idx(POTSDAM)
    text = torch.from_numpy(Wt.make_text_features(len(words), cfg.embed_dim))
    kw = dict(model_type="SegEarth", cls_token_lambda=-0.3, slide_crop=40, slide_stride=24)
    if cls_name == "SegmentorEx":
        kw["global_debias_factor"] = 0.2
    cls = segmentor.SegmentorEx if cls_name == "SegmentorEx" else segearth_segmentor.Segmentor
    seg = cls(clip_type="CLIP", vit_type="tiny-16", name_path=POTSDAM, device=torch.device("cuda:0"), precision=precision, synthetic_ok=True,
              text_features=text, apply_sim_feat_up=True, sim_feat_up_cfg=dict(model_name="resize_conv", model_path=None), **kw)
    img = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, 72, 88), dtype=np.float32))
    oracle = OS.SegOracle(cfg, OV.to_torch(Wt.make_vit_weights(cfg, seed=0)), seg.query_features.cpu(), torch.tensor(qidx),
                          segearth_variant=cls_name == "Segmentor", **kw)
    oracle.jbu_weights = {}
    orig = JO.jbu_forward
    rc = _torch_resize_conv(Wt.make_resize_conv_weights(cfg.embed_dim, seed=3))
    JO.jbu_forward = lambda _w, src, im: rc(src, im)
    try:
        with torch.no_grad():
            ref = oracle.forward_slide(img)
    finally:
        JO.jbu_forward = orig
    got = seg.forward_slide(img.cuda(), [dict(ori_shape=(72, 88))], 24, 40)
    d = (got.cpu() - ref).abs().max().item()
    assert d < (1e-3 if precision != "bf16" else 2e-2), f"max |dlogit| {d:.3g}"


# ---- bilinear: two ranks on one GPU equal one process at patch 14; packed multi-image inference ---------------------------------------
QIDX = [0, 0, 1, 2, 3, 4, 5, 5]


def _pipe(dev="cuda:0"):
    from clip_decontamination_amd import weights as Wt
    from clip_decontamination_amd.engine import HipVisionTower, HipCLIP
    from clip_decontamination_amd.pipeline import SegPipeline
    from clip_decontamination_amd.upsampler import get_upsampler
    cfg = Wt.vit_config("tiny-14")
    tower = HipVisionTower(cfg, Wt.make_vit_weights(cfg, seed=0), precision="f32", device=dev)
    text = torch.from_numpy(Wt.make_text_features(len(QIDX), cfg.embed_dim))
    return SegPipeline(HipCLIP(tower), text, torch.tensor(QIDX), model_type="SegEarth", global_debias_factor=0.2, prob_thd=0.1, bg_idx=5,
                       tiles_per_launch=4, upsampler=get_upsampler("bilinear", cfg.embed_dim, dev, "f32"))


def _scene():
    return torch.from_numpy(np.random.default_rng(11).standard_normal((3, 96, 128), dtype=np.float32))


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pipe = _pipe()
        out = pipe.forward_slide(_scene().cuda(), 24, 40, group="world")
        lab = pipe.segment_scene(_scene().cuda(), 24, 40, group="world")
        torch.cuda.synchronize()
        q.put((rank, out.cpu().numpy(), lab.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_bilinear_two_ranks_equal_one_process_patch14():
    sp = _pipe()
    single = sp.forward_slide(_scene().cuda(), 24, 40).cpu()
    single_lab = sp.segment_scene(_scene().cuda(), 24, 40).cpu()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out, lab in res:
        assert out.shape == tuple(single.shape)
        assert (torch.from_numpy(out) - single).abs().max().item() < 1e-5, f"rank {rank}"
        assert torch.equal(torch.from_numpy(lab), single_lab), f"rank {rank} labels"


def test_bilinear_packed_images_equal_per_image():
    """forward_slide_many (windows of many images in shared launches): f32 results equal forward_slide per image bit for bit."""
    pipe = _pipe()
    rng = np.random.default_rng(4)
    scenes = [torch.from_numpy(rng.standard_normal((3, h, w), dtype=np.float32)).cuda() for h, w in [(64, 96), (48, 48), (80, 56)]]
    many = pipe.forward_slide_many(scenes, 24, 40)
    for sc, m in zip(scenes, many):
        assert torch.equal(m, pipe.forward_slide(sc, 24, 40))
