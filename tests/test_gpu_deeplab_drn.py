"""sky_swap.py --backbone drn: DeepLab v3+ on DRN-D-54 (output stride 8) on libnst_hip against the reference.

The bars are the ones tests/test_gpu_deeplab.py holds the ResNet network to:
  * tests/golden/deeplab_drn_*.npz hold the REFERENCE module's logits (tests/golden/make_golden_deeplab_drn.py);
    fp32 and fp32s within 1e-4 of max |logit| and the same argmax wherever the reference's top-2 margin exceeds
    1e-4 of max |logit|; bf16 / fp16 within 3e-2 / 5e-3 of max |logit|, the same argmax wherever the margin exceeds
    twice that bar, >= 98 % argmax agreement overall.
  * sizes no golden covers, u8 frames and the 1080p mask chain: against tests/drn_ref.py (pinned bit-exact to the
    goldens by tests/test_deeplab_drn_host.py) and the oracle's Pillow / cv2 restatements, the fp32 bars and masks
    within 1 LSB.
The head (three direct convolutions at full resolution, csrc/seg_drn_head.hip) sees here: extents that are no
multiple of its 64 x 16 / 64 x 8 / 32 x 8 / 32 x 4 tiles (33x47, 54x96, 104x136, 200x296, 144x256: several
workgroups per axis with partial last tiles, odd extents under the stride-2 layer), both input formats, all three
storage types."""
import os

import numpy as np
import pytest
import torch

import drn_ref
from neuralstyletransferv1_amd import deeplab, synthetic
from oracle import deeplab_oracle as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("deeplab_drn_s0_33x47.npz", "deeplab_drn_s101_104x136.npz")
DEV = torch.device("cuda", 0)
LOGIT_REL = {"bf16": 3e-2, "fp16": 5e-3}

_models = {}
_goldens = {}
_refs = {}


def _model(nc, seed, dtype):
    key = (nc, seed)
    if key not in _models:
        m = deeplab.DeepLabDRN(num_classes=nc)
        m.load_state_dict(deeplab.make_state_dict(nc, seed, backbone="drn"))
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.compute_dtype = dtype
    return m


def _golden(case):
    if case not in _goldens:
        _goldens[case] = drn_ref.load_golden(os.path.join(GOLDEN, case))
    return _goldens[case]


def _cpu_sd(m):
    return {k: v.cpu() for k, v in m.state_dict().items()}


def _mask_chain_ref(key, m, frames, ids, resolution, feather):
    """drn_ref's mask chain, computed once per (frames, settings) and shared."""
    if key not in _refs:
        _refs[key] = drn_ref.masks_from_frames(_cpu_sd(m), frames, ids, resolution=resolution, feather_px=feather)
    return _refs[key]


def _margin(y):
    s = np.sort(y, axis=1)
    return s[:, -1] - s[:, -2]


def _check_fp32(y, ref, what):
    assert y.shape == ref.shape
    rel = float(np.abs(y - ref).max() / np.abs(ref).max())
    decided = _margin(ref) > 1e-4 * np.abs(ref).max()
    agree = y.argmax(1) == ref.argmax(1)
    print(what, f"max rel {rel:.2e}, argmax agreement {agree.mean():.6f}, on decided pixels {agree[decided].mean()}")
    assert rel <= 1e-4, rel
    assert agree[decided].all()


@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
@pytest.mark.parametrize("case", CASES)
def test_forward_fp32_vs_reference(case, dtype):
    z = _golden(case)
    m = _model(int(z["num_classes"]), int(z["seed"]), dtype)
    y = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
    _check_fp32(y, z["y"], f"{case} {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_forward_16bit_vs_reference(case, dtype):
    z = _golden(case)
    m = _model(int(z["num_classes"]), int(z["seed"]), dtype)
    y = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
    ref = z["y"]
    rel = float(np.abs(y - ref).max() / np.abs(ref).max())
    agree_px = y.argmax(1) == ref.argmax(1)
    agree = float(agree_px.mean())
    decided = _margin(ref) > 2 * LOGIT_REL[dtype] * np.abs(ref).max()
    print(case, f"{dtype} max rel {rel:.2e}, argmax agreement {agree:.4f}, decided pixels {decided.mean():.4f} "
          f"(agreement there {agree_px[decided].mean():.6f})")
    assert rel <= LOGIT_REL[dtype], rel
    assert agree_px[decided].all()
    assert agree >= 0.98, agree


def test_forward_200x296_vs_restatement():
    """25x37 feature map: ASPP dilation 24 live on both axes, 36 on one; four head workgroups per axis."""
    m = _model(19, 0, "fp32")
    x = torch.randn(1, 3, 200, 296, generator=torch.Generator().manual_seed(17)) * 1.2
    ref = drn_ref.forward(_cpu_sd(m), x).numpy()
    _check_fp32(m(x.to(DEV)).cpu().numpy(), ref, "200x296 fp32")


def test_u8_frames_preprocess_fused():
    """nst_seg_forward on uint8 frames == drn_ref on preprocess_pil(frames) (sky_swap.py:179-183), and the fused
    argmax is the argmax of the returned logits."""
    m = _model(19, 0, "fp32")
    frames = synthetic.make_frames(2, 54, 96, seed=41)
    lg, pred = m.engine(DEV, "fp32").run(torch.from_numpy(frames).to(DEV), logits=True, pred=True)
    sd = _cpu_sd(m)
    for i in range(2):
        ref = drn_ref.forward(sd, D.preprocess_u8(frames[i])).numpy()
        got = lg[i:i + 1].cpu().numpy()
        _check_fp32(got, ref, f"u8 frame {i}")
        assert (pred[i].cpu().numpy() == got[0].argmax(0)).all()


@pytest.mark.parametrize("dtype", ["fp32", "fp32s", "bf16", "fp16"])
def test_forward_deterministic(dtype):
    m = _model(19, 0, dtype)
    x = torch.randn(2, 3, 72, 96, generator=torch.Generator().manual_seed(5)).to(DEV)
    a = m(x)
    b = m(x)
    assert torch.equal(a, b)


MASK_IDS = [8, 11, 18]


@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
def test_mask_engine_1080p_vs_oracle(dtype):
    """MaskEngine, unchanged, on a DeepLabDRN: two 1080p frames at the 256x144 working size against the chain built
    from drn_ref and the oracle's helpers — same class maps wherever the reference's margin is decided, masks within
    1 LSB (the logic of test_gpu_deeplab.py test_mask_engine_1080p_vs_oracle)."""
    m = _model(19, 0, dtype)
    frames = synthetic.make_frames(2, 1080, 1920, seed=21)
    me = deeplab.MaskEngine(m, DEV, resolution=256, dtype=dtype)
    masks, pred = me.masks(torch.from_numpy(frames).to(DEV), MASK_IDS, feather_px=3, return_pred=True)
    masks, pred = masks.cpu().numpy(), pred.cpu().numpy()
    ref_m, ref_p, ref_lg = _mask_chain_ref("1080p", m, frames, MASK_IDS, 256, 3)
    assert pred.shape == ref_p.shape == (2, 144, 256)
    decided = _margin(ref_lg) > 1e-4 * np.abs(ref_lg).max()
    assert (pred == ref_p)[decided].all()
    if (pred == ref_p).all():
        d = np.abs(masks.astype(int) - ref_m.astype(int))
        print("mask max |d|", d.max(), "pixels off", (d > 0).mean(), "mask mean", ref_m.mean())
        assert d.max() <= 1
    else:  # a near-tie flipped a class: compare the masks made from the GPU's own class maps
        print("near-tie flips:", int((pred != ref_p).sum()))
        for i in range(2):
            mm = D.cv_resize_linear_u8(D.infer_post(pred[i], MASK_IDS, 0, 0, 3), 1920, 1080)
            assert np.abs(masks[i].astype(int) - mm.astype(int)).max() <= 1


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mask_engine_1080p_16bit_report(dtype):
    """The same 1080p mask program in the 16-bit modes.  The class maps are held to the logit bars' logic; the share
    of mask pixels within 1 LSB is printed, not asserted (DESIGN.md records it: ResNet's 0.95 / 0.985 floors were
    measured for ResNet)."""
    m = _model(19, 0, dtype)
    frames = synthetic.make_frames(2, 1080, 1920, seed=21)
    me = deeplab.MaskEngine(m, DEV, resolution=256, dtype=dtype)
    masks, pred = me.masks(torch.from_numpy(frames).to(DEV), MASK_IDS, feather_px=3, return_pred=True)
    masks, pred = masks.cpu().numpy(), pred.cpu().numpy()
    ref_m, ref_p, ref_lg = _mask_chain_ref("1080p", m, frames, MASK_IDS, 256, 3)
    decided = _margin(ref_lg) > 2 * LOGIT_REL[dtype] * np.abs(ref_lg).max()
    agree = pred == ref_p
    d = np.abs(masks.astype(int) - ref_m.astype(int))
    print(f"drn {dtype} 1080p: class agreement {agree.mean():.5f}, decided {decided.mean():.4f}; mask within 1 LSB "
          f"{(d <= 1).mean():.5f}, max {d.max()}")
    assert agree[decided].all()


def test_sky_swap_cli_batch_frames_drn(tmp_path):
    """sky_swap.py --backbone drn --batch_frames (frame_####.png -> mask_####.png) against the drn_ref chain."""
    from PIL import Image

    from neuralstyletransferv1_amd import sky_swap
    sd = deeplab.make_state_dict(19, 0, backbone="drn")
    ck = tmp_path / "deeplab-drn.pth.tar"
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "epoch": 1}, ck)
    fdir = tmp_path / "frames"
    fdir.mkdir()
    frames = synthetic.make_frames(3, 90, 160, seed=5)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(fdir / f"frame_{i + 1:04d}.png")
    rc = sky_swap.main(["--batch_frames", str(fdir), "--weights", str(ck), "--backbone", "drn", "--target_labels",
                        "vegetation,person", "--resolution", "64", "--mask_feather", "2", "--dtype", "fp32"])
    assert rc == 0
    ref_m, _, _ = drn_ref.masks_from_frames(sd, frames, [8, 11], resolution=64, feather_px=2)
    for i in range(3):
        got = np.array(Image.open(tmp_path / "masks" / f"mask_{i + 1:04d}.png"))
        assert got.shape == (90, 160)
        assert np.abs(got.astype(int) - ref_m[i].astype(int)).max() <= 1


def test_missing_or_misshaped_tensor_is_named():
    """nst_seg_create_ex names the first DRN tensor it cannot use (head, bottleneck and conv-layer lookups)."""
    sd = {k: v for k, v in _model(19, 0, "fp32").state_dict().items()}
    for key, bad in (("backbone.layer0.0.weight", None), ("backbone.layer7.1.running_var", None),
                     ("backbone.layer5.0.downsample.0.weight", torch.zeros(1024, 512, 3, 3))):
        broken = dict(sd)
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(deeplab.NstError, match=key.replace(".", r"\.")):
            deeplab.SegEngine(broken, 19, "fp32", DEV, backbone="drn")
    with pytest.raises(deeplab.NstError, match="backbone"):
        deeplab.SegEngine(sd, 19, "fp32", DEV, backbone="xception")


def test_resnet_and_drn_engines_side_by_side():
    """One process, one engine of each backbone, run alternately (twice each): each still matches its golden — no
    workspace plan, split-K dry run or cache shared between the two programs."""
    zr = np.load(os.path.join(GOLDEN, "deeplab_s0_33x47.npz"))
    zd = _golden(CASES[0])
    res = deeplab.DeepLab(num_classes=int(zr["num_classes"]))
    res.load_state_dict(deeplab.make_state_dict(int(zr["num_classes"]), int(zr["seed"])))
    res = res.eval().to(DEV)
    drn = _model(int(zd["num_classes"]), int(zd["seed"]), "fp32")
    xr, xd = torch.from_numpy(zr["x"]).to(DEV), torch.from_numpy(zd["x"]).to(DEV)
    for rnd in range(2):
        _check_fp32(res(xr).cpu().numpy(), zr["y"], f"resnet round {rnd}")
        _check_fp32(drn(xd).cpu().numpy(), zd["y"], f"drn round {rnd}")
