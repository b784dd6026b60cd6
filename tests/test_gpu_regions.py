"""Region-blend compositor on the GPU (libnst_hip region kernels) against the reference's own vectors
(tests/golden/regions.npz from region_blend.py) and, at 1080p, against the CPU oracle (oracle/region_oracle.py).

Bars: hard masks bit-exact where the pattern needs only +,-,*,/,sqrt (grid, fractal, diagonal, voronoi,
concentric); the atan2/sin patterns (radial, spiral, waves) may flip a pixel sitting on a band edge (GPU libm
vs torch's SLEEF, <= 0.05 % of pixels).  Feathered masks 2e-6 absolute (separable vs 2-D conv rounding).
Composites 2e-6 absolute in fp32, uint8 within 1 LSB of the truncated fp32 reference.  Rotation is checked
against the oracle's restatement of cv2.warpAffine only (cv2 absent: parity unpinned).
nst_region_feather is also pinned bit for bit to what it gave before it moved to the blur it shares with the
temporal stage (tests/golden/flow_blur_parent.npz, recorded from the parent commit): no tolerance.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from neuralstyletransferv1_amd import regions as R
from oracle import region_oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import make_golden_flow_blur as MG  # noqa: E402  (the seeded inputs of the recorded cases)

G = np.load(os.path.join(GOLD, "regions.npz"))
with open(os.path.join(GOLD, "regions.json")) as f:
    META = json.load(f)
H, W = META["H"], META["W"]
DEV = torch.device("cuda", 0)
EXACT = {"grid", "fractal", "diagonal", "voronoi", "concentric"}


def gpu_masks(mode, count, seed, feather, h=H, w=W, sizes=None):
    g = R.draw_geometry(h, w, mode, count, seed, sizes)
    m = R.render_masks(g, h, w, feather, DEV)
    torch.cuda.synchronize()
    return g, m.cpu()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("count", [4, 5, 7])
def test_hard_masks_vs_reference(mode, count):
    g, m = gpu_masks(mode, count, 7, 0)
    ref = G[f"masks_{mode}_{count}"]
    diff = int((m.numpy().astype(np.uint8) != ref).sum())
    if g.mode in EXACT:
        assert diff == 0, (g.mode, diff)
    else:
        assert diff <= max(1, ref.size // 2000), (g.mode, diff)


def test_weighted_voronoi_and_feathers_vs_reference():
    _, m = gpu_masks("voronoi", 4, 11, 0, sizes=META["region_sizes"])
    assert np.array_equal(m.numpy().astype(np.uint8), G["masks_voronoi_sized"])
    for mode in ("voronoi", "fractal"):
        _, m = gpu_masks(mode, 4, 3, 6)
        assert np.abs(m.numpy() - G[f"fmasks_{mode}"]).max() <= 2e-6, mode
    _, m = gpu_masks("grid", 4, 1, 20)
    assert np.abs(m.numpy() - G["fmasks_grid_f20"]).max() <= 2e-6


@pytest.mark.parametrize("name", sorted(MG.FEATHER_CASES))
def test_feather_bits_equal_parent_commit(name):
    """nst_region_feather on seeded random planes: 4 x 45x80 with ks = 81 (half-width 40, the widest the entry point
    admits at that height), 2 x 12x300 with ks = 21 (two 256-pixel row tiles, the second partial: the LDS halo across
    the tile edge, for every user of the shared row kernel)."""
    got, ref = MG.gpu_feather(name), np.load(MG.FIXTURE)[name]
    assert got.dtype == np.float32 and got.shape == ref.shape
    same = got.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), f"{name}: {int((~same).sum())} of {same.size} values differ from the parent commit's bits"


def _sources():
    outs = torch.from_numpy(G["src_outputs"])  # [3 models, 3, H, W] in [0,1]
    orig_u8 = torch.from_numpy(G["src_orig_u8"])  # [H, W, 3]
    srcs = [R.Source(outs[i:i + 1].contiguous().to(DEV), "none") for i in range(3)]
    return outs, orig_u8, srcs


def _check(got_f32, got_u8, ref):
    ref = np.asarray(ref, dtype=np.float32)
    assert np.abs(got_f32 - ref).max() <= 2e-6
    ref_u8 = (torch.from_numpy(ref) * 255).to(torch.uint8).permute(1, 2, 0).numpy().astype(np.int16)
    assert np.abs(got_u8.astype(np.int16) - ref_u8).max() <= 1


def _terms(cfgs):
    return [[(mi, w) for mi, w in zip(c.model_indices, c.model_weights)] for c in cfgs]


def test_full_frame_composites_vs_reference():
    outs, orig_u8, srcs = _sources()
    masks = torch.from_numpy(G["comp_masks"]).to(DEV)
    o = orig_u8[None].contiguous().to(DEV)
    single = [[(a, 1.0)] for a in META["comp_assign"]]
    for terms, ref in ((single, G["comp_out"]), (_terms(R.RegionConfig(*c) for c in META["adv_configs"]), G["adv_out"])):
        f = R.composite(srcs, terms, masks, o, out_f32=True)[0].cpu().numpy()
        u = R.composite(srcs, terms, masks, o)[0].cpu().numpy()
        _check(f, u, ref)


def test_scaled_sources_vs_reference():
    outs, orig_u8, srcs = _sources()
    masks = torch.from_numpy(G["comp_masks"]).to(DEV)
    half = [R.Source(R.resized_source(s.y, "none", (H, W), (H // 2, W // 2)), "none") for s in srcs]
    ref_half = torch.nn.functional.interpolate(outs, size=(H // 2, W // 2), mode="bilinear", align_corners=False)
    assert (torch.cat([h.y for h in half]).cpu() - ref_half).abs().max() <= 1e-6
    cf = [R.RegionConfig(*c) for c in META["adv_scaled_configs"]]
    terms = [[((mi if c.scale == 1.0 else 3 + mi), w) for mi, w in zip(c.model_indices, c.model_weights)] for c in cf]
    f = R.composite(srcs + half, terms, masks, None, out_f32=True)[0].cpu().numpy()
    u = R.composite(srcs + half, terms, masks, None)[0].cpu().numpy()
    _check(f, u, G["adv_scaled_out"])


@pytest.mark.parametrize("case", [0, 1, 2])
def test_crops_composite_vs_reference(case):
    outs, orig_u8, _ = _sources()
    c = META["crops"][case]
    _, m = gpu_masks(c["mode"], c["count"], c["seed"], c["feather"])
    assert np.abs(m.numpy() - G[f"crops_{case}_masks"]).max() <= 2e-6
    masks = m.to(DEV)
    boxes = R.mask_bboxes(masks)
    assert [list(b) for b in boxes] == c["bbox"]
    padded = [tuple(b) for b in c["padded"]]
    cf = [R.RegionConfig(*x) for x in c["configs"]]
    anims = R.parse_region_blend_animations("30,triangle", len(cf))
    srcs, terms = [], []
    for k, ((x1, y1, x2, y2), cfg) in enumerate(zip(padded, cf)):
        wts = R.compute_animated_weights(cfg.model_weights, 7, anims[k])
        tl = []
        for mi, w in zip(cfg.model_indices, wts):
            if mi < 0:
                tl.append((-1, w))
                continue
            crop = (outs[mi][:, y1:y2, x1:x2].clone() * 0.9)[None].contiguous()
            srcs.append(R.Source(crop.to(DEV), "none"))
            tl.append((len(srcs) - 1, w))
        terms.append(tl)
    o = orig_u8[None].contiguous().to(DEV) if c["with_orig"] else None
    f = R.composite(srcs, terms, masks, o, boxes=padded, out_f32=True)[0].cpu().numpy()
    u = R.composite(srcs, terms, masks, o, boxes=padded)[0].cpu().numpy()
    _check(f, u, G[f"crops_{case}_out"])


def test_crop_input_matches_interpolate():
    gen = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 256, (2, 70, 90, 3), generator=gen, dtype=torch.uint8)
    box = (7, 5, 71, 63)
    x01 = fr.permute(0, 3, 1, 2).float().div(255)[:, :, 5:63, 7:71]
    same = R.crop_input(fr.to(DEV), box, (58, 64)).cpu()
    assert torch.equal(same, x01)
    small = R.crop_input(fr.to(DEV), box, (29, 32)).cpu()
    ref = torch.nn.functional.interpolate(x01, size=(29, 32), mode="bilinear", align_corners=False)
    assert (small - ref).abs().max() <= 1e-6


def test_rotation_vs_restatement():
    _, m = gpu_masks("voronoi", 5, 3, 4)
    for ang in (2.0, 33.5, -71.0):
        got = R.rotate_planes(m.to(DEV), ang).cpu()
        ref = O.rotate(m, ang)
        assert (got - ref).abs().max() <= 2e-6, ang


@pytest.mark.parametrize("mode", ["voronoi", "spiral", "fractal"])
def test_1080p_chain_vs_oracle(mode):
    """masks + feather 20 + 4-model composite with the original at 1080p, raw imagenet_255 outputs decoded
    on the fly (the reference decodes y/255 then clamps, pipeline.py:1445-1486)."""
    h, w = 1080, 1920
    g = R.draw_geometry(h, w, mode, 6, 5)
    masks = R.render_masks(g, h, w, 20, DEV)
    ref_masks = O.feather(O.masks_from_geometry(g, h, w), 20)
    dm = (masks.cpu() - ref_masks).abs()
    if g.mode in EXACT:
        assert dm.max() <= 2e-6
    else:  # band-edge flips of atan2/sin spread by the feather: a thin set of pixels
        assert float((dm > 2e-6).float().mean()) < 0.01
    gen = torch.Generator().manual_seed(9)
    raw = [torch.rand(1, 3, h, w, generator=gen) * 300 - 20 for _ in range(4)]
    orig_u8 = torch.randint(0, 256, (1, h, w, 3), generator=gen, dtype=torch.uint8)
    cf = R.parse_region_configs(6, 4, "random", "A+B|C|O+D|B:0.3+D:0.7", None, 5, 0.0)
    srcs = [R.Source(r.to(DEV), "imagenet_255") for r in raw]
    got = R.composite(srcs, _terms(cf), masks, orig_u8.to(DEV), out_f32=True)[0].cpu()
    dec = [(r[0] / 255.0).clamp(0, 1) for r in raw]
    ref = O.composite_adv({1.0: dec}, masks.cpu(), cf, orig_u8[0].permute(2, 0, 1).float().div(255), h, w)
    assert (got - ref).abs().max() <= 2e-6
    u8 = R.composite(srcs, _terms(cf), masks, orig_u8.to(DEV))[0].cpu()
    ref_u8 = (ref * 255).to(torch.uint8).permute(1, 2, 0)
    assert (u8.int() - ref_u8.int()).abs().max() <= 1


# ----------------------------------------------------------------------------- CLI (pipeline.main) vs oracle
from PIL import Image  # noqa: E402

from neuralstyletransferv1_amd import pipeline as P  # noqa: E402
from neuralstyletransferv1_amd import synthetic  # noqa: E402
from oracle import nst_oracle as NO  # noqa: E402


def _ckpts(tmp_path, seeds):
    out = []
    for s in seeds:
        sd = synthetic.make_state_dict("johnson", s)
        p = tmp_path / f"j{s}.pth"
        torch.save(sd, p)
        out.append((str(p), sd))
    return out


def _run_dir(tmp_path, frames, argv):
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(f).save(d_in / f"frame_{i + 1:04d}.png")
    assert P.main(["--input_dir", str(d_in), "--output_dir", str(d_out), "--work_dir", str(tmp_path / "w")] + argv) == 0
    return [np.array(Image.open(d_out / f"styled_frame_{i + 1:04d}.png")) for i in range(len(frames))]


def _decoded(sd, x01, preset):
    with torch.no_grad():
        return NO.decode(NO.FORWARDS["johnson"](sd, NO.encode(x01, preset)), preset)


def _close(got, ref, frac=0.002):
    d = np.abs(got.astype(int) - ref.astype(int))
    assert (d > 1).mean() <= frac, f"{(d > 1).mean():.4%} of values differ by > 1 LSB (max {d.max()})"


@pytest.mark.parametrize("variant", ["simple", "advanced", "rotate"])
def test_cli_region_mode_vs_oracle(tmp_path, variant):
    """pipeline.py:1720-1839 (fp32): 3 models styled full frame, composited through the region masks, then the
    LAB EMA (default on) and the save."""
    cks = _ckpts(tmp_path, [0, 5, 9])
    h, w = 72, 96
    frames = synthetic.make_frames(3, h, w, seed=40)
    argv = ["--model", cks[0][0], "--model_b", cks[1][0], "--model_c", cks[2][0], "--io_preset", "imagenet_255",
            "--batch", "2"]
    if variant == "simple":
        mode, count, seed, feather, oc = "voronoi", 5, 3, 6, 0.3
        argv += ["--region_mode", mode, "--region_count", "5", "--region_seed", "3", "--region_feather", "6",
                 "--region_original", "0.3"]
    elif variant == "advanced":
        mode, count, seed, feather, oc = "grid", 3, 8, 8, 0.0  # region_count defaults to 1+B+C+D = 3
        argv += ["--region_mode", mode, "--region_seed", "8", "--region_feather", "8", "--region_blend_spec",
                 "A+B|C|O|B:0.2+C", "--region_scales", "1.0,0.5", "--no-smooth_lightness"]
    else:
        mode, count, seed, feather, oc = "diagonal", 3, None, 10, 0.0
        argv += ["--region_mode", mode, "--region_rotate", "7.5", "--region_feather", "10",
                 "--region_assignment", "sequential"]
        seed = 42  # rotating without a seed: fixed 42 (pipeline.py:1742-1743)
    got = _run_dir(tmp_path, frames, argv)
    base = O.feather(O.masks_from_geometry(R.draw_geometry(h, w, mode, count, seed), h, w), feather)
    ema = NO.LabEMA(variant != "advanced", 0.7)
    for i, fr in enumerate(frames):
        x01 = NO.to_tensor01(fr[None])
        outs = [_decoded(sd, x01, "imagenet_255")[0] for _, sd in cks]
        orig = x01[0]
        if variant == "advanced":
            cf = R.parse_region_configs(count, 3, "random", "A+B|C|O|B:0.2+C", "1.0,0.5", seed, 0.0)
            half = [torch.nn.functional.interpolate(o[None], size=(int(h * 0.5), int(w * 0.5)), mode="bilinear",
                                                    align_corners=False)[0] for o in outs]
            out01 = O.composite_adv({1.0: outs, 0.5: half}, base, cf, orig, h, w)
        else:
            masks = base
            asn = R.assign_models_to_regions(count, 3, "sequential" if variant == "rotate" else "random", None, seed, oc)
            if variant == "rotate":
                masks = O.feather(O.rotate(base, (i + 1) * 7.5), feather // 2)
            cf = [R.RegionConfig([a], [1.0], 1.0) for a in asn]
            out01 = O.composite_adv({1.0: outs}, masks, cf, orig if oc > 0 else None, h, w)
        ref = ema(NO.to_pil_u8(out01[None])[0])
        _close(got[i], ref)


def test_cli_region_optimize_vs_oracle(tmp_path):
    """pipeline.py:1120-1407 (fp32): per-region crops (padding 8) styled by the models of each region's blend,
    scales 1.0 / 0.5, blend animation, composite_from_crops with the original; then the LAB EMA."""
    cks = _ckpts(tmp_path, [1, 6])
    h, w = 80, 112
    frames = synthetic.make_frames(3, h, w, seed=41)
    spec, scales, anim = "A|B|A+B|O+A", "1.0,0.5", "30,triangle"
    got = _run_dir(tmp_path, frames, ["--model", cks[0][0], "--model_b", cks[1][0], "--io_preset", "imagenet_255",
                                      "--region_optimize", "--region_mode", "fractal", "--region_count", "4",
                                      "--region_padding", "8", "--region_blend_spec", spec, "--region_scales", scales,
                                      "--blend_animate", anim, "--region_feather", "6", "--batch", "3"])
    masks = O.feather(O.masks_from_geometry(R.draw_geometry(h, w, "fractal", 4, 42), h, w), 6)
    cf = R.parse_region_configs(masks.shape[0], 2, "random", spec, scales, 42, 0.0)
    boxes = []
    for k in range(masks.shape[0]):
        x1, y1, x2, y2 = O.bbox(masks[k])
        boxes.append((max(0, x1 - 8), max(0, y1 - 8), min(w, x2 + 8), min(h, y2 + 8)))
    anims = R.parse_region_blend_animations(anim, len(cf))
    ema = NO.LabEMA(True, 0.7)
    for i, fr in enumerate(frames):
        x01 = NO.to_tensor01(fr[None])
        styled = {}
        for k, ((x1, y1, x2, y2), c) in enumerate(zip(boxes, cf)):
            crop = x01[:, :, y1:y2, x1:x2]
            ch, cw = y2 - y1, x2 - x1
            if c.scale < 1.0:
                crop = torch.nn.functional.interpolate(crop, size=(max(1, int(ch * c.scale)), max(1, int(cw * c.scale))),
                                                       mode="bilinear", align_corners=False)
            for mi in c.model_indices:
                if mi < 0:
                    continue
                o = _decoded(cks[mi][1], crop, "imagenet_255")
                if c.scale < 1.0:
                    o = torch.nn.functional.interpolate(o, size=(ch, cw), mode="bilinear", align_corners=False)
                styled.setdefault(mi, {})[k] = o[0]
        wts = [R.compute_animated_weights(c.model_weights, i + 1, anims[k]) for k, c in enumerate(cf)]
        out01 = O.composite_crops(styled, boxes, cf, masks, x01[0], h, w, wts)
        _close(got[i], ema(NO.to_pil_u8(out01[None])[0]))


@pytest.mark.parametrize("mode", ["blob", "tentacle", "wave", "pulse"])
@pytest.mark.parametrize("hw", [(45, 80), (270, 480)])
def test_morph_vs_restatement(mode, hw):
    """warp_all_masks_organic on the GPU vs the oracle (numpy noise pinned by the goldens; cv2.remap restated:
    parity unpinned).  float64 libm differences can move a remap coordinate across a 1/32-pixel step: a few
    pixels may differ beyond float rounding."""
    h, w = hw
    _, m = gpu_masks("voronoi", 4, 3, 4, h, w)
    morph = R.MorphAnimation(enabled=True, mode=mode, speed=1.5, amplitude=0.12, frequency=3.0)
    got = R.morph_planes(m.to(DEV), morph, 7).cpu()
    ref = O.morph(m, mode, 1.5, 0.12, 3.0, 42, 7)
    d = (got - ref).abs()
    assert float((d > 2e-6).float().mean()) < 1e-3, (mode, float(d.max()))
    assert torch.allclose(got.sum(0), torch.ones(h, w), atol=1e-5)


def test_cli_region_morph_vs_oracle(tmp_path):
    """--region_morph blob with --region_rotate (standard path): masks rotated then warped then re-feathered
    per frame (region_blend.py:1757-1768)."""
    cks = _ckpts(tmp_path, [2, 7])
    h, w = 64, 96
    frames = synthetic.make_frames(2, h, w, seed=43)
    got = _run_dir(tmp_path, frames, ["--model", cks[0][0], "--model_b", cks[1][0], "--io_preset", "imagenet_255",
                                      "--region_mode", "concentric", "--region_count", "3", "--region_feather", "12",
                                      "--region_rotate", "3", "--region_morph", "1.5,0.1,2.0,blob",
                                      "--region_assignment", "sequential", "--no-smooth_lightness"])
    base = O.feather(O.masks_from_geometry(R.draw_geometry(h, w, "concentric", 3, 42), h, w), 12)
    for i, fr in enumerate(frames):
        x01 = NO.to_tensor01(fr[None])
        outs = [_decoded(sd, x01, "imagenet_255")[0] for _, sd in cks]
        masks = O.feather(O.rotate(base, (i + 1) * 3.0), 6)
        masks = O.feather(O.morph(masks, "blob", 1.5, 0.1, 2.0, 42, i + 1), 5)
        cf = [R.RegionConfig([a], [1.0], 1.0) for a in R.assign_models_to_regions(3, 2, "sequential", None, 42, 0.0)]
        out01 = O.composite_adv({1.0: outs}, masks, cf, None, h, w)
        _close(got[i], NO.to_pil_u8(out01[None])[0], frac=0.01)
