"""Optical-flow morph on the GPU (csrc/morph_ops.hip, the Gaussian-window Farneback of csrc/flow_ops.hip,
neuralstyletransferv1_amd/morph.py) against the numpy restatement tests/morph_ref.py, and end to end through the CLI.
cv2 is not installed here: parity with OpenCV itself is unpinned for every test below; the yardstick is the
restatement, which tests/test_morph_host.py pins to closed forms and properties.

Bars: the box path of nst_flow_farneback_ex is bit-identical to nst_flow_farneback (the same code since the two
Farneback implementations became one, so at n = 1 that compares the code with itself: what pins those bits is
test_gpu_flow.test_farneback_bits_equal_parent_commit; at n = 2 it still says that a pair in a batch equals the pair
alone); grey, pre-blur and every morph frame byte-exact (integer weights, fp32 products and sums without contraction: nothing to tolerate); the flow
post-processing within 1e-5 * max(1, |v|) away from the 2-px threshold; the Gaussian-window flow see
test_gaussian_flow_vs_restatement."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import morph_ref as MR
from neuralstyletransferv1_amd import _lib, morph as MO, synthetic, temporal as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G = _lib.NST_FLOW_GAUSSIAN


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_box_path_equals_farneback_bit_for_bit():
    prev, nxt = MR.texture_pair(72, 96, 3, -2)
    one = T.farneback(_dev(prev), _dev(nxt)).cpu().numpy()
    ex = MO.farneback_ex(_dev(prev[None]), _dev(nxt[None]), T.FARNEBACK, 0).cpu().numpy()
    assert ex.shape == (1, 72, 96, 2)
    assert np.array_equal(ex[0].view(np.uint32), one.view(np.uint32))
    # two pairs in the same launches: each equals its own single run
    two = MO.farneback_ex(_dev(np.stack([prev, nxt])), _dev(np.stack([nxt, prev])), T.FARNEBACK, 0).cpu().numpy()
    back = T.farneback(_dev(nxt), _dev(prev)).cpu().numpy()
    assert np.array_equal(two[0], one) and np.array_equal(two[1], back)


@functools.lru_cache(maxsize=None)
def _gauss_ref(hw, preset):
    prev, nxt = MR.texture_pair(hw[0], hw[1], 3, -2)
    p = MR.PRESETS[preset]["farneback"]
    ref = np.stack([MR.farneback_gauss(prev, nxt, *p), MR.farneback_gauss(nxt, prev, *p)])
    ref.setflags(write=False)
    return prev, nxt, ref


@pytest.mark.parametrize("preset", ["slideshow", "v2"])
@pytest.mark.parametrize("hw", [(72, 96), (135, 240), (270, 480)])
def test_gaussian_flow_vs_restatement(hw, preset):
    """OPTFLOW_FARNEBACK_GAUSSIAN for n = 2 (forward, and backward with the images swapped) against
    morph_ref.farneback_gauss: 72x96 keeps 1 pyramid level under the 32-pixel rule, 135x240 2, 270x480 3; the
    slideshow parameters run 3 iterations per level, v2's 5 with a 21-pixel window.

    Bar: the box path's, |diff| > 2e-3 px on at most 0.1 % of the pixels (the same operation order in fp32; the
    host exp() of the taps and libm can move a fraction of an ulp through the levels and iterations).
    Measured on an MI355X, all six cases (both pairs each): maximum 0 and 99.9th percentile 0 -- every flow value is
    identical to the restatement's, through v2's 5 iterations on 4 levels too, so no level or step diverges.  The
    bar stays at the box path's: it is the margin for a host whose libm rounds an exp() of the taps differently,
    which moves values by fractions of an ulp, orders of magnitude below 2e-3 px.

    Translation: the interior's median recovers the (3, -2) shift (and its negative for the swapped pair) within
    max(0.05, 2 x 4.5e-4) = 0.05 px, 4.5e-4 px being the restatement's own median error
    (test_morph_host.test_gaussian_window_recovers_a_translation)."""
    prev, nxt, ref = _gauss_ref(hw, preset)
    got = MO.farneback_ex(_dev(np.stack([prev, nxt])), _dev(np.stack([nxt, prev])), MR.PRESETS[preset]["farneback"],
                          G).cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    d = np.abs(got - ref)
    print(hw, preset, f"max |d| {d.max():.3e}, p99.9 {np.quantile(d, 0.999):.3e}, identical {(d == 0).mean():.4f}, "
          f"share > 2e-3 {(d > 2e-3).mean():.2e}")
    assert (d > 2e-3).mean() <= 1e-3, float(d.max())
    bar = max(0.05, 2 * 4.5e-4)
    for k, (sx, sy) in enumerate(((3, -2), (-3, 2))):
        c = got[k][20:-20, 20:-20]
        assert abs(float(np.median(c[..., 0])) - sx) < bar and abs(float(np.median(c[..., 1])) - sy) < bar


def test_gaussian_flow_deep_pyramid_wide_pre_blur():
    """A pyramid whose coarsest level needs a wide pre-blur (the 1080p presets need 77 taps; every size runs the one
    blur with its 511-tap table): 896x900 at pyr_scale 0.19 / 2 levels blurs with round(5 * 13.35) | 1 = 67 taps (the
    smallest frame that passes 63: the coarsest level must keep 32 pixels), 2 iterations to keep the numpy side
    short.  Same bar."""
    par = (0.19, 2, 15, 2, 5, 1.1)
    assert MR.surviving_levels(896, 900, 2, 0.19) == 2
    prev, nxt = MR.texture_pair(896, 900, 3, -2)
    got = MO.farneback_ex(_dev(prev[None]), _dev(nxt[None]), par, G).cpu().numpy()[0]
    d = np.abs(got - MR.farneback_gauss(prev, nxt, *par))
    print("deep pyramid", f"max |d| {d.max():.3e}, p99.9 {np.quantile(d, 0.999):.3e}, identical {(d == 0).mean():.4f}")
    assert (d > 2e-3).mean() <= 1e-3, float(d.max())
    c = got[40:-40, 40:-40]
    assert abs(float(np.median(c[..., 0])) - 3) < 0.05 and abs(float(np.median(c[..., 1])) + 2) < 0.05
    # a pyramid deeper than the table is refused before any launch (the check precedes every use of the pointers)
    rc = _lib.lib().nst_flow_farneback_ex(1, 1, 1, 20000, 20000, 0.5, 9, 15, 3, 7, 1.5, G, 1, 1, 10 ** 15, None)
    assert rc == _lib.NST_E_SHAPE


def test_gray_cv_and_pre_blur_bit_exact():
    fr = synthetic.make_frames(2, 67, 131, seed=4)
    g = MO.gray_cv_u8(_dev(fr))
    got = g.cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], MR.gray_cv(fr[i]))
    rng = np.random.default_rng(8)
    noisy = rng.integers(0, 256, (2, 67, 131), dtype=np.uint8)  # the luma of smooth frames rarely sits on a .5
    for src in (got, noisy):
        b = MO.gauss_u8(_dev(src)).cpu().numpy()
        for i in range(2):
            assert np.array_equal(b[i], MR.pre_blur(src[i])), i


def test_flow_post_vs_restatement():
    flow = MR.post_test_flow(11)  # [2,64,80,2], amplitude +-6: both sides of the 2-px threshold occur
    got = MO.flow_post(_dev(flow), (1.0, -1.0)).cpu().numpy()
    for k, sign in enumerate((1.0, -1.0)):
        ref, mag = MR.flow_post(flow[k], sign)
        assert (mag < 2).mean() > 0.1 and (mag >= 2).mean() > 0.1
        keep = np.abs(mag - 2.0) >= 1e-4
        assert (~keep).mean() <= 1e-3
        err = np.abs(got[k] - ref) / np.maximum(1.0, np.abs(ref))
        print("flow_post", k, "max rel err", float(err[keep].max()), "left out", int((~keep).sum()))
        assert err[keep].max() <= 1e-5
    # the input is left alone (a copy is returned), and the two signs differ where the radial term applies
    assert not np.array_equal(got[0], MO.flow_post(_dev(flow[:1]), (-1.0,)).cpu().numpy()[0])


def _stills(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _flows(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    f = ((rng.random((2, h, w, 2)) - 0.5) * 24).astype(np.float32)  # amplitude +-12
    if kind == "random":
        return f
    if kind == "zero":
        return np.zeros_like(f)
    if kind == "beyond":  # entries larger than the frame: the mirror is crossed more than once
        f[0, ::2, ::3] = (2.5 * w, -1.7 * h)
        f[1, 1::2, ::2] = (-2.25 * w, 2.75 * h)
        f[0, 0, 0] = (7.0 * w, -9.0 * h)  # beyond the [-2w, 3w] clamp too
        return f
    if kind == "nonfinite":
        f[0, 0, 1] = np.nan
        f[0, 1, 2, 0] = np.inf
        f[0, 2, 3, 1] = -np.inf
        f[1, 0, 0] = 1e30
        f[1, 1, 1] = -1e30
        f[1, 2, 2] = (np.nan, 3.0)
        f[1, 2, 4] = (-np.inf, np.inf)
        return f
    if kind == "ties":  # (2m + 1) / 16: at t = 1/4 and 3/4 the map lands exactly on a 1/64-pixel tie of rint(mx * 32)
        m = rng.integers(-40, 40, (2, h, w, 2))
        return ((2 * m + 1) / 16.0).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "zero", "beyond", "nonfinite", "ties"])
@pytest.mark.parametrize("hw", [(40, 56), (3, 5)])
def test_morph_frames_byte_exact(hw, kind):
    """k = 5 frames of both presets' schedules; 40x56 takes the dword-store path (h*w a multiple of 4), 3x5 the byte
    path with a ragged last run."""
    h, w = hw
    a, b = _stills(h, w, 3)
    f = _flows(kind, h, w, 5)
    for preset in ("slideshow", "v2"):
        t, al = MR.schedule(5, preset, "smooth")
        if kind == "ties":
            assert t[1] in (0.25, 0.0625)  # slideshow 1/4 (ties at 1/64), v2 smooth 4 * (1/4)^3 = 1/16
        ref = MR.morph_frames(a, b, f[0], f[1], t, al)
        got = MO.morph_frames(_dev(a), _dev(b), _dev(f[0]), _dev(f[1]), t, al).cpu().numpy()
        assert got.shape == (5, h, w, 3)
        assert np.array_equal(got, ref), (preset, int((got != ref).sum()))
        if kind == "zero":
            assert np.array_equal(got[0], a) and np.array_equal(got[-1], b)
        # the same frames two per launch (the second launch's output starts off a 4-byte boundary for odd sizes)
        got2 = MO.morph_frames(_dev(a), _dev(b), _dev(f[0]), _dev(f[1]), t, al, batch=2).cpu().numpy()
        assert np.array_equal(got2, ref)


def test_morph_frames_single_frame():
    a, b = _stills(40, 56, 9)
    f = _flows("random", 40, 56, 10)
    for preset in ("slideshow", "v2"):
        t, al = MR.schedule(1, preset)
        assert t.tolist() == [0.0]
        got = MO.morph_frames(_dev(a), _dev(b), _dev(f[0]), _dev(f[1]), t, al).cpu().numpy()
        assert got.shape == (1, 40, 56, 3)
        assert np.array_equal(got, MR.morph_frames(a, b, f[0], f[1], t, al))


def test_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    g = torch.zeros((2, 40, 56), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.NstError, match=r"\(-1\).*flags"):
        MO.farneback_ex(g, g, T.FARNEBACK, 1)
    with pytest.raises(_lib.NstError, match=r"\(-1\)"):
        MO.farneback_ex(g, g, (0.5, 3, 14, 3, 5, 1.1), G)  # even window
    with pytest.raises(_lib.NstError, match=r"\(-1\)"):
        MO.farneback_ex(g, g, (0.5, 3, 129, 3, 5, 1.1), G)  # Gaussian window wider than its tap table
    sz = ctypes.c_size_t()
    assert L.nst_flow_scratch_floats_ex(0, 40, 56, ctypes.byref(sz)) == _lib.NST_E_INVALID
    img = torch.zeros((40, 56, 3), dtype=torch.uint8, device=DEV)
    fl = torch.zeros((40, 56, 2), dtype=torch.float32, device=DEV)
    out = torch.zeros((1, 40, 56, 3), dtype=torch.uint8, device=DEV)
    row = (ctypes.c_float * 200)()
    st = _lib.stream_ptr(DEV)
    args = (img.data_ptr(), img.data_ptr(), fl.data_ptr(), fl.data_ptr())
    assert L.nst_morph_frames(*args, 40, 56, 0, row, row, row, row, out.data_ptr(), st) == _lib.NST_E_INVALID
    assert L.nst_morph_frames(*args, 40, 56, 129, row, row, row, row, out.data_ptr(), st) == _lib.NST_E_INVALID
    assert L.nst_morph_frames(*args, 40, 56, 1, None, row, row, row, out.data_ptr(), st) == _lib.NST_E_INVALID
    assert L.nst_morph_frames(*args, 40000, 56, 1, row, row, row, row, out.data_ptr(), st) == _lib.NST_E_SHAPE
    assert L.nst_morph_frames(*args, 40, 0, 1, row, row, row, row, out.data_ptr(), st) == _lib.NST_E_SHAPE
    sg = (ctypes.c_float * 2)(1.0, 0.5)
    assert L.nst_morph_flow_post(fl.data_ptr(), 1, 40, 56, sg, fl.data_ptr(), st) == _lib.NST_E_INVALID  # scratch
    assert L.nst_morph_flow_post(fl.data_ptr(), 2, 20, 56, sg, out.data_ptr(), st) == _lib.NST_E_INVALID  # sign 0.5
    assert L.nst_gauss_u8(g.data_ptr(), 2, 40, 56, g.data_ptr(), st) == _lib.NST_E_INVALID  # in place
    assert L.nst_gray_cv_u8(img.data_ptr(), 0, 40, 56, g.data_ptr(), st) == _lib.NST_E_INVALID
    with pytest.raises(_lib.NstError):
        MO.optical_flow_morph(img, img[:20], 3)
    with pytest.raises(_lib.NstError, match="no CPU path"):
        MO.optical_flow_morph(img.cpu(), img.cpu(), 3)


def test_cli_end_to_end(tmp_path):
    """Three 64x96 stills -> 3 held + 2 x 4 transition + 2 end frames; the held files are the fitted stills, every
    transition file is optical_flow_morph's frame; then the same run through --jpeg_writer gpu for the count."""
    stills = synthetic.make_frames(3, 64, 96, seed=60)
    d_in = tmp_path / "in"
    d_in.mkdir()
    names = ["a.png", "b.png", "c.png"]
    for nm, s in zip(names, stills):
        Image.fromarray(s).save(d_in / nm)
    common = ["--images_dir", str(d_in), "--size", "96x64", "--fps", "4", "--morph_seconds", "1", "--hold_frames", "1",
              "--hold_end", "2", "--preset", "v2"]
    d_out = tmp_path / "out"
    assert MO.main(common + ["--output_dir", str(d_out), "--batch", "3"]) == 0
    files = sorted(d_out.iterdir())
    assert [f.name for f in files] == [f"morph_frame_{i:04d}.png" for i in range(1, 14)]
    assert len(files) == 3 + 8 + 2 == MO.total_frames(3, 4, 1, 2)
    dec = [np.array(Image.open(f)) for f in files]
    fitted = [MO.load_fitted(d_in / nm, 96, 64, DEV) for nm in names]
    for i in range(3):
        assert np.array_equal(fitted[i].cpu().numpy(), stills[i])  # same size: cover + crop is the identity
    assert np.array_equal(dec[0], stills[0]) and np.array_equal(dec[5], stills[1])
    for i in (10, 11, 12):
        assert np.array_equal(dec[i], stills[2])
    for tr, first in ((0, 1), (1, 6)):
        want = MO.optical_flow_morph(fitted[tr], fitted[tr + 1], 4, "v2", "smooth").cpu().numpy()
        for j in range(4):
            assert np.array_equal(dec[first + j], want[j]), (tr, j)
    d_jpg = tmp_path / "out_jpg"
    assert MO.main(common + ["--output_dir", str(d_jpg), "--jpeg_writer", "gpu", "--image_ext", "jpg"]) == 0
    jf = sorted(d_jpg.iterdir())
    assert [f.name for f in jf] == [f"morph_frame_{i:04d}.jpg" for i in range(1, 14)]
    assert Image.open(jf[0]).size == (96, 64)


def test_cli_fits_larger_stills_by_cover_and_crop(tmp_path):
    """Stills of another size and aspect go through the Pillow-exact GPU LANCZOS (cover) and the centre crop."""
    big = synthetic.make_frames(1, 100, 200, seed=61)[0]
    p = tmp_path / "big.png"
    Image.fromarray(big).save(p)
    got = MO.load_fitted(p, 96, 64, DEV).cpu().numpy()
    nw, nh, sx, sy = MO.cover_geometry(200, 100, 96, 64)
    assert (nw, nh, sx, sy) == (128, 64, 16, 0)
    want = np.array(Image.fromarray(big).resize((nw, nh), Image.LANCZOS))[sy:sy + 64, sx:sx + 96]
    assert np.array_equal(got, want)
