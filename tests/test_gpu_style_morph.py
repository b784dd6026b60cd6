"""nst_style_morph_frames and the style_morph CLI on the GPU against tests/style_morph_ref.py: the descriptor
evaluator (the header's arithmetic in numpy float32) and render() (the reference's frame loop).  Every comparison is
np.array_equal.  Sizes: 37x53 (odd: the scalar tail; the second output frame and every bank image start off a dword
boundary) and 40x56 (the dword path)."""
from __future__ import annotations

import ctypes
import functools
import random

import numpy as np
import pytest
import torch
from PIL import Image

import camera_ref as CR
import style_morph_ref as SR
from neuralstyletransferv1_amd import _lib, style_morph as SM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [(37, 53), (40, 56)]
N_BANK = 11


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached banks are read-only


@functools.lru_cache(maxsize=None)
def _bank(h, w, seed=31):
    a = np.random.default_rng(seed).integers(0, 256, (N_BANK, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _random_side(rng, n_terms, scale):
    """orig_w + sum(weight) = scale (about): scale > 1 clips at 255, a negative scale at 0."""
    raw = rng.uniform(0.1, 1.0, n_terms + 1)
    wts = scale * raw / raw.sum()
    terms = []
    for t in range(n_terms):
        lo = int(rng.integers(0, N_BANK))
        kind = (t + n_terms) % 4
        hi = -1 if kind == 0 else (lo if kind == 1 else int(rng.integers(0, N_BANK)))  # one rung / lo == hi / two rungs
        blend = float(rng.uniform(0, 1))
        terms.append(dict(lo=lo, hi=hi, w_lo=1 - blend, w_hi=blend, weight=float(wts[t + 1])))
    return dict(orig=int(rng.integers(0, N_BANK)), orig_w=float(wts[0]), terms=terms)


@functools.lru_cache(maxsize=None)
def _descriptors(seed=7):
    """19 frames (three launches of 8, 8 and 3): n_terms 0, 1, 5 and 8 on either side, one and two sides, the four
    filters mixed, sums that clip at both ends."""
    rng = np.random.default_rng(seed)
    out = []
    counts = (0, 1, 5, 8)
    for i in range(19):
        n_sides = 1 + (i // 4) % 2
        scale = (1.0, 1.3, 0.6, -0.2, 1.0)[i % 5]
        sides = [_random_side(rng, counts[(i + s) % 4], scale) for s in range(n_sides)]
        fade_t = float(rng.uniform(0, 1))
        code, fparam = SM.FILTER_PARAMS[SM.FILTERS[i % 4]]
        out.append(dict(n_sides=n_sides, fade=(1 - fade_t, fade_t) if n_sides == 2 else (1.0, 0.0), sides=sides,
                        filter=code, fparam=fparam))
    assert {len(s["terms"]) for d in out for s in d["sides"]} == {0, 1, 5, 8}
    assert {d["filter"] for d in out[:8]} == {0, 1, 2, 3} and {d["n_sides"] for d in out} == {1, 2}
    return out


@pytest.mark.parametrize("hw", SIZES)
def test_random_descriptors_byte_exact(hw):
    bank, descs = _bank(*hw), _descriptors()
    got = SM.style_morph_frames(_dev(bank), descs).cpu().numpy()
    assert got.shape == (19,) + hw + (3,)
    for i, d in enumerate(descs):
        want = SR.evaluate(bank, d)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    assert got.min() == 0 and got.max() == 255  # both clips were reached


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("value", [0, 255])
def test_flat_banks(hw, value):
    bank = np.full((N_BANK,) + hw + (3,), value, np.uint8)
    descs = _descriptors()
    got = SM.style_morph_frames(_dev(bank), descs).cpu().numpy()
    for i, d in enumerate(descs):
        assert np.array_equal(got[i], SR.evaluate(bank, d)), i


def test_filters_over_their_whole_domain():
    """Every (r, g) pair at 8 blues on one 512x1024 frame, passed through unchanged (orig_w 1, no terms) into each
    filter: the fp32 division of vibrance and the HSV tables over all of their inputs."""
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    blues = (0, 1, 63, 127, 128, 200, 254, 255)
    img = np.stack([np.stack([r, g, np.full_like(r, b)], -1) for b in blues]).reshape(512, 1024, 3)
    descs = []
    for name in SM.FILTERS:
        code, fparam = SM.FILTER_PARAMS[name]
        descs.append(dict(n_sides=1, fade=(1.0, 0.0), sides=[dict(orig=0, orig_w=1.0, terms=[])], filter=code, fparam=fparam))
    got = SM.style_morph_frames(_dev(img[None]), descs).cpu().numpy()
    assert np.array_equal(got[0], img)
    for i, name in enumerate(SM.FILTERS):
        want = SR.FILTERS[name](img)
        assert np.array_equal(got[i], want), (name, int((got[i] != want).sum()))
    assert not np.array_equal(got[1], got[2]) and not np.array_equal(got[1], img)


def test_refusals():
    L = _lib.lib()
    INV, SHP = _lib.NST_E_INVALID, _lib.NST_E_SHAPE
    st = _lib.stream_ptr(DEV)
    h, w = 37, 53
    buf = torch.zeros((N_BANK + 12, h, w, 3), dtype=torch.uint8, device=DEV)
    bank, out = buf[:N_BANK], buf[N_BANK:]
    out.fill_(7)
    bp, op = bank.data_ptr(), out.data_ptr()
    good = _descriptors()[:12]

    def call(descs, n=None, n_bank=N_BANK, hh=h, ww=w, b=bp, o=op, arr=True):
        fr = SM.pack(descs) if arr else None
        return L.nst_style_morph_frames(b, n_bank, hh, ww, fr, len(descs) if n is None else n, o, st)

    def edit(i, fn):
        import copy
        d = copy.deepcopy(good)
        fn(d[i])
        return d

    assert call(good, n=0) == INV and call(good, n=-1) == INV
    assert call(good, b=None) == INV and call(good, o=None) == INV and call(good, arr=False) == INV
    assert call(good, n_bank=0) == INV
    # an index outside the bank, in the last frame (its launch would be the second): nothing may run
    assert call(edit(11, lambda d: d["sides"][0].update(orig=N_BANK))) == INV
    assert call(edit(11, lambda d: d["sides"][0].update(orig=-1))) == INV
    with_terms = next(i for i, d in enumerate(good) if len(d["sides"][0]["terms"]) >= 1)
    assert call(edit(with_terms, lambda d: d["sides"][0]["terms"][0].update(lo=N_BANK))) == INV
    assert call(edit(with_terms, lambda d: d["sides"][0]["terms"][0].update(lo=-1))) == INV
    assert call(edit(with_terms, lambda d: d["sides"][0]["terms"][0].update(hi=N_BANK))) == INV
    assert call(good, n_bank=max(t["lo"] for d in good for s in d["sides"] for t in s["terms"])) == INV
    two = next(i for i, d in enumerate(good) if d["n_sides"] == 2)
    assert call(edit(two, lambda d: d["sides"][1].update(orig=N_BANK))) == INV
    for bad in (0, 3, -1):
        assert call(edit(3, lambda d: d.update(n_sides=bad))) == INV
    for bad in (4, -1):
        assert call(edit(3, lambda d: d.update(filter=bad))) == INV
    fr = SM.pack(good)
    for bad in (_lib.NST_STYLE_MORPH_MAX_STYLES + 1, -1):
        fr[2].side[0].n_terms = bad
        assert L.nst_style_morph_frames(bp, N_BANK, h, w, fr, 12, op, st) == INV
    # out overlapping the bank: inside it, its last image, and a bank that starts inside out
    fb = h * w * 3
    assert call(good, o=bp) == INV and call(good, o=bp + (N_BANK - 1) * fb) == INV and call(good, o=bp + fb * N_BANK - 1) == INV
    flat = [dict(n_sides=1, fade=(1.0, 0.0), sides=[dict(orig=0, orig_w=1.0, terms=[])], filter=0, fparam=(0, 0, 0))] * 12
    assert call(flat, b=op + 11 * fb, n_bank=1, o=op) == INV
    for hh, ww in ((0, w), (h, 0), (32769, w), (h, 32769), (-1, w)):
        assert call(good, hh=hh, ww=ww) == SHP
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7 and int(bank.max()) == 0  # no refused call launched anything
    assert call(good) == 0  # out directly behind the bank is no overlap
    assert call(flat, b=op + 11 * fb, n_bank=1, o=op, n=11) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.NstError, match="no CPU path"):
        SM.style_morph_frames(bank.cpu(), good)


def _save_jpeg(path, w, h, seed):
    rng = np.random.default_rng(seed)
    # smooth content (a random 6x6 grid enlarged) so that the JPEG is an ordinary photograph-like file
    small = rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)
    Image.fromarray(small).resize((w, h), Image.BICUBIC).save(path, format="JPEG", quality=92)


@pytest.mark.parametrize("case,wh,size,portrait,want_wh", [
    ("square_from_landscape", (64, 50), 48, False, (48, 48)),
    ("square_from_portrait", (50, 64), 48, False, (48, 48)),
    ("portrait_mode", (40, 60), 48, True, (32, 48)),
    ("same_size", (48, 48), 48, False, (48, 48)),
    ("same_size_portrait_mode", (32, 48), 48, True, (32, 48)),
])
def test_load_resize(tmp_path, case, wh, size, portrait, want_wh):
    p = tmp_path / f"{case}.jpg"
    _save_jpeg(p, wh[0], wh[1], seed=len(case))
    rgb = np.array(Image.open(p).convert("RGB"), dtype=np.uint8)
    h, w = rgb.shape[:2]
    if not portrait:
        if w > h:
            x = (w - h) // 2
            rgb = rgb[:, x:x + h]
        elif h > w:
            y = (h - w) // 2
            rgb = rgb[y:y + w, :]
        tw = th = size
    else:
        tw, th = int(w * (size / h)), size
    assert (tw, th) == want_wh == SM.fitted_size(w, h, size, portrait)
    want = rgb if rgb.shape[:2] == (th, tw) else CR.lanczos_resize(rgb, tw, th)
    got = SM.load_resize(p, size, portrait, DEV)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (th, tw, 3)
    assert np.array_equal(got.cpu().numpy(), want)


def _write_layout(d):
    """LAYOUT's stills as Pillow JPEGs plus IMG_000 (skipped by default) and junk; originals 64x50 (cropped and
    resampled to 48x48), ladder images already 48x48 (copied)."""
    seed = 100
    for name, fams in (("IMG_000", {"candy": 1}),) + SR.LAYOUT:
        _save_jpeg(d / f"{name}_original.jpg", 64, 50, seed)
        for fam, n in fams.items():
            for style in SM.LADDERS[fam][:n]:
                seed += 1
                _save_jpeg(d / f"{name}_{style}.jpg", 48, 48, seed)
    _save_jpeg(d / "ZZZ_candy.jpg", 48, 48, 1)  # no original
    _save_jpeg(d / "cover.jpg", 48, 48, 2)      # no '_'


def _loaded_layout(d, filters):
    data = []
    for (name, fams), flt in zip(SR.LAYOUT, filters):
        load = lambda style: SM.load_resize(d / f"{name}_{style}.jpg", 48, False, DEV).cpu().numpy()
        data.append(dict(orig=load("original"), ladders={fam: [load(s) for s in SM.LADDERS[fam][:n]] for fam, n in fams.items()},
                         filter=flt))
    return data


@pytest.mark.parametrize("mode", ["fixed", "seeded"])
def test_cli_end_to_end(tmp_path, mode):
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    _write_layout(d_in)
    argv = ["--styled_dir", str(d_in), "--size", "48", "--fps", "4", "--frame_time", "2.0", "--output_dir", str(d_out),
            "--image_ext", "png", "--batch", "5"]
    if mode == "fixed":
        argv += ["--filter", "vibrance"]
        filters = ["vibrance"] * 3
    else:
        argv += ["--seed", "7"]
        rng = random.Random(7)
        filters = [rng.choice(SM.FILTERS) for _ in range(3)]
    assert SM.main(argv) == 0
    files = sorted(d_out.iterdir())
    assert [f.name for f in files] == [f"style_morph_frame_{i:04d}.png" for i in range(1, 13)]
    want = SR.render(_loaded_layout(d_in, filters), 2.0, 4, 0.08)
    assert len(want) == 12
    for i, f in enumerate(files):
        got = np.array(Image.open(f))
        assert got.shape == (48, 48, 3) and np.array_equal(got, want[i]), (i, int((got != want[i]).sum()))


def test_load_bank_scatter(tmp_path):
    """load_bank over three source geometries interleaved (80x60, 48x48, 50x70, 80x60; the two 80x60 files differ):
    one Lanczos call per geometry, scattered back into bank order.  Expected as test_load_resize builds it."""
    files = [("original", 80, 60, 11), ("candy", 48, 48, 12), ("candy_style1e9", 50, 70, 13), ("candy_style5e9", 80, 60, 14)]
    want = []
    for style, w, h, seed in files:
        p = tmp_path / f"IMG_{style}.jpg"
        _save_jpeg(p, w, h, seed)
        rgb = np.array(Image.open(p).convert("RGB"), dtype=np.uint8)
        if w > h:
            x = (w - h) // 2
            rgb = rgb[:, x:x + h]
        elif h > w:
            y = (h - w) // 2
            rgb = rgb[y:y + w, :]
        want.append(rgb if rgb.shape[:2] == (48, 48) else CR.lanczos_resize(rgb, 48, 48))
    assert not np.array_equal(want[0], want[3])
    still = dict(orig=tmp_path / "IMG_original.jpg",
                 ladders={"candy": [tmp_path / f"IMG_{s}.jpg" for s, *_ in files[1:]]})
    needs = [SM.ORIGINAL, ("candy", 0), ("candy", 1), ("candy", 2)]
    got = SM.load_bank(still, needs, 48, False, DEV)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (4, 48, 48, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack(want))


def test_wrapper_refuses_bank():
    """The shared wrapper's messages carry this wrapper's name."""
    good = _descriptors()[:1]
    with pytest.raises(_lib.NstError, match=r"^style_morph_frames: expected a uint8 \[n_bank,h,w,3\] bank, got torch.float32"):
        SM.style_morph_frames(torch.zeros((N_BANK, 4, 4, 3), dtype=torch.float32, device=DEV), good)
    with pytest.raises(_lib.NstError, match=r"^style_morph_frames: expected a uint8 \[n_bank,h,w,3\] bank, got torch.uint8 \(4, 4, 3\)"):
        SM.style_morph_frames(torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV), good)
    with pytest.raises(_lib.NstError, match=r"^style_morph_frames: expected a uint8 \[n_bank,h,w,3\] bank"):
        SM.style_morph_frames(torch.zeros((N_BANK, 4, 4, 4), dtype=torch.uint8, device=DEV), good)
