"""nst_blob_masks, nst_blob_frames, nst_add_weighted_u8 and the selfstyle_blob CLI on the GPU against tests/blob_ref.py.

sin and exp come from three maths libraries here (numpy's float32 ones, float64 rounded once, the GPU's), so equality
has two forms.  Masks: max |gpu - ref_numpy| <= 4 * max |ref_numpy - ref_double| + 2**-22, the right-hand side from
the two CPU variants alone (the factor 4: a library up to about 2 ulp where the two CPU ones are within about 1).
Frames: every byte within 1 of the reference and at most 1e-3 of a case's bytes different (the two CPU variants differ
in at most 7e-6 of the bytes on these shapes, a +-2 ulp library in at most 1.6e-4; a wrong phase, blob order, linspace
denominator, summation order or index changes far more).  A case is one call: one shape, blob count and feather, 9
frames.  With one blob no library is in the way (e = 1, w = 1 / (1 + 1e-6f)): byte-exact.

Shapes, the smallest that reach each path: 37x50 (h*w % 4 != 0: the byte path, runs that straddle rows), 36x52 (the
dword path), 1x7 and 7x1 (linspace of one element; at w = 1 a run covers four rows).  9 frames per call cross the
8-frame launch group.  The stills are random bytes, so a wrong index shows.

Measured on the MI355X: masks at most 1.79e-6 from the numpy variant where the bound is 4.29e-6 (37x50,
3 blobs, T = 0.1); frames at most one byte of a case's 49,950 different, by one grey level.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from PIL import Image

import blob_ref as BR
import morph_ref
from neuralstyletransferv1_amd import _lib, selfstyle_blob as SB

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SHAPES = [(37, 50), (36, 52), (1, 7), (7, 1)]
FRAME_IDX = (0, 1, 17, 360, 719, 2, 100, 500, 718)
BLOBS = (1, 2, 3, 8)
FEATHERS = (0.0, 0.15, 0.3)
N_BANK = 7
FREQ, SPEED, SEED = 2.5, 1.0, 42


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached arrays are read-only


@functools.lru_cache(maxsize=None)
def _bank(h, w):
    a = np.random.default_rng(97).integers(0, 256, (N_BANK, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref_masks(h, w, nb, feather):
    """(numpy variant, double variant), each float32 [9, nb, h, w]; computed once, shared, read-only."""
    out = []
    for libm in ("numpy", "double"):
        a = np.stack([BR.soft_masks(h, w, i, nb, FREQ, SPEED, SEED, feather, libm) for i in FRAME_IDX])
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _descs(nb):
    """9 descriptors: the time terms of FRAME_IDX, per blob two random stills and a random cross-fade (the first
    frame: blend 0, the second: lo == hi)."""
    rng = np.random.default_rng(5 + nb)
    out = []
    for k, i in enumerate(FRAME_IDX):
        d = SB.frame_times(i, SPEED)
        blobs = []
        for b in range(nb):
            lo, hi = (int(v) for v in rng.integers(0, N_BANK, 2))
            blend = 0.0 if k == 0 else float(rng.uniform(0, 1))
            blobs.append(dict(lo=lo, hi=lo if k == 1 else hi, w_lo=1 - blend, w_hi=blend))
        d["blobs"] = blobs
        out.append(d)
    return out


def _ref_frames(bank, descs, masks):
    out = []
    for d, m in zip(descs, masks):
        imgs = [morph_ref.add_weighted(bank[s["lo"]], s["w_lo"], bank[s["hi"]], s["w_hi"]) for s in d["blobs"]]
        out.append(BR.blend_frame(imgs, m))
    return np.stack(out)


def _gpu_frames(bank_t, h, w, nb, feather, descs):
    yn, xn = SB.norm_tables(h, w, DEV)
    return SB.blob_frames(bank_t, yn, xn, SB.field(nb, FREQ, SEED, feather), descs).cpu().numpy()


def _frame_condition(got, want, tag):
    d = np.abs(got.astype(int) - want.astype(int))
    share = float((d > 0).mean())
    print(f"frames {tag}: max |d| {int(d.max())}, differing share {share:.3e} ({int((d > 0).sum())} of {d.size})")
    assert d.max() <= 1, tag
    assert share <= 1e-3, tag


@pytest.mark.parametrize("nb", BLOBS)
@pytest.mark.parametrize("hw", SHAPES)
def test_masks(hw, nb):
    h, w = hw
    yn, xn = SB.norm_tables(h, w, DEV)
    times = [SB.frame_times(i, SPEED) for i in FRAME_IDX]
    for feather in FEATHERS:
        ref, ref_d = _ref_masks(h, w, nb, feather)
        got = SB.blob_masks(h, w, yn, xn, SB.field(nb, FREQ, SEED, feather), times).cpu().numpy()
        assert got.shape == ref.shape and got.dtype == np.float32
        bound = 4 * float(np.abs(ref - ref_d).max()) + 2.0 ** -22
        err = float(np.abs(got - ref).max())
        sums = float(np.abs(got.sum(axis=1, dtype=np.float64) - 1).max())
        print(f"masks {h}x{w} nb {nb} feather {feather}: max |gpu - ref| {err:.3e}, bound {bound:.3e}, |sum - 1| {sums:.3e}")
        assert err <= bound, (hw, nb, feather, err, bound)
        assert sums <= 1e-5, (hw, nb, feather, sums)


@pytest.mark.parametrize("nb", BLOBS[1:])
@pytest.mark.parametrize("hw", SHAPES)
def test_frames(hw, nb):
    h, w = hw
    bank, descs = _bank(h, w), _descs(nb)
    bank_t = _dev(bank)
    for feather in FEATHERS:
        want = _ref_frames(bank, descs, _ref_masks(h, w, nb, feather)[0])
        got = _gpu_frames(bank_t, h, w, nb, feather, descs)
        assert got.shape == want.shape
        _frame_condition(got, want, f"{h}x{w} nb {nb} feather {feather}")


@pytest.mark.parametrize("hw", SHAPES)
def test_one_blob_is_byte_exact(hw):
    h, w = hw
    bank, descs = _bank(h, w), _descs(1)
    for feather in FEATHERS:
        masks = _ref_masks(h, w, 1, feather)[0]
        assert np.all(masks == np.float32(1) / (np.float32(1) + np.float32(1e-6)))
        want = _ref_frames(bank, descs, masks)
        got = _gpu_frames(_dev(bank), h, w, 1, feather, descs)
        assert np.array_equal(got, want), (hw, feather, int((got != want).sum()))
        gm = SB.blob_masks(h, w, *SB.norm_tables(h, w, DEV), SB.field(1, FREQ, SEED, feather),
                           [SB.frame_times(i, SPEED) for i in FRAME_IDX]).cpu().numpy()
        assert np.array_equal(gm, masks)
    assert not np.array_equal(want[0], bank[descs[0]["blobs"][0]["lo"]])  # w < 1 truncates every byte above 0 down


def test_dword_path_equals_byte_path():
    """36x52 through an aligned bank (the dword path) and through a view one byte into a buffer (the byte path)."""
    h, w = 36, 52
    bank = _bank(h, w)
    aligned = _dev(bank)
    buf = torch.empty(bank.size + 1, dtype=torch.uint8, device=DEV)
    shifted = buf[1:].view(bank.shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    for nb, feather in ((3, 0.15), (8, 0.0)):
        a = _gpu_frames(aligned, h, w, nb, feather, _descs(nb))
        b = _gpu_frames(shifted, h, w, nb, feather, _descs(nb))
        assert np.array_equal(a, b), (nb, feather)


def test_add_weighted_u8_byte_exact():
    """Every (a, b) pair of bytes: at 0.5 / 0.5 (half of the sums are ties: half-to-even), at a cross-fade, at weights
    that saturate at both ends; then an odd length from an odd address (the byte path and the tail)."""
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    ta, tb = _dev(a), _dev(b)
    for wa, wb in ((0.5, 0.5), (0.3, 0.7), (1 - 0.37, 0.37), (1.0, 0.0), (1.5, 0.25), (-0.5, 0.25)):
        got = SB.add_weighted_u8(ta, wa, tb, wb).cpu().numpy()
        want = morph_ref.add_weighted(a, wa, b, wb)
        assert np.array_equal(got, want), (wa, wb, int((got != want).sum()))
    ties = SB.add_weighted_u8(ta, 0.5, tb, 0.5).cpu().numpy()
    assert ties[1, 2] == 2 and ties[2, 3] == 2 and ties[3, 4] == 4  # 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    n = 4099
    buf_a = torch.empty(n + 1, dtype=torch.uint8, device=DEV)
    buf_b = torch.empty(n + 3, dtype=torch.uint8, device=DEV)
    va, vb = buf_a[1:], buf_b[3:]
    va.copy_(ta.view(-1)[:n])
    vb.copy_(tb.view(-1)[5:5 + n])
    assert va.data_ptr() % 4 == 1 and vb.data_ptr() % 4 == 3
    got = SB.add_weighted_u8(va, 0.5, vb, 0.5).cpu().numpy()
    assert np.array_equal(got, morph_ref.add_weighted(a.reshape(-1)[:n], 0.5, b.reshape(-1)[5:5 + n], 0.5))


def _message():
    return _lib.lib().nst_last_error().decode()


def test_refusals():
    lib = _lib.lib()
    INV, SHP = _lib.NST_E_INVALID, _lib.NST_E_SHAPE
    st = _lib.stream_ptr(DEV)
    h, w, nb = 37, 50, 3
    buf = torch.zeros((N_BANK + 9, h, w, 3), dtype=torch.uint8, device=DEV)
    bank, out = buf[:N_BANK], buf[N_BANK:]
    out.fill_(7)
    mout = torch.full((9, nb, h, w), 7.0, dtype=torch.float32, device=DEV)
    yn, xn = SB.norm_tables(h, w, DEV)
    good, fd = _descs(nb), SB.field(nb, FREQ, SEED, 0.15)
    bp, op, yp, xp = bank.data_ptr(), out.data_ptr(), yn.data_ptr(), xn.data_ptr()

    def frames(descs=good, n=None, n_bank=N_BANK, hh=h, ww=w, b=bp, o=op, y=yp, x=xp, f=fd, arr=True):
        return lib.nst_blob_frames(b, n_bank, hh, ww, y, x, SB.pack_field(f) if f is not None else None,
                                   SB.pack(descs) if arr else None, len(descs) if n is None else n, o, st)

    def masks(descs=good, n=None, hh=h, ww=w, o=mout.data_ptr(), y=yp, x=xp, f=fd, arr=True):
        return lib.nst_blob_masks(hh, ww, y, x, SB.pack_field(f) if f is not None else None,
                                  SB.pack(descs) if arr else None, len(descs) if n is None else n, o, st)

    def edit(i, b, **kw):
        d = [dict(x, blobs=[dict(s) for s in x["blobs"]]) for x in good]
        d[i]["blobs"][b].update(kw)
        return d

    args = "nst_blob_frames: invalid arguments (bank, frames, out non-null; n >= 1; n_bank >= 1)"
    for rc in (frames(n=0), frames(n=-1), frames(b=None), frames(o=None), frames(arr=False), frames(n_bank=0)):
        assert rc == INV and _message() == args
    for rc in (frames(y=None), frames(x=None), frames(f=None)):
        assert rc == INV and _message() == "nst_blob_frames: invalid arguments (yn, xn, field non-null)"
    for bad in (0, 9, -1):
        assert frames(f=dict(fd, n_blobs=bad)) == INV and _message() == f"nst_blob_frames: n_blobs {bad} outside 1..8"
        assert masks(f=dict(fd, n_blobs=bad)) == INV and _message() == f"nst_blob_masks: n_blobs {bad} outside 1..8"
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert frames(f=dict(fd, T=bad)) == INV and _message() == "nst_blob_frames: T must be finite and > 0"
        assert masks(f=dict(fd, T=bad)) == INV and _message() == "nst_blob_masks: T must be finite and > 0"
    # an index outside the bank, in the last frame (its launch would be the second): nothing may run
    for kw in (dict(lo=N_BANK), dict(lo=-1), dict(hi=N_BANK), dict(hi=-1)):
        assert frames(edit(8, 2, **kw)) == INV
        assert _message() == f"nst_blob_frames: frame 8: a bank index outside 0..{N_BANK - 1}"
    assert frames(n_bank=max(max(s["lo"], s["hi"]) for d in good for s in d["blobs"])) == INV
    fb = h * w * 3
    for o in (bp, bp + (N_BANK - 1) * fb, bp + N_BANK * fb - 1):
        assert frames(o=o) == INV and _message() == "nst_blob_frames: out overlaps the bank"
    assert frames(b=op + 8 * fb, n_bank=1, o=op, descs=[dict(d, blobs=[dict(lo=0, hi=0, w_lo=1.0, w_hi=0.0)] * nb)
                                                         for d in good]) == INV
    for hh, ww in ((0, w), (h, 0), (32769, w), (h, 32769), (-1, w)):
        assert frames(hh=hh, ww=ww) == SHP and _message() == f"nst_blob_frames: frame {ww}x{hh} outside 1..32768"
        assert masks(hh=hh, ww=ww) == SHP and _message() == f"nst_blob_masks: frame {ww}x{hh} outside 1..32768"
    for rc in (masks(n=0), masks(o=None), masks(arr=False)):
        assert rc == INV and _message() == "nst_blob_masks: invalid arguments (frames, out non-null; n >= 1)"
    for rc in (masks(y=None), masks(x=None), masks(f=None)):
        assert rc == INV and _message() == "nst_blob_masks: invalid arguments (yn, xn, field non-null)"
    # nst_add_weighted_u8
    aw = lambda a, b, n, o: lib.nst_add_weighted_u8(a, 0.5, b, 0.5, n, o, st)
    for rc in (aw(None, bp, fb, op), aw(bp, None, fb, op), aw(bp, bp + fb, fb, None), aw(bp, bp + fb, 0, op)):
        assert rc == INV and _message().startswith("nst_add_weighted_u8: invalid arguments")
    for rc in (aw(bp, bp + fb, fb, bp), aw(bp, bp + fb, fb, bp + 2 * fb - 1), aw(op, bp, fb, op + fb - 1)):
        assert rc == INV and _message() == "nst_add_weighted_u8: out overlaps an input"
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7 and int(bank.max()) == 0  # no refused call launched anything
    assert float(mout.min()) == 7.0 and float(mout.max()) == 7.0
    # what a call does not read is not checked: the stills of blobs past n_blobs; out directly behind the bank is fine
    loose = [dict(d, blobs=d["blobs"] + [dict(lo=N_BANK + 9, hi=-4, w_lo=0.0, w_hi=0.0)]) for d in good]
    assert frames(loose) == 0 and masks(loose) == 0
    assert aw(bp, bp + fb, fb, bp + 2 * fb) == 0
    torch.cuda.synchronize()
    assert int(out.max()) == 0 and abs(float(mout.sum()) / (9 * h * w) - 1) < 1e-4
    with pytest.raises(_lib.NstError, match="no CPU path"):
        SB.blob_frames(bank.cpu(), yn, xn, fd, good)
    with pytest.raises(_lib.NstError, match=r"^blob_frames: expected a contiguous float32 \[50\] xn"):
        SB.blob_frames(bank, yn, yn, fd, good)


def _save_jpeg(path, w, h, seed):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (5, 4, 3), dtype=np.uint8)
    Image.fromarray(small).resize((w, h), Image.BICUBIC).save(path, format="JPEG", quality=92)


def _load(p):
    return np.array(Image.open(p).convert("RGB"), dtype=np.uint8)


def test_cli_end_to_end(tmp_path):
    """Six 20x28 stills (written out of (tile, overlap) order) and a 40x56 original through the CLI at 3 blobs, 6
    frames, --max_resolution 24 (16x24 output): the file names and the count, the pixels against blob_ref.render over
    the same Pillow decodes; then the same with a second directory for the odd blob."""
    styled_dir, magenta_dir = tmp_path / "styled", tmp_path / "magenta"
    styled_dir.mkdir()
    magenta_dir.mkdir()
    configs = [(256, 32), (256, 85), (288, 36), (320, 40), (96, 16), (1024, 128)]
    for k, (tile, ov) in enumerate(configs):
        _save_jpeg(styled_dir / f"img_tile{tile}_overlap{ov}.jpg", 20, 28, 300 + k)
    for k, (tile, ov) in enumerate(configs[:3]):
        _save_jpeg(magenta_dir / f"img_tile{tile}_overlap{ov}.jpg", 20, 28, 400 + k)
    (styled_dir / "img_original.jpg").write_bytes((styled_dir / "img_tile96_overlap16.jpg").read_bytes())  # not a still
    original = tmp_path / "img.jpg"
    _save_jpeg(original, 40, 56, 500)
    order = sorted(configs)
    styled = [_load(styled_dir / f"img_tile{t}_overlap{o}.jpg") for t, o in order]
    magenta = [_load(magenta_dir / f"img_tile{t}_overlap{o}.jpg") for t, o in sorted(configs[:3])]
    assert [BR.sort_key(p) for p in SB.find_stills(styled_dir)] == order and order[0] == (96, 16)
    for tag, extra, mg in (("plain", [], None), ("mixed", ["--magenta_dir", str(magenta_dir)], magenta)):
        out = tmp_path / f"out_{tag}"
        argv = ["--styled_dir", str(styled_dir), "--original", str(original), "--output_dir", str(out), "--fps", "2",
                "--duration", "3", "--num_blobs", "3", "--max_resolution", "24", "--batch", "4", *extra]
        assert SB.main(argv) == 0
        files = sorted(out.iterdir())
        assert [f.name for f in files] == [f"blob_frame_{i:04d}.png" for i in range(1, 7)]
        got = np.stack([np.array(Image.open(f)) for f in files])
        want = np.stack(BR.render(styled, _load(original), mg, fps=2, duration=3, num_blobs=3, max_resolution=24))
        assert got.shape == want.shape == (6, 24, 16, 3)
        _frame_condition(got, want, f"cli {tag}")
        assert not np.array_equal(got[0], got[1])
    a, b = (np.array(Image.open(tmp_path / f"out_{t}" / "blob_frame_0003.png")) for t in ("plain", "mixed"))
    assert not np.array_equal(a, b)  # the odd blob walks through the other stills
