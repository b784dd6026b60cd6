"""nst_multi_model_frames and the multi_model_video CLI on the GPU against tests/multi_model_ref.py: the descriptor
evaluator (the header's arithmetic in numpy float32) and render() (the reference's frame loop).  Every comparison is
np.array_equal.  Sizes: 37x53 (odd: the byte path; the second output frame and every bank image start off a dword
boundary) and 40x56 (the dword path)."""
from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import camera_ref as CR
import multi_model_ref as MR
from neuralstyletransferv1_amd import _lib, multi_model_video as MM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [(37, 53), (40, 56)]
N_BANK = 11
L = MR.LAYOUT


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached banks are read-only


@functools.lru_cache(maxsize=None)
def _bank(h, w, seed=41):
    a = np.random.default_rng(seed).integers(0, 256, (N_BANK, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _random_still(rng, form, scale):
    """form 0: lo < 0 (the original alone), 1: one rung, 2: two rungs, 3: two rungs with lo == hi.  orig_w + style_w =
    scale: above 1 clips at 255, a negative one at 0."""
    ob = float(rng.uniform(0.2, 0.6))
    blend = float(rng.uniform(0.02, 0.98))
    lo = -1 if form == 0 else int(rng.integers(0, N_BANK))
    hi = -1 if form < 2 else (lo if form == 3 else int(rng.integers(0, N_BANK)))
    return dict(orig=int(rng.integers(0, N_BANK)), lo=lo, hi=hi, orig_w=scale * ob, style_w=scale * (1 - ob),
                w_lo=1 - blend, w_hi=blend)


@functools.lru_cache(maxsize=None)
def _descriptors(seed=13):
    """19 frames (three launches of 8, 8 and 3).  The stages cycle at different periods so that, as the asserts below
    say, every combination of (saturation, fade-in, cross-fade none / plain / styled) occurs, with both base kinds, 0,
    1 and 2 overlays and every form of ST in every place; the scale cycle makes sums clip at both ends."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(19):
        scale = (1.0, 1.4, 1.0, -0.3, 0.7)[i % 5]
        styled_base = i % 3 != 0
        n_over = (i // 2) % 3
        fade_in, cross, sat = i % 2 == 1, (i // 2) % 3, (i // 6) % 2 == 1
        if i >= 12:
            n_over, cross, sat = (i + 1) % 3, i % 3, i % 4 < 2
        base = _random_still(rng, i % 4, scale)
        over = [_random_still(rng, (i + k + 1) % 4, (1.0, scale)[k]) for k in range(n_over)]
        blends = [float(rng.uniform(0.02, 0.5)) for _ in range(n_over)]
        t_in, t_x = float(rng.uniform(0, 1)), float(rng.uniform(0, 1))
        d = dict(base_kind=MR.STYLED if styled_base else MR.PLAIN, base=base, n_over=n_over, over=over,
                 keep=[1 - b for b in blends], over_w=blends, sat_on=int(sat), sat=(1.3, 0.6)[i % 2],
                 fin=int(rng.integers(0, N_BANK)) if fade_in else -1, fin_w=(1 - t_in, t_in) if fade_in else (0.0, 0.0),
                 cross_kind=(MR.NONE, MR.PLAIN, MR.STYLED)[cross],
                 next=_random_still(rng, (i + 2) % 4, 1.0) if cross else None,
                 cross_w=(1 - t_x, t_x) if cross else (0.0, 0.0))
        out.append(d)
    combos = {(d["base_kind"], d["n_over"], d["sat_on"], d["fin"] >= 0, d["cross_kind"]) for d in out}
    assert {c[0] for c in combos} == {MR.PLAIN, MR.STYLED} and {c[1] for c in combos} == {0, 1, 2}
    assert {c[2:] for c in combos} >= {(s, f, c) for s in (0, 1) for f in (False, True) for c in (0, 1, 2)}
    forms = lambda s: 0 if s["lo"] < 0 else (1 if s["hi"] < 0 else 2)
    assert {forms(d["base"]) for d in out if d["base_kind"] == MR.STYLED} == {0, 1, 2}
    assert {forms(o) for d in out for o in d["over"]} == {0, 1, 2}
    assert {forms(d["next"]) for d in out if d["cross_kind"] == MR.STYLED} == {0, 1, 2}
    return out


def _read_indices(d):
    """The bank indices a descriptor reads (a plain image: orig alone; lo < 0 / hi < 0: absent)."""
    stills = [(d["base"], d["base_kind"] == MR.STYLED)] + [(o, True) for o in d["over"]]
    if d["cross_kind"] != MR.NONE:
        stills.append((d["next"], d["cross_kind"] == MR.STYLED))
    idx = [d["fin"]] if d["fin"] >= 0 else []
    for s, styled in stills:
        idx.append(s["orig"])
        if styled and s["lo"] >= 0:
            idx += [s["lo"]] + ([s["hi"]] if s["hi"] >= 0 else [])
    return idx


@pytest.mark.parametrize("hw", SIZES)
def test_random_descriptors_byte_exact(hw):
    bank, descs = _bank(*hw), _descriptors()
    got = MM.multi_model_frames(_dev(bank), descs).cpu().numpy()
    assert got.shape == (19,) + hw + (3,)
    for i, d in enumerate(descs):
        want = MR.evaluate(bank, d)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    assert got.min() == 0 and got.max() == 255  # both clips were reached


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("value", [0, 255])
def test_flat_banks(hw, value):
    bank = np.full((N_BANK,) + hw + (3,), value, np.uint8)
    descs = _descriptors()
    got = MM.multi_model_frames(_dev(bank), descs).cpu().numpy()
    for i, d in enumerate(descs):
        assert np.array_equal(got[i], MR.evaluate(bank, d)), i


def _plain(sat_on, sat=1.3):
    return dict(base_kind=MR.PLAIN, base=dict(orig=0, lo=-1, hi=-1, orig_w=0.0, style_w=0.0, w_lo=0.0, w_hi=0.0),
                n_over=0, over=[], keep=[], over_w=[], sat_on=sat_on, sat=sat, fin=-1, fin_w=(0.0, 0.0),
                cross_kind=MR.NONE, next=None, cross_w=(0.0, 0.0))


def test_saturation_over_its_whole_domain():
    """Every (r, g) pair at 8 blues on one 512x1024 frame, passed through unchanged (a plain base, no other stage)
    into the saturation stage: the HSV tables over all of their inputs, at a boost and at a cut."""
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    blues = (0, 1, 63, 127, 128, 200, 254, 255)
    img = np.stack([np.stack([r, g, np.full_like(r, b)], -1) for b in blues]).reshape(512, 1024, 3)
    descs = [_plain(0), _plain(1, 1.3), _plain(1, 0.6)]
    got = MM.multi_model_frames(_dev(img[None]), descs).cpu().numpy()
    assert np.array_equal(got[0], img)
    for i, factor in ((1, 1.3), (2, 0.6)):
        want = MR.adjust_saturation(img, factor)
        assert np.array_equal(got[i], want), (factor, int((got[i] != want).sum()))
    assert not np.array_equal(got[1], got[2]) and not np.array_equal(got[1], img)


def test_refusals():
    lib = _lib.lib()
    INV, SHP = _lib.NST_E_INVALID, _lib.NST_E_SHAPE
    st = _lib.stream_ptr(DEV)
    h, w = 37, 53
    buf = torch.zeros((N_BANK + 12, h, w, 3), dtype=torch.uint8, device=DEV)
    bank, out = buf[:N_BANK], buf[N_BANK:]
    out.fill_(7)
    bp, op = bank.data_ptr(), out.data_ptr()
    good = _descriptors()[:12]

    def call(descs, n=None, n_bank=N_BANK, hh=h, ww=w, b=bp, o=op, arr=True):
        fr = MM.pack(descs) if arr else None
        return lib.nst_multi_model_frames(b, n_bank, hh, ww, fr, len(descs) if n is None else n, o, st)

    def edit(i, fn):
        d = copy.deepcopy(good)
        fn(d[i])
        return d

    assert call(good, n=0) == INV and call(good, n=-1) == INV
    assert call(good, b=None) == INV and call(good, o=None) == INV and call(good, arr=False) == INV
    assert call(good, n_bank=0) == INV
    # an index outside the bank, in the last frame (its launch would be the second): nothing may run
    assert call(edit(11, lambda d: d["base"].update(orig=N_BANK))) == INV
    assert call(edit(11, lambda d: d["base"].update(orig=-1))) == INV
    pick = lambda cond: next(i for i, d in enumerate(good) if cond(d))
    sb = pick(lambda d: d["base_kind"] == MR.STYLED and d["base"]["hi"] >= 0)
    assert call(edit(sb, lambda d: d["base"].update(lo=N_BANK))) == INV
    assert call(edit(sb, lambda d: d["base"].update(hi=N_BANK))) == INV
    ov = pick(lambda d: d["n_over"] == 2 and d["over"][1]["lo"] >= 0)
    assert call(edit(ov, lambda d: d["over"][1].update(lo=N_BANK))) == INV
    assert call(edit(ov, lambda d: d["over"][0].update(orig=-1))) == INV
    fi = pick(lambda d: d["fin"] >= 0)
    assert call(edit(fi, lambda d: d.update(fin=N_BANK))) == INV
    for kind in (MR.PLAIN, MR.STYLED):
        nx = pick(lambda d: d["cross_kind"] == kind)
        assert call(edit(nx, lambda d: d["next"].update(orig=N_BANK))) == INV
    nx = pick(lambda d: d["cross_kind"] == MR.STYLED and d["next"]["lo"] >= 0)
    assert call(edit(nx, lambda d: d["next"].update(lo=N_BANK + 5))) == INV
    assert call(good, n_bank=max(i for d in good for i in _read_indices(d))) == INV
    for bad in (3, -1):
        assert call(edit(3, lambda d: d.update(n_over=bad))) == INV
    for bad in (MR.NONE, 3, -1):
        assert call(edit(3, lambda d: d.update(base_kind=bad))) == INV
    for bad in (3, -1):
        assert call(edit(3, lambda d: d.update(cross_kind=bad, next=d["base"]))) == INV
    # out overlapping the bank: inside it, its last image, and a bank that starts inside out
    fb = h * w * 3
    assert call(good, o=bp) == INV and call(good, o=bp + (N_BANK - 1) * fb) == INV and call(good, o=bp + fb * N_BANK - 1) == INV
    flat = [_plain(0)] * 12
    assert call(flat, b=op + 11 * fb, n_bank=1, o=op) == INV
    for hh, ww in ((0, w), (h, 0), (32769, w), (h, 32769), (-1, w)):
        assert call(good, hh=hh, ww=ww) == SHP
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7 and int(bank.max()) == 0  # no refused call launched anything
    # what a descriptor does not read is not checked: lo and hi of a plain image, an absent stage's fields
    loose = edit(0, lambda d: None)
    pl = pick(lambda d: d["base_kind"] == MR.PLAIN)
    loose[pl]["base"].update(lo=N_BANK + 9, hi=-44)
    assert call(loose) == 0  # and out directly behind the bank is no overlap
    assert call(flat, b=op + 11 * fb, n_bank=1, o=op, n=11) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.NstError, match="no CPU path"):
        MM.multi_model_frames(bank.cpu(), good)


def _save_jpeg(path, w, h, seed):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)
    Image.fromarray(small).resize((w, h), Image.BICUBIC).save(path, format="JPEG", quality=92)


@pytest.mark.parametrize("case,wh,size,want_wh", [
    ("portrait_from_landscape", (64, 50), 48, (48, 37)),
    ("portrait_from_portrait", (40, 60), 48, (48, 72)),
    ("same_size", (48, 37), 48, (48, 37)),
])
def test_load_resize(tmp_path, case, wh, size, want_wh):
    p = tmp_path / f"{case}.jpg"
    _save_jpeg(p, wh[0], wh[1], seed=len(case))
    rgb = np.array(Image.open(p).convert("RGB"), dtype=np.uint8)
    h, w = rgb.shape[:2]
    tw, th = size, int(h * (size / w))
    assert (tw, th) == want_wh == MM.fitted_size(w, h, size)
    want = rgb if (w, h) == (tw, th) else CR.lanczos_resize(rgb, tw, th)
    got = MM.load_resize(p, size, True, DEV)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (th, tw, 3)
    assert np.array_equal(got.cpu().numpy(), want)


def test_cli_end_to_end(tmp_path):
    """LAYOUT through the CLI: originals 64x50 (resampled to 48x37), rungs already 48x37 (copied), against render()
    over the same loads; the file names, the hold repetition, and --jpeg_reader gpu giving the same bytes."""
    dirs = MR.write_layout(tmp_path / "in")
    styled = {k: dirs[k] for k in ("udnie", "mosaic", "tenharmsel")}

    def argv(out, *extra):
        return ["--orig_dir", str(dirs["orig"]), "--styled_udnie", str(dirs["udnie"]), "--styled_mosaic",
                str(dirs["mosaic"]), "--styled_tenharmsel", str(dirs["tenharmsel"]), "--output_dir", str(out),
                "--size", "48", "--fps", str(L["fps"]), "--crossfade_seconds", str(L["crossfade_seconds"]),
                "--hold_frames", str(L["hold_frames"]), "--styled_start", str(L["styled_start"]),
                "--styled_end", str(L["styled_end"]), "--total_frames", str(L["total_frames"]), "--batch", "4", *extra]

    assert MM.main(argv(tmp_path / "out")) == 0
    files = {}
    for key, name, kind in MR.layout_files():
        p = dirs[key] / name
        files[p] = None if kind == "bad" else MM.load_resize(p, 48, True, DEV).cpu().numpy()
    assert {a.shape for a in files.values() if a is not None} == {(37, 48, 3)}
    weights = MM.load_weights({k: str(v) for k, v in styled.items()})
    assert weights == {k: list(v) for k, v in L["weights"].items()}
    want = MR.render(files, dirs["orig"], styled, weights, L["total_frames"], L["styled_start"], L["styled_end"],
                     int(L["crossfade_seconds"] * L["fps"]), L["hold_frames"], 0.4, 1.3)
    assert len(want) == 22
    outs = sorted((tmp_path / "out").iterdir())
    assert [f.name for f in outs] == [f"multi_model_frame_{i:04d}.png" for i in range(1, 23)]
    got = [np.array(Image.open(f)) for f in outs]
    for i, g in enumerate(got):
        assert g.shape == (37, 48, 3) and np.array_equal(g, want[i]), (i, int((g != want[i]).sum()))
    for i in range(0, 22, 2):  # each source frame twice, consecutive numbers
        assert np.array_equal(got[i], got[i + 1])
    assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[6], got[8])
    assert MM.main(argv(tmp_path / "out_gpu", "--jpeg_reader", "gpu")) == 0
    outs_gpu = sorted((tmp_path / "out_gpu").iterdir())
    assert [f.name for f in outs_gpu] == [f.name for f in outs]
    for a, b in zip(outs, outs_gpu):
        assert a.read_bytes() == b.read_bytes(), a.name


@pytest.mark.parametrize("reader", ["pil", "gpu"])
def test_load_bank_scatter(tmp_path, reader):
    """load_bank over three source geometries interleaved (64x50, 48x37, 96x75, 64x50; the two 64x50 files differ), all
    fitting to 48x37: one Lanczos call per geometry, scattered back into bank order.  Expected as test_load_resize
    builds it; the GPU reader on the kind of file test_cli_end_to_end shows it byte-equal to Pillow on."""
    paths, want = [], []
    for i, (w, h, seed) in enumerate([(64, 50, 21), (48, 37, 22), (96, 75, 23), (64, 50, 24)]):
        p = tmp_path / f"f{i}.jpg"
        _save_jpeg(p, w, h, seed)
        rgb = np.array(Image.open(p).convert("RGB"), dtype=np.uint8)
        assert MM.fitted_size(w, h, 48) == (48, 37)
        paths.append(p)
        want.append(rgb if (w, h) == (48, 37) else CR.lanczos_resize(rgb, 48, 37))
    assert not np.array_equal(want[0], want[3])
    got = MM.load_bank(paths, 48, True, DEV, reader)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (4, 37, 48, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack(want))


def test_wrapper_refuses_bank():
    """The shared wrapper's messages carry this wrapper's name."""
    good = _descriptors()[:1]
    with pytest.raises(_lib.NstError, match=r"^multi_model_frames: expected a uint8 \[n_bank,h,w,3\] bank, got torch.float32"):
        MM.multi_model_frames(torch.zeros((N_BANK, 4, 4, 3), dtype=torch.float32, device=DEV), good)
    with pytest.raises(_lib.NstError, match=r"^multi_model_frames: expected a uint8 \[n_bank,h,w,3\] bank, got torch.uint8 \(4, 4, 3\)"):
        MM.multi_model_frames(torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV), good)
    with pytest.raises(_lib.NstError, match=r"^multi_model_frames: expected a uint8 \[n_bank,h,w,3\] bank"):
        MM.multi_model_frames(torch.zeros((N_BANK, 4, 4, 4), dtype=torch.uint8, device=DEV), good)
