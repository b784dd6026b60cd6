"""The camera stage on the GPU (csrc/camera_ops.hip, neuralstyletransferv1_amd/camera.py, the morph CLI's --pan_zoom
path) against the numpy restatement tests/camera_ref.py, which tests/test_camera_host.py pins to closed forms.  cv2 is
not installed here: parity with OpenCV itself is unpinned.

Bar: every comparison is np.array_equal.  The arithmetic is integer fixed point, fp32 without contraction, or double,
so there is nothing to tolerate.

Shapes: 5 x 37 x 53 x 3 frames to a 24 x 16 target (odd sizes: rows are no multiple of 4 bytes, 16 * 24 is, and the
second frame of a launch starts off a dword boundary; five different descriptors in one launch), and 40 x 56 for the
aligned path."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import camera_ref as CR
from neuralstyletransferv1_amd import _lib, camera as CAM, morph as MO, synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TW, TH = 24, 16
SHIFTS = (0.05, 37.3, 180, 359.9, -45)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _frames(h, w, seed=21):
    fr = np.random.default_rng(seed).integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    fr.setflags(write=False)
    return fr


@pytest.mark.parametrize("hw", [(37, 53), (40, 56)])
def test_zoom_pulse_byte_exact(hw):
    h, w = hw
    fr = _frames(h, w)
    sizes = [(w + 2, h + 1), (w, h), (w + 2, h + 1), (w + 9, h + 7), (2 * w, 2 * h)]  # 37x53: (55, 38) and (53, 37)
    got = CAM.zoom_pulse_frames(_dev(fr), sizes).cpu().numpy()
    for i, (nw, nh) in enumerate(sizes):
        assert np.array_equal(got[i], CR.pulse(fr[i], nw, nh)), (i, nw, nh)
    assert np.array_equal(got[1], fr[1])


@pytest.mark.parametrize("hw", [(37, 53), (40, 56)])
def test_rect_subpix_byte_exact(hw):
    h, w = hw
    fr = _frames(h, w)
    cx0, cy0 = (TW - 1) / 2.0, (TH - 1) / 2.0  # the centre of a patch at corner 0
    centres = [(cx0 + 7.3, cy0 + 4.81),             # fractional
               (cx0 + 5.0, cy0 + 7.0),              # integer-aligned: the slice
               (cx0 + (w - TW) + 0.5, cy0 + 3.25),  # ip.x + patch = w, a = 0.5: replicated column
               (cx0 + 2.75, cy0 + (h - TH) + 0.25),  # ip.y + patch = h: replicated row
               (cx0 + (w - TW), cy0 + (h - TH))]    # the far corner, integer
    got = CAM.rect_subpix(_dev(fr), (TW, TH), centres).cpu().numpy()
    for i, (cx, cy) in enumerate(centres):
        assert np.array_equal(got[i], CR.rect_subpix(fr[i], TW, TH, cx, cy)), i
    assert np.array_equal(got[1], fr[1][7:7 + TH, 5:5 + TW])
    # pan end: corner x = w - TW exactly plus the half pixel of the centre formula's float32 (x + tw / 2.0)
    end = [(float(w - TW) + TW / 2.0, float(h - TH) + TH / 2.0)] * 5
    got = CAM.rect_subpix(_dev(fr), (TW, TH), end).cpu().numpy()
    for i in range(5):
        assert np.array_equal(got[i], CR.rect_subpix(fr[i], TW, TH, *end[i])), i
    # full-size patch at corner 0.5: replicated column and row at once
    full = [(w / 2.0, h / 2.0)] * 5
    got = CAM.rect_subpix(_dev(fr), (w, h), full).cpu().numpy()
    assert got.shape == (5, h, w, 3)
    for i in range(5):
        assert np.array_equal(got[i], CR.rect_subpix(fr[i], w, h, *full[i])), i


def test_lanczos_byte_exact():
    fr = _frames(37, 53)
    crops = [(53, 37), (30, 21), (24, 16), (41, 29), (25, 17)]  # (cw, ch), one table slot each
    got = CAM.lanczos_resize(_dev(fr), crops, (TW, TH)).cpu().numpy()
    for i, (cw, ch) in enumerate(crops):
        assert np.array_equal(got[i], CR.lanczos_resize(fr[i][:ch, :cw], TW, TH)), (i, cw, ch)
    assert np.array_equal(got[2], fr[2][:16, :24])  # crop == target
    # extremes drive the negative lobes into the clamps of sat_u8
    hard = np.where(np.random.default_rng(3).random((5, 40, 56, 1)) < 0.5, 0, 255).astype(np.uint8).repeat(3, 3)
    got = CAM.lanczos_resize(_dev(hard), [(56, 40), (55, 39), (33, 22), (25, 40), (56, 17)], (TW, TH)).cpu().numpy()
    for i, (cw, ch) in enumerate([(56, 40), (55, 39), (33, 22), (25, 40), (56, 17)]):
        assert np.array_equal(got[i], CR.lanczos_resize(hard[i][:ch, :cw], TW, TH)), i


@functools.lru_cache(maxsize=None)
def _hue_inputs():
    g = np.arange(256, dtype=np.uint8)
    greys = np.stack([g, g, g], -1).reshape(16, 16, 3)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0],
                     [255, 255, 255], [255, 128, 0], [1, 0, 0], [254, 255, 255], [128, 128, 127]], np.uint8)
    prim = np.tile(prim, (22, 1))[:256].reshape(16, 16, 3)
    rnd = np.random.default_rng(31).integers(0, 256, (3, 16, 16, 3), dtype=np.uint8)
    x = np.concatenate([rnd, greys[None], prim[None]])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("shift", SHIFTS)
def test_hue_shift_byte_exact(shift):
    x = _hue_inputs()
    got = CAM.hue_shift_frames(_dev(x), [shift] * 5).cpu().numpy()
    for i in range(5):
        want = CR.hue_shift(x[i], shift)
        assert np.array_equal(got[i], want), (i, shift, int((got[i] != want).sum()))
    assert np.array_equal(got[3], x[3])  # greys stay
    if abs(shift) < 0.1:
        assert np.array_equal(got, x)


def test_hue_shift_every_colour_class_and_mixed_shifts():
    """All 2^12 colours on a 16-level lattice plus the 255 corner (every max / min ordering, diff and v from 0 to
    255), each frame its own shift."""
    lv = np.array([0, 1, 17, 34, 51, 68, 85, 102, 119, 127, 128, 153, 187, 221, 254, 255], np.uint8)
    cube = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(64, 64, 3)
    x = np.stack([cube] * 5)
    got = CAM.hue_shift_frames(_dev(x), list(SHIFTS)).cpu().numpy()
    for i, s in enumerate(SHIFTS):
        assert np.array_equal(got[i], CR.hue_shift(cube, s)), (s, int((got[i] != CR.hue_shift(cube, s)).sum()))


@pytest.mark.parametrize("k", [3, 5])
def test_temporal_smooth_byte_exact(k):
    seq = np.random.default_rng(40 + k).integers(0, 256, (9, 7, 11, 3), dtype=np.uint8)  # 231 bytes: the byte path
    want = np.stack(CR.temporal_smooth(list(seq), k))
    got = CAM.temporal_smooth_frames(_dev(seq), k).cpu().numpy()
    assert np.array_equal(got, want)
    half = k // 2
    # windows with halo: the start of the sequence, the middle, the end
    for first, n, o0, cnt in ((0, 3 + half, 0, 3), (3 - half, 3 + 2 * half, 3, 3), (6 - half, 3 + half, 6, 3)):
        w = CAM.temporal_smooth_window(_dev(seq[first:first + n]), first, 9, o0, cnt, k).cpu().numpy()
        assert np.array_equal(w, want[o0:o0 + cnt]), (first, n, o0)
    # the stream the CLI uses, in batches of 2 and of 4
    for step in (2, 4):
        s = CAM.SmoothStream(9, k)
        parts = [s.push(_dev(seq[i:i + step])) for i in range(0, 9, step)]
        assert np.array_equal(torch.cat([p for p in parts if p is not None]).cpu().numpy(), want)
    # dword path (8 * 12 * 3 bytes) and a sequence no longer than the kernel
    seq4 = np.random.default_rng(50).integers(0, 256, (k + 1, 8, 12, 3), dtype=np.uint8)
    assert np.array_equal(CAM.temporal_smooth_frames(_dev(seq4), k).cpu().numpy(), np.stack(CR.temporal_smooth(list(seq4), k)))
    short = seq4[:k]
    assert np.array_equal(CAM.temporal_smooth_frames(_dev(short), k).cpu().numpy(), short)
    assert np.array_equal(CAM.temporal_smooth_window(_dev(short), 0, k, 0, k, k).cpu().numpy(), short)  # the ABI's copy


def _plan5(w, h, pulse, hue):
    """Five different descriptors: zoom phase at three crop sizes (one equal to the frame, one to the target), pan
    phase at a fractional position and at the end of the pan (replicated column)."""
    plan = [CAM.CameraFrame(0.0, w, h, True, w, h, w / 2.0, h / 2.0, 0.0),
            CAM.CameraFrame(0.1, w, h, True, 31, 22, w / 2.0, h / 2.0, 37.3),
            CAM.CameraFrame(0.2, w, h, True, TW, TH, w / 2.0, h / 2.0, -45.0),
            CAM.CameraFrame(0.6, w, h, False, TW, TH, 7.37 + TW / 2.0, (h - TH) / 2.0 + TH / 2.0, 180.0),
            CAM.CameraFrame(1.0, w, h, False, TW, TH, float(w - TW) + TW / 2.0, float(h - TH) + TH / 2.0, 359.9)]
    sizes = [(w + 2, h + 1), (w + 5, h + 3), (w, h), (w + 1, h + 1), (w + 9, h + 6)]
    out = []
    for p, (nw, nh) in zip(plan, sizes):
        d = dict(p.__dict__)
        if pulse:
            d["pulse_w"], d["pulse_h"] = nw, nh
        if not hue:
            d["hue_shift"] = 0.0
        out.append(CAM.CameraFrame(**d))
    return out


@pytest.mark.parametrize("hue", [False, True])
@pytest.mark.parametrize("pulse", [False, True])
@pytest.mark.parametrize("hw", [(37, 53), (40, 56)])
def test_fused_camera_equals_the_chain_of_stages(hw, pulse, hue):
    h, w = hw
    fr = _frames(h, w)
    plan = _plan5(w, h, pulse, hue)
    got = CAM.camera_frames(_dev(fr), plan, (TW, TH)).cpu().numpy()
    assert got.shape == (5, TH, TW, 3)
    for i, p in enumerate(plan):
        want = CR.camera_frame(fr[i], dict(p.__dict__), TW, TH)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    # a batch that starts off a dword boundary, and the single stages chained on the device
    got2 = CAM.camera_frames(_dev(fr)[1:], plan[1:], (TW, TH)).cpu().numpy()
    assert np.array_equal(got2, got[1:])
    p = plan[3]
    x = _dev(fr[3:4])
    if pulse:
        x = CAM.zoom_pulse_frames(x, [(p.pulse_w, p.pulse_h)])
    x = CAM.hue_shift_frames(CAM.rect_subpix(x, (TW, TH), [(p.cx, p.cy)]), [p.hue_shift])
    assert np.array_equal(x.cpu().numpy()[0], got[3])


def test_fused_camera_more_frames_than_one_call_takes():
    fr = np.random.default_rng(9).integers(0, 256, (CAM.MAX_FRAMES + 3, 20, 28, 3), dtype=np.uint8)
    plan = CAM.frame_plan(len(fr), (28, 20), (14, 10), 2.0, "diagonal", 0.25, 0.05, 2.0, 120.0)
    ref = CR.frame_plan(len(fr), 28, 20, 14, 10, 2.0, "diagonal", 0.25, 0.05, 2.0, 120.0)
    got = CAM.camera_frames(_dev(fr), plan, (14, 10)).cpu().numpy()
    for i in range(len(fr)):
        assert np.array_equal(got[i], CR.camera_frame(fr[i], ref[i], 14, 10)), i


def test_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    INV, SHP, WSP = _lib.NST_E_INVALID, _lib.NST_E_SHAPE, _lib.NST_E_WORKSPACE
    st = _lib.stream_ptr(DEV)
    x = torch.zeros((2, 37, 53, 3), dtype=torch.uint8, device=DEV)
    o = torch.zeros((2, 37, 53, 3), dtype=torch.uint8, device=DEV)
    xp, op = x.data_ptr(), o.data_ptr()
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    F = lambda *v: (ctypes.c_float * len(v))(*v)
    assert L.nst_camera_pulse_u8(xp, 2, 37, 53, I(53, 52), I(37, 37), op, st) == INV  # smaller than the frame
    assert L.nst_camera_pulse_u8(xp, 0, 37, 53, I(53), I(37), op, st) == INV
    assert L.nst_camera_pulse_u8(xp, 33, 37, 53, I(*[53] * 33), I(*[37] * 33), op, st) == INV
    assert L.nst_camera_pulse_u8(xp, 2, 37, 53, I(53, 53), I(37, 37), xp, st) == INV  # in place
    assert L.nst_camera_pulse_u8(xp, 1, 40000, 53, I(53), I(40000), op, st) == SHP
    assert L.nst_camera_pulse_u8(None, 1, 37, 53, I(53), I(37), op, st) == INV
    cx0, cy0 = (TW - 1) / 2.0, (TH - 1) / 2.0
    sub = lambda cx, cy, pw=TW, ph=TH: L.nst_camera_rect_subpix_u8(xp, 1, 37, 53, pw, ph, F(cx), F(cy), op, st)
    assert sub(cx0 + 3, cy0 + 3) == 0
    assert sub(cx0 - 0.5, cy0) == INV       # left border
    assert sub(cx0, cy0 - 0.25) == INV      # top border
    assert sub(cx0 + 29.5, cy0) == 0        # floor + patch = w: the replicated column
    assert sub(cx0 + 30, cy0) == INV        # one further
    assert sub(cx0, cy0 + 22) == INV
    assert sub(float("nan"), cy0) == INV and sub(cx0, float("inf")) == INV
    assert sub(26.0, 18.0, 54, 37) == INV   # patch wider than the frame
    assert sub(cx0, cy0, 0, TH) == INV
    tab = CAM.LanczosTables([(53, 37)], TW, TH, DEV)
    lan = lambda cw, ch, tw=TW, th=TH, t=tab.ptrs(): L.nst_camera_lanczos_u8(xp, 1, 37, 53, I(cw), I(ch), tw, th, *t, op, st)
    assert lan(53, 37) == 0
    assert lan(54, 37) == INV and lan(53, 0) == INV
    assert lan(53, 37, 0, TH) == SHP
    assert lan(53, 37, t=(None,) + tab.ptrs()[1:]) == INV
    assert L.nst_camera_hue_u8(xp, 1, 37, 53, I(1), F(float("nan")), op, st) == INV
    assert L.nst_camera_hue_u8(xp, 1, 37, 53, I(1), F(float("inf")), op, st) == INV
    assert L.nst_camera_hue_u8(xp, 1, 0, 53, I(1), F(1.0), op, st) == SHP
    wts = CAM.smooth_weights(3).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    sm = lambda win_n, first, seq, o0, cnt, k=3: L.nst_camera_smooth_u8(xp, win_n, 37, 53, first, seq, o0, cnt, k, wts, op, st)
    assert sm(2, 0, 2, 0, 2) == 0           # len <= kernel: the copy
    assert sm(2, 0, 9, 0, 2) == INV         # output 1 needs frame 2
    assert sm(2, 3, 9, 3, 1) == INV         # output 3 needs frame 2
    assert sm(2, 8, 9, 8, 1) == INV         # window past the sequence
    assert sm(2, 0, 9, 0, 1) == 0
    assert sm(2, 0, 9, 0, 1, 0) == INV and sm(2, 0, 9, 0, 1, 16) == INV
    w15 = CAM.smooth_weights(15).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.nst_camera_smooth_u8(xp, 2, 37, 53, 0, 2, 0, 2, 15, w15, op, st) == 0
    fr = (_lib.NstCameraFrame * 2)(_lib.NstCameraFrame(53, 37, 1, 30, 21, 26.5, 18.5, 0, 0.0, 0),
                                  _lib.NstCameraFrame(53, 37, 0, TW, TH, cx0 + 3, cy0 + 3, 0, 0.0, 0))
    sz = ctypes.c_size_t()
    assert L.nst_camera_scratch_bytes(fr, 2, ctypes.byref(sz)) == 0 and sz.value == (30 * 21 * 3 + 15) // 16 * 16
    assert L.nst_camera_scratch_bytes(fr, 0, ctypes.byref(sz)) == INV
    sc = torch.zeros((sz.value,), dtype=torch.uint8, device=DEV)
    t1 = CAM.LanczosTables([(30, 21)], TW, TH, DEV)
    run = lambda fr_, n=2, tw=TW, th=TH, slots=1, sb=sz.value: L.nst_camera_frames_u8(
        xp, n, 37, 53, fr_, tw, th, *t1.ptrs(), slots, op, sc.data_ptr(), sb, st)
    assert run(fr) == 0
    assert run(fr, sb=sz.value - 1) == WSP
    assert run(fr, slots=0) == INV           # the zoom frame's table slot does not exist
    assert run(fr, tw=54) == SHP
    bad = (_lib.NstCameraFrame * 2)(fr[0], _lib.NstCameraFrame(53, 37, 0, TW + 1, TH, cx0 + 3, cy0 + 3, 0, 0.0, 0))
    assert run(bad) == INV                   # a pan-phase patch that is not the target
    bad = (_lib.NstCameraFrame * 2)(fr[0], _lib.NstCameraFrame(52, 37, 0, TW, TH, cx0 + 3, cy0 + 3, 0, 0.0, 0))
    assert run(bad) == INV                   # pulse smaller than the frame
    bad = (_lib.NstCameraFrame * 2)(fr[0], _lib.NstCameraFrame(53, 37, 0, TW, TH, cx0 - 1, cy0 + 3, 0, 0.0, 0))
    assert run(bad) == INV                   # left border
    torch.cuda.synchronize()
    with pytest.raises(_lib.NstError, match="no CPU path"):
        CAM.camera_frames(x.cpu(), [], (TW, TH))


def _cli_stills(tmp_path):
    stills = synthetic.make_frames(3, 64, 96, seed=60)  # test_gpu_morph.test_cli_end_to_end's stills
    d_in = tmp_path / "in"
    d_in.mkdir()
    for nm, s in zip(("a.png", "b.png", "c.png"), stills):
        Image.fromarray(s).save(d_in / nm)
    return stills, d_in


def test_cli_camera_end_to_end(tmp_path):
    """Three 64x96 stills to 48x32 at pan_zoom 2 (pan size 96x64: load_for_pan is the identity), 2 x 4 transition
    frames + 2 held: the files are camera_ref applied to optical_flow_morph's frames (pinned by test_gpu_morph.py),
    smoothed over the whole sequence across the batches of 3."""
    stills, d_in = _cli_stills(tmp_path)
    d_out = tmp_path / "out"
    argv = ["--images_dir", str(d_in), "--size", "48x32", "--pan_zoom", "2", "--fps", "4", "--morph_seconds", "1",
            "--hold_end", "2", "--preset", "v2", "--batch", "3", "--temporal_smooth", "3", "--zoom_pulse", "0.05",
            "--zoom_pulse_freq", "2.0", "--hue_rotate", "90", "--pan_direction", "diagonal", "--zoom_in_pct", "0.25",
            "--output_dir", str(d_out)]
    assert MO.main(argv) == 0
    files = sorted(d_out.iterdir())
    total = MO.total_frames(3, 4, 0, 2)
    assert total == 10 and [f.name for f in files] == [f"morph_frame_{i:04d}.png" for i in range(1, 11)]
    dec = [np.array(Image.open(f)) for f in files]
    assert dec[0].shape == (32, 48, 3)
    loaded = [CAM.load_for_pan(d_in / nm, 48, 32, 2.0, 1.0, DEV) for nm in ("a.png", "b.png", "c.png")]
    for i in range(3):
        assert np.array_equal(loaded[i].cpu().numpy(), stills[i])
    morph = [MO.optical_flow_morph(loaded[t], loaded[t + 1], 4, "v2", "smooth").cpu().numpy() for t in range(2)]
    seq = list(morph[0]) + list(morph[1]) + [stills[2]] * 2
    plan = CR.frame_plan(total, 96, 64, 48, 32, 2.0, "diagonal", 0.25, 0.05, 2.0, 90.0)
    assert [d["zoom"] for d in plan] == [True] * 3 + [False] * 7
    want = CR.camera_sequence(seq, plan, 48, 32, 3)
    for i in range(total):
        assert np.array_equal(dec[i], want[i]), (i, int((dec[i] != want[i]).sum()))
    unsmoothed = CR.camera_sequence(seq, plan, 48, 32, 0)
    assert any(not np.array_equal(a, b) for a, b in zip(want, unsmoothed))


def test_cli_without_camera_flags_is_unchanged(tmp_path):
    """The run of test_gpu_morph.test_cli_end_to_end, once more: no new flag, the same files."""
    stills, d_in = _cli_stills(tmp_path)
    d_out = tmp_path / "out"
    assert MO.main(["--images_dir", str(d_in), "--size", "96x64", "--fps", "4", "--morph_seconds", "1", "--hold_frames",
                    "1", "--hold_end", "2", "--preset", "v2", "--output_dir", str(d_out), "--batch", "3"]) == 0
    files = sorted(d_out.iterdir())
    assert [f.name for f in files] == [f"morph_frame_{i:04d}.png" for i in range(1, 14)]
    dec = [np.array(Image.open(f)) for f in files]
    assert np.array_equal(dec[0], stills[0]) and np.array_equal(dec[5], stills[1])
    for i in (10, 11, 12):
        assert np.array_equal(dec[i], stills[2])
    for tr, first in ((0, 1), (1, 6)):
        want = MO.optical_flow_morph(_dev(stills[tr]), _dev(stills[tr + 1]), 4, "v2", "smooth").cpu().numpy()
        for j in range(4):
            assert np.array_equal(dec[first + j], want[j]), (tr, j)
