"""Host-side checks of the optical-flow morph (neuralstyletransferv1_amd/morph.py) and of its numpy restatement
(tests/morph_ref.py): schedules, CLI parsing, frame counts, file order, and properties the restatement must have on
its own.  No GPU.  cv2 is not installed here: parity with OpenCV itself is unpinned; these tests pin the restatement
to the closed forms and to properties (identity at zero flow, a brute-force mirror, a recovered translation)."""
import numpy as np
import pytest

import morph_ref as MR
from neuralstyletransferv1_amd import morph as MO


def _closed(easing, x):
    if easing == "linear":
        return x
    if easing == "smooth":
        return 4 * x ** 3 if x < 0.5 else 1 - (-2 * x + 2) ** 3 / 2
    return x ** 3 * (x * (6 * x - 15) + 10)


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("easing", ["linear", "smooth", "smoother"])
def test_schedules_closed_forms(k, easing):
    lin = [0.0] if k == 1 else [i / (k - 1) for i in range(k)]
    t, a = MO.schedule(k, "v2", easing)
    assert t.dtype == np.float64 and t.tolist() == [_closed(easing, x) for x in lin]
    assert a.tolist() == [x * x * (3 - 2 * x) for x in lin]
    ts, as_ = MO.schedule(k, "slideshow", easing)
    assert ts.tolist() == lin and as_.tolist() == lin
    # the restatement's schedules are the same numbers
    for preset in ("v2", "slideshow"):
        rt, ra = MR.schedule(k, preset, easing)
        mt, ma = MO.schedule(k, preset, easing)
        assert np.array_equal(rt, mt) and np.array_equal(ra, ma)
    assert t[0] == 0 and a[0] == 0
    if k > 1:
        assert t[-1] == 1 and a[-1] == 1
    # what the kernel is given: each row computed in double and rounded once
    r = MO.kernel_schedule(t, a)
    assert all(x.dtype == np.float32 for x in r)
    assert np.array_equal(r[1], np.array([np.float32(1.0 - x) for x in t]))
    assert np.array_equal(r[2], np.array([np.float32(1.0 - x) for x in a]))


def test_schedule_rejects_bad_arguments():
    with pytest.raises(ValueError):
        MO.schedule(0, "v2", "smooth")
    with pytest.raises(ValueError):
        MO.schedule(3, "v3", "smooth")
    with pytest.raises(ValueError):
        MO.schedule(3, "v2", "bouncy")


def test_presets_are_the_reference_parameter_sets():
    assert MO.PRESETS["slideshow"] == dict(farneback=(0.5, 5, 15, 3, 7, 1.5), pre_blur=False, post=False)
    assert MO.PRESETS["v2"] == dict(farneback=(0.5, 6, 21, 5, 7, 1.5), pre_blur=True, post=True)
    assert MO.PRESETS == MR.PRESETS


def test_cli_parsing_and_defaults():
    ap = MO.build_parser()
    a = ap.parse_args(["--images", "a.png", "b.png", "--output_dir", "o"])
    assert (a.size, a.fps, a.morph_seconds, a.preset, a.easing) == ((1920, 1080), 24.0, 2.0, "v2", "smooth")
    assert (a.hold_frames, a.hold_end, a.image_ext, a.png_writer, a.jpeg_writer) == (0, 24, "png", "pil", "pil")
    assert int(a.fps * a.morph_seconds) == 48
    a = ap.parse_args(["--images_dir", "d", "--output_dir", "o", "--size", "96x64", "--fps", "4", "--morph_seconds", "1",
                       "--hold_frames", "1", "--hold_end", "2", "--preset", "slideshow", "--easing", "smoother",
                       "--image_ext", "jpg", "--jpeg_writer", "gpu", "--jpeg_quality", "90", "--batch", "3",
                       "--output_prefix", "f", "--output_video", "v.mp4"])
    assert a.size == (96, 64) and a.images is None and a.images_dir == "d" and a.batch == 3
    for bad in (["--output_dir", "o"], ["--images", "a", "--images_dir", "d", "--output_dir", "o"],
                ["--images", "a", "b", "--output_dir", "o", "--size", "96"],
                ["--images", "a", "b", "--output_dir", "o", "--preset", "v3"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(bad)
        assert e.value.code == 2


def test_fewer_than_two_images_is_exit_2(tmp_path, capsys):
    (tmp_path / "only.png").write_bytes(b"")
    assert MO.main(["--images_dir", str(tmp_path), "--output_dir", str(tmp_path / "o")]) == 2
    assert MO.main(["--images", str(tmp_path / "only.png"), "--output_dir", str(tmp_path / "o")]) == 2
    assert "at least 2 images" in capsys.readouterr().err
    assert not (tmp_path / "o").exists()


def test_frame_count_formula():
    assert MO.total_frames(3, 4, 1, 2) == 3 + 8 + 2
    assert MO.total_frames(2, 72, 0, 24) == 96
    assert MO.total_frames(5, 12, 18, 0) == 5 * 18 + 4 * 12


def test_file_order_rule(tmp_path):
    for name in ("b.png", "a.jpeg", "c.jpg", "A.png", "notes.txt", "d.bmp"):
        (tmp_path / name).write_bytes(b"")
    got = [p.name for p in MO.list_images(str(tmp_path), None)]
    assert got == ["A.png", "a.jpeg", "b.png", "c.jpg"]  # the three patterns together, sorted by path
    assert [p.name for p in MO.list_images(None, ["z.png", "a.png"])] == ["z.png", "a.png"]  # --images: as given


def test_cover_geometry():
    # morph_v2.py:704-712: scale = max(tw / w, th / h), int(w * scale), (new - target) // 2
    assert MO.cover_geometry(100, 50, 96, 64) == (128, 64, 16, 0)
    assert MO.cover_geometry(96, 64, 96, 64) == (96, 64, 0, 0)
    assert MO.cover_geometry(64, 96, 96, 64) == (96, 144, 0, 40)
    for (w, h, tw, th) in [(1000, 667, 1280, 720), (333, 77, 96, 64), (4032, 3024, 1920, 1080)]:
        nw, nh, sx, sy = MO.cover_geometry(w, h, tw, th)
        assert nw >= tw and nh >= th and 0 <= sx <= nw - tw and 0 <= sy <= nh - th


# ---- properties of the restatement ----
def _stills(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("preset", ["slideshow", "v2"])
def test_zero_flow_ends_are_the_stills(preset):
    a, b = _stills(40, 56, 1)
    z = np.zeros((40, 56, 2), np.float32)
    t, al = MR.schedule(5, preset)
    fr = MR.morph_frames(a, b, z, z, t, al)
    assert fr.shape == (5, 40, 56, 3) and fr.dtype == np.uint8
    assert np.array_equal(fr[0], a) and np.array_equal(fr[-1], b)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_reflect_index_vs_brute_force_mirror(n):
    # BORDER_REFLECT: ...cba|abc...|cba...: walk an explicit mirrored tape
    period = list(range(n)) + list(range(n - 1, -1, -1))
    for p in range(-3 * n, 4 * n):
        q = p
        while q < 0:
            q += 2 * n
        assert int(MR.reflect_index(np.int64(p), n)) == period[q % (2 * n)], (p, n)
    got = MR.reflect_index(np.arange(-3 * n, 4 * n), n)
    assert got.min() >= 0 and got.max() <= n - 1


def test_window_taps():
    k = MR.window_taps(15)
    assert k.dtype == np.float32 and len(k) == 8
    assert abs(float(k[0]) + 2 * float(k[1:].sum()) - 1) < 1e-6
    assert (np.diff(k) < 0).all()


def test_gray_cv_and_add_weighted():
    assert MR.gray_cv(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)).tolist() \
        == [[255, 0, 76, 150, 29]]
    a = np.array([[1, 3, 255, 0]], np.uint8)
    b = np.array([[2, 4, 255, 1]], np.uint8)
    assert MR.add_weighted(a, 0.5, b, 0.5).tolist() == [[2, 4, 255, 0]]  # 1.5 -> 2, 3.5 -> 4, 0.5 -> 0 (half to even)


def test_flow_post_threshold_seed():
    """The GPU test's flow (MR.post_test_flow: 64x80, amplitude +-6, seed 11, both signs): both sides of the 2-px
    threshold occur, and at most 0.1 % of the pixels lie within 1e-4 of it (those are left out of the GPU
    comparison)."""
    flow = MR.post_test_flow(11)
    assert flow.shape == (2, 64, 80, 2) and np.abs(flow).max() <= 6
    for k, sign in enumerate((1.0, -1.0)):
        out, mag = MR.flow_post(flow[k], sign)
        near = np.abs(mag - 2.0) < 1e-4
        assert near.mean() <= 1e-3
        assert (mag < 2.0).mean() > 0.1 and (mag >= 2.0).mean() > 0.1
        print("share below the threshold", float((mag < 2.0).mean()), "left out", int(near.sum()))
        assert out.dtype == np.float32


def test_gaussian_window_recovers_a_translation():
    """The Gaussian-window restatement on the (3, -2) shifted texture at 135x240 with the slideshow parameters:
    measured median of the interior (20 px margin) 2.99955 / -1.99972, i.e. a median error of 4.5e-4 / 2.8e-4 px.
    Bar 0.05 px, as for the box window (tests/test_gpu_flow.py); the GPU bar is max(0.05, 2 x this error) = 0.05."""
    prev, nxt = MR.texture_pair(135, 240, 3, -2)
    fl = MR.farneback_gauss(prev, nxt, *MR.PRESETS["slideshow"]["farneback"])
    c = fl[20:-20, 20:-20]
    ex, ey = abs(float(np.median(c[..., 0])) - 3), abs(float(np.median(c[..., 1])) + 2)
    print("median error", ex, ey, "medians", float(np.median(c[..., 0])), float(np.median(c[..., 1])))
    assert ex < 0.05 and ey < 0.05
