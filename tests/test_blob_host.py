"""selfstyle_blob's host side (no GPU): the tile configurations, the legacy-generator phases, the field and the plan
against tests/blob_ref.py, the parser's defaults, every exit-2 condition, the output-size rule, and the numpy
reference's own cast discipline."""
from __future__ import annotations

import numpy as np
import pytest
from PIL import Image

import blob_ref as BR
from neuralstyletransferv1_amd import _lib, selfstyle_blob as SB


def test_tile_configs():
    want = [(256, 32), (256, 56), (256, 85), (288, 36), (288, 64), (288, 96), (320, 40), (320, 72), (320, 106),
            (352, 44), (352, 80), (352, 117), (384, 48), (384, 88), (384, 128), (416, 52), (416, 88), (416, 138),
            (448, 56), (448, 96), (448, 149), (480, 60), (480, 104), (480, 160)]
    assert SB.generate_tile_configs(256, 512, 24) == want == BR.tile_configs(256, 512, 24)
    # 64 // 8 < 16: the low overlap is 16 and 21 is too near for a midpoint; the count cuts the third tile short
    small = [(64, 16), (64, 21), (80, 16), (80, 26), (96, 16)]
    assert SB.generate_tile_configs(64, 128, 5) == small == BR.tile_configs(64, 128, 5)
    for a in ((256, 512, 100), (100, 100, 3), (16, 700, 50), (40, 47, 9)):
        assert SB.generate_tile_configs(*a) == BR.tile_configs(*a), a
    assert SB.generate_tile_configs(40, 47, 9) == [(40, 16)]  # tile // 3 < 16: one overlap


def test_sort_key():
    assert SB.sort_key("/x/img_tile256_overlap32.jpg") == (256, 32) == BR.sort_key("/x/img_tile256_overlap32.jpg")
    assert SB.sort_key("a_tile96_overlap16_udnie.jpg") == (96, 16)
    assert SB.sort_key("plain.jpg") == (0, 0)
    names = ["b_tile1024_overlap128.jpg", "a_tile96_overlap16.jpg", "a_tile256_overlap85.jpg", "a_tile256_overlap32.jpg"]
    assert sorted(names, key=SB.sort_key) == [names[1], names[3], names[2], names[0]]
    with pytest.raises(ValueError):
        SB.sort_key("a_tileX_overlap3.jpg")


@pytest.mark.parametrize("seed", [42, 7])
def test_phases(seed):
    """The legacy global generator's stream, drawn x, y, t per octave, without touching the global state."""
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    got = SB.phases(seed, 3)
    assert np.array_equal(np.random.get_state()[1], before)
    for b in range(3):
        np.random.seed(seed + 1000 * b)
        for o in range(4):
            for k in range(3):
                assert got[b, o, k] == np.random.random() * 2 * np.pi
    fd = SB.field(3, 2.5, seed, 0.15)
    assert fd["phase_x"][2][1] == got[2, 1, 0] and fd["phase_y"][2][1] == got[2, 1, 1] and fd["phase_t"][0][3] == got[0, 3, 2]
    if seed == 42:  # np.random.seed(42); np.random.random()
        assert got[0, 0, 0] == 0.3745401188473625 * 2 * np.pi


def test_field_and_times():
    fd = SB.field(8, 4.0, 42, 0.3)
    assert fd["T"] == 1.5 and SB.field(2, feather=0.0)["T"] == 0.1 and SB.field(2)["T"] == 0.75
    assert fd["freq"] == [4.0, 8.0, 16.0, 32.0] and fd["amp"][2] == 1.0 / 2.25 and fd["amp_half"][3] == (1.0 / 1.5 ** 3) * 0.5
    assert fd["blob_phase"][3] == 3 * 2 * np.pi / 8
    t = SB.frame_times(360, 2.0)
    off = 360 * 2.0 * 0.02
    assert t["t_y"] == [off * (1 + o * 0.3) for o in range(4)] and t["t_x"][3] == off * (1.2 + 3 * 0.2) and t["t_t"] == off * 1.5
    packed = SB.pack_field(fd)
    assert packed.n_blobs == 8 and packed.T == 1.5 and packed.phase_t[7][3] == np.float32(fd["phase_t"][7][3])
    assert packed.amp_half[1] == np.float32((1.0 / 1.5) * 0.5)
    for bad in (0, 9):
        with pytest.raises(_lib.NstError, match="outside 1..8"):
            SB.field(bad)


@pytest.mark.parametrize("nb", [1, 2, 3, 8])
@pytest.mark.parametrize("n_magenta", [0, 4])
@pytest.mark.parametrize("speed", [0.5, 2.0])
def test_plan_against_the_reference_schedule(nb, n_magenta, speed):
    n_styled, fps, duration = 6, 4, 5
    pl = SB.plan(n_styled, n_magenta, fps, duration, nb, speed, 1.5)
    sched = BR.schedule(n_styled, n_magenta, fps, duration, nb, speed)
    assert len(pl) == len(sched) == 20
    wrapped = False
    for i, (d, row) in enumerate(zip(pl, sched)):
        assert d["t_t"] == i * 1.5 * 0.02 * 1.5 and len(d["blobs"]) == nb
        for b, (s, (stream, i1, i2, w1, w2)) in enumerate(zip(d["blobs"], row)):
            base = n_styled if stream == "magenta" else 0
            assert (s["lo"], s["hi"], s["w_lo"], s["w_hi"]) == (base + i1, base + i2, w1, w2), (i, b)
            assert stream == ("magenta" if n_magenta and b % 2 else "styled")
            wrapped = wrapped or (i2 == 0 and i1 > 0)
    if nb > 1:
        assert wrapped  # some blob stands on the last still and fades into the first


def test_plan_wraps_and_single_still():
    # speed 2 over 6 stills: positions pass n and start again
    pl = SB.plan(6, 0, 4, 5, 1, 2.0)
    los = [d["blobs"][0]["lo"] for d in pl]
    assert max(los) == 5 and los[-1] < 5 and los.index(5) < len(los) - 1
    one = SB.plan(1, 0, 2, 2, 3)
    assert all(s["lo"] == 0 and s["hi"] == 0 for d in one for s in d["blobs"])
    with pytest.raises(_lib.NstError, match="no styled stills"):
        SB.plan(0)


def test_pack_rounds_each_double_once():
    pl = SB.plan(6, 0, 4, 5, 3, 1.0, 1.0)
    arr = SB.pack(pl)
    assert len(arr) == 20
    d = pl[13]
    assert arr[13].t_y[2] == np.float32(d["t_y"][2]) and arr[13].t_t == np.float32(d["t_t"])
    assert arr[13].blob[2].w_hi == np.float32(d["blobs"][2]["w_hi"]) and arr[13].blob[2].lo == d["blobs"][2]["lo"]
    with pytest.raises(_lib.NstError, match="at most 8 blobs"):
        SB.pack([dict(d, blobs=d["blobs"] * 3)])


def test_parser_defaults():
    a = SB.build_parser().parse_args(["--styled_dir", "s", "--original", "o.jpg", "--output_dir", "out"])
    assert (a.fps, a.duration, a.blend_original, a.blob_frequency, a.blob_speed) == (24, 30, 0.5, 2.5, 1.0)
    assert (a.max_resolution, a.seed, a.num_blobs, a.transition_speed, a.feather) == (1280, 42, 2, 1.0, 0.15)
    assert a.magenta_dir is None and a.output is None and a.jpeg_reader == "pil"
    assert (a.output_prefix, a.image_ext, a.jpeg_quality, a.png_writer, a.jpeg_writer) == ("blob_frame", "png", 85, "pil", "pil")


def test_output_size():
    assert SB.output_size(1080, 1440, 1280) == (960, 1280)
    assert SB.output_size(1081, 1441, 1280) == (960, 1280)   # int(1081 * 1280 / 1441) = 960
    assert SB.output_size(1000, 1441, 1280) == (888, 1280)
    assert SB.output_size(1441, 999, 1280) == (1280, 886)    # 887 made even
    assert SB.output_size(37, 51, 1280) == (36, 50) and SB.output_size(36, 50, 50) == (36, 50)
    assert SB.output_size(20, 28, 24) == (16, 24)
    for w, h, cap in ((1081, 1441, 1280), (1441, 999, 1280), (37, 51, 1280), (333, 77, 100), (20, 28, 24)):
        assert SB.output_size(w, h, cap) == BR.output_size(h, w, cap)


def _jpeg(path, w, h, value=90):
    Image.fromarray(np.full((h, w, 3), value, np.uint8)).save(path, format="JPEG")


def _argv(tmp, *extra):
    return ["--styled_dir", str(tmp / "styled"), "--original", str(tmp / "orig.jpg"), "--output_dir", str(tmp / "out"),
            *extra]


@pytest.fixture
def layout(tmp_path):
    (tmp_path / "styled").mkdir()
    for tile, ov in ((256, 32), (288, 36), (320, 40)):
        _jpeg(tmp_path / "styled" / f"img_tile{tile}_overlap{ov}.jpg", 20, 28)
    _jpeg(tmp_path / "orig.jpg", 40, 56)
    return tmp_path


def _refused(argv, capsys, text):
    assert SB.main(argv) == 2
    assert text in capsys.readouterr().err


def test_usage_errors(layout, capsys, monkeypatch):
    """Exit status 2, a message, and no touch of the device or of --output_dir."""
    import torch
    monkeypatch.setattr(torch, "device", lambda *a, **k: pytest.fail("the device was touched"))
    tmp = layout
    args = SB.build_parser().parse_args(_argv(tmp))
    styled, magenta, size, out_wh = SB.prepare(args)
    assert [p.name for p in styled] == ["img_tile256_overlap32.jpg", "img_tile288_overlap36.jpg", "img_tile320_overlap40.jpg"]
    assert magenta == [] and size == (20, 28) and out_wh == (20, 28)
    for bad in ("0", "9", "-1"):
        _refused(_argv(tmp, "--num_blobs", bad), capsys, f"--num_blobs {bad} outside 1..8")
    (tmp / "empty").mkdir()
    _refused(["--styled_dir", str(tmp / "empty"), "--original", str(tmp / "orig.jpg"), "--output_dir", str(tmp / "out")],
             capsys, "no readable *_tile*_overlap*.jpg stills")
    _refused(_argv(tmp, "--original", str(tmp / "missing.jpg")), capsys, "missing.jpg: not a readable image")
    (tmp / "text.jpg").write_text("not an image")
    _refused(_argv(tmp, "--original", str(tmp / "text.jpg")), capsys, "text.jpg: not a readable image")
    _refused(_argv(tmp, "--seed", "-1"), capsys, "--seed")
    _refused(_argv(tmp, "--fps", "0"), capsys, "--fps")
    _refused(_argv(tmp, "--blend_original", "1.5"), capsys, "--blend_original outside 0..1")
    # a second directory whose stills have another size
    (tmp / "magenta").mkdir()
    _jpeg(tmp / "magenta" / "img_tile256_overlap32.jpg", 28, 20)
    _refused(_argv(tmp, "--magenta_dir", str(tmp / "magenta")), capsys, "is 28x20")
    # a still of another size among the styled ones; an unreadable still is skipped, as the script skips it
    (tmp / "styled" / "img_tile999_overlap9.jpg").write_text("not an image")
    assert len(SB.prepare(SB.build_parser().parse_args(_argv(tmp)))[0]) == 3
    _jpeg(tmp / "styled" / "img_tile512_overlap64.jpg", 20, 30)
    _refused(_argv(tmp), capsys, "img_tile512_overlap64.jpg: is 20x30")
    assert not (tmp / "out").exists()


def test_reference_masks_stay_float32():
    """Under NumPy 2 an unwrapped Python scalar would promote the reference's lines to float64: the restatement wraps
    every scalar, so both variants return float32 and differ only by their library's rounding."""
    a = BR.soft_masks(9, 11, 17, 3, 2.5, 1.0, 42, 0.15, "numpy")
    d = BR.soft_masks(9, 11, 17, 3, 2.5, 1.0, 42, 0.15, "double")
    assert a.dtype == np.float32 and d.dtype == np.float32 and a.shape == (3, 9, 11)
    assert np.abs(a.sum(axis=0, dtype=np.float64) - 1).max() < 1e-5
    assert 0 < np.abs(a - d).max() < 1e-5 or np.array_equal(a, d)
    one = BR.soft_masks(1, 7, 0, 1, 2.5, 1.0, 42, 0.0)
    assert one.dtype == np.float32 and np.all(one == np.float32(1) / (np.float32(1) + np.float32(1e-6)))
    y = np.linspace(0, 1, 9, dtype=np.float32)
    assert (y * np.float32(2.5) * np.float32(np.pi)).dtype == np.float32
