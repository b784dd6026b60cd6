"""Host side of the style morph (neuralstyletransferv1_amd/style_morph.py): discovery, the plan against the
reference's loop (tests/style_morph_ref.py render(), the script's own float32 numpy expressions), the filters' closed
forms and every exit-2 condition of the CLI.  No GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from PIL import Image

import style_morph_ref as SR
from neuralstyletransferv1_amd import style_morph as SM

FPS, FRAME_TIME = 4, 2.0  # 8 frames per image, a 6-frame cross-fade


def _touch(d, *names):
    for n in names:
        (d / n).write_bytes(b"")


def _jpeg(path, w, h, seed=0):
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path, format="JPEG", quality=90)


def _write_stills(d, names=("A", "B", "C"), w=24, h=20, styles=("original", "candy", "candy_style1e9")):
    for i, n in enumerate(names):
        for j, s in enumerate(styles):
            _jpeg(d / f"{n}_{s}.jpg", w, h, seed=10 * i + j)


def test_ladder_tables():
    assert list(SM.LADDERS) == ["candy", "udnie", "mosaic", "rain_princess", "tenharmsel"]
    assert [len(SM.LADDERS[k]) for k in SM.LADDERS] == [8, 8, 8, 8, 28]
    assert SM.LADDERS["candy"][:3] == ("candy", "candy_style1e9", "candy_style5e9")
    assert SM.LADDERS["rain_princess"][-1] == "rain_princess_style1e12"
    t = SM.LADDERS["tenharmsel"]
    assert t[0] == "tenharmsel_style1e9" and t[8] == "tenharmsel_style9e9" and t[9] == "tenharmsel_style1e10"
    assert t[26] == "tenharmsel_style9e11" and t[27] == "tenharmsel_style1e12" and len(set(t)) == 28


def test_discover_name_rule_junk_and_skip_first(tmp_path):
    _touch(tmp_path, "IMG_001_original.jpg", "IMG_001_candy.jpg", "IMG_001_candy_style1e9.jpg",
           "IMG_002_original.jpg", "IMG_002_rain_princess.jpg", "AAA_original.jpg", "cover.jpg", "IMG_003_candy.png")
    every = SM.discover(tmp_path, skip_first=False)
    # IMG_001_candy comes from IMG_001_candy_style1e9.jpg, IMG_002_rain from IMG_002_rain_princess.jpg; cover.jpg has
    # no '_' and the .png is not globbed
    assert every == ["AAA", "IMG_001", "IMG_001_candy", "IMG_002", "IMG_002_rain"]
    assert SM.discover(tmp_path) == every[1:]
    one = tmp_path / "one"  # a single name is never skipped
    one.mkdir()
    _touch(one, "X_original.jpg")
    assert SM.discover(one, skip_first=True) == ["X"]


def test_collect_drops_junk_names_and_draws_filters_in_order(tmp_path):
    _write_stills(tmp_path)
    _jpeg(tmp_path / "D_candy.jpg", 24, 20)          # no original
    _jpeg(tmp_path / "E_original.jpg", 24, 20)       # no ladder image
    (tmp_path / "B_candy_style5e9.jpg").write_bytes(b"not a jpeg")  # unreadable: skipped like imread's None
    names = SM.discover(tmp_path, skip_first=False)
    assert "A_candy" in names and "D" in names and "E" in names
    stills = SM.collect(tmp_path, names, SM.select_ladders(None), 16, False, "random", seed=3)
    assert [s["name"] for s in stills] == ["A", "B", "C"]
    assert [len(s["ladders"]["candy"]) for s in stills] == [2, 2, 2] and list(stills[0]["ladders"]) == ["candy"]
    import random
    rng = random.Random(3)
    assert [s["filter"] for s in stills] == [rng.choice(SM.FILTERS) for _ in range(3)]
    fixed = SM.collect(tmp_path, names, SM.select_ladders(["candy"]), 16, False, "warm", seed=3)
    assert [s["filter"] for s in fixed] == ["warm"] * 3
    # skip_first removes the first sorted name before the usable filter runs
    assert [s["name"] for s in SM.collect(tmp_path, SM.discover(tmp_path), SM.LADDERS, 16)] == ["B", "C"]


@pytest.mark.parametrize("k", [2, 3, 5])
def test_frame_count(k):
    images = [dict(families=[("candy", 8), ("udnie", 3)], filter="none")] * k
    pl = SM.plan(images, FRAME_TIME, FPS, 0.08)
    fc, cf = SM.frame_counts(FRAME_TIME, FPS)
    assert (fc, cf) == (8, 6)
    assert len(pl["frames"]) == fc + (k - 1) * (fc - cf) == SM.total_frames(k, fc, cf)
    assert SM.frame_counts(4.0, 24) == (96, 36)
    # frames f < crossfade_frames of every image but the first are not emitted
    assert [d["still"] for d in pl["frames"]] == [0] * 8 + [i for i in range(1, k) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def _case():
    data = SR.layout_images(16, 20)
    return data, SM.plan(SR.plan_images(data), FRAME_TIME, FPS, 0.08), SR.render(data, FRAME_TIME, FPS, 0.08)


def test_plan_descriptors_equal_the_reference_loop():
    data, pl, ref = _case()
    assert len(ref) == len(pl["frames"]) == 8 + 2 * 2
    for k, (d, want) in enumerate(zip(pl["frames"], ref)):
        got = SR.evaluate(SR.bank_of(data, pl["needs"], d["still"]), d)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"frame {k}"


def test_plan_covers_the_cases_the_layout_is_for():
    data, pl, _ = _case()
    fr = pl["frames"]
    # frame 0: IMG_001's second family at ladder position exactly 1.0 -> idx_low == idx_high, blend 0
    t = fr[0]["sides"][0]["terms"][1]
    assert SR.get_ladder_position(1, 0.0) == 1.0
    assert t["lo"] == t["hi"] and (t["w_lo"], t["w_hi"]) == (1.0, 0.0)
    # the one-rung ladder (mosaic of IMG_001) is taken as it is
    assert all(d["sides"][0]["terms"][2]["hi"] == -1 for d in fr if d["still"] == 0)
    # cross-fades: frames 2..7 of stills 0 and 1 have two sides, the last still none
    assert [d["n_sides"] for d in fr] == [1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1]
    # IMG_002 lacks udnie: its style_idx 1 is mosaic, two terms only
    assert [len(d["sides"][0]["terms"]) for d in fr if d["still"] == 1] == [2, 2]
    assert len(fr[2]["sides"][1]["terms"]) == 2
    # bank indices stay inside needs[i] + needs[i + 1]
    for d in fr:
        n_bank = len(pl["needs"][d["still"]]) + (len(pl["needs"][d["still"] + 1]) if d["still"] + 1 < len(data) else 0)
        for sd in d["sides"]:
            idx = [sd["orig"]] + [t["lo"] for t in sd["terms"]] + [t["hi"] for t in sd["terms"] if t["hi"] >= 0]
            assert all(0 <= i < n_bank for i in idx)
    assert all(n[0] == SM.ORIGINAL for n in pl["needs"])
    # every scalar is a Python float (a np.float64 would promote the float32 frame arithmetic)
    for d in fr:
        vals = list(d["fade"]) + list(d["fparam"])
        for sd in d["sides"]:
            vals.append(sd["orig_w"])
            for t in sd["terms"]:
                vals += [t["w_lo"], t["w_hi"], t["weight"]]
        assert all(type(v) is float for v in vals)


def test_weights_sum_to_one_per_side():
    _, pl, _ = _case()
    for d in pl["frames"]:
        for sd in d["sides"]:
            assert abs(sd["orig_w"] + sum(t["weight"] for t in sd["terms"]) - 1.0) <= 1e-6
        assert abs(d["fade"][0] + d["fade"][1] - 1.0) <= 1e-12


def test_filter_parameters():
    assert SM.FILTER_PARAMS["subtle_sat"] == (1, (1.08, 0.0, 0.0))
    assert SM.FILTER_PARAMS["vibrance"] == (2, (1.08, 1 - 1.08, 0.0))
    assert SM.FILTER_PARAMS["warm"] == (3, (1 + 0.05, 1 + 0.05 * 0.3, 1 - 0.05 * 0.3))


def test_filter_closed_forms():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for name in ("subtle_sat", "vibrance"):
        code, fp = SM.FILTER_PARAMS[name]
        assert np.array_equal(SR.FILTERS[name](grey), grey)
        assert np.array_equal(SR.apply_filter(grey, code, fp), grey)
    code, fp = SM.FILTER_PARAMS["warm"]
    # float32(1.05) = 1.04999995: 100 * it = 104.99999 -> 104; 200 * float32(1.015) = 203.0; 50 * float32(0.985) = 49.25
    # 250 * 1.05 = 262.5 and 255 * 1.015 = 258.8 clip to 255; 255 * 0.985 = 251.175 -> 251
    px = np.array([[[100, 200, 50], [250, 255, 255]]], np.uint8)
    want = np.array([[[104, 203, 49], [255, 255, 251]]], np.uint8)
    assert np.array_equal(SR.FILTERS["warm"](px), want)
    assert np.array_equal(SR.apply_filter(px, code, fp), want)
    # saturation clips at 255: a fully saturated colour keeps s = 255
    red = np.array([[[200, 0, 0]]], np.uint8)
    assert np.array_equal(SR.apply_filter(red, *SM.FILTER_PARAMS["subtle_sat"]), red)
    # the evaluator's filters are the script's, over every (r, g) pair at four blues
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for b in (0, 77, 128, 255):
        img = np.stack([r, g, np.full_like(r, b)], -1)
        for name in SM.FILTERS:
            assert np.array_equal(SR.apply_filter(img, *SM.FILTER_PARAMS[name]), SR.FILTERS[name](img)), (name, b)


def test_vibrance_division_is_not_a_reciprocal_multiply():
    s = np.arange(256, dtype=np.float32)
    assert int((s / np.float32(255) != s * (np.float32(1) / np.float32(255))).sum()) == 126


# ---- exit status 2, before the device is touched (this file runs without one) ----
def _run(tmp_path, *extra):
    return SM.main(["--styled_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--size", "16",
                    "--fps", str(FPS), "--frame_time", str(FRAME_TIME), "--no_skip_first", "--device", "cuda:0", *extra])


def test_cli_refuses_fewer_than_two_usable_images(tmp_path, capsys):
    _write_stills(tmp_path, names=("A",))
    _jpeg(tmp_path / "B_original.jpg", 24, 20)  # no ladder image: not usable
    assert _run(tmp_path) == 2
    assert "at least 2" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
    # two usable names, but skip_first removes one
    _jpeg(tmp_path / "B_candy.jpg", 24, 20)
    assert SM.main(["--styled_dir", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--size", "16", "--fps", "4",
                    "--frame_time", "2.0"]) == 2


def test_cli_refuses_a_frame_count_below_the_crossfade(tmp_path, capsys):
    _write_stills(tmp_path)
    assert _run(tmp_path, "--frame_time", "1.25") == 2  # int(4 * 1.25) = 5 < int(4 * 1.5) = 6
    assert "cross-fade" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_cli_refuses_an_unknown_family(tmp_path, capsys):
    _write_stills(tmp_path)
    assert _run(tmp_path, "--families", "candy", "starry_night") == 2
    assert "starry_night" in capsys.readouterr().err


def test_cli_refuses_images_of_differing_sizes(tmp_path, capsys):
    _write_stills(tmp_path)
    _jpeg(tmp_path / "C_candy.jpg", 30, 20)  # portrait mode keeps the aspect: int(30 * 16 / 20) = 24, the others 19
    assert _run(tmp_path, "--portrait") == 2
    assert "C_candy.jpg" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_prepare_accepts_the_good_directory(tmp_path):
    _write_stills(tmp_path)
    args = SM.build_parser().parse_args(["--styled_dir", str(tmp_path), "--output_dir", "x", "--size", "16", "--fps", "4",
                                         "--frame_time", "2.0", "--no_skip_first", "--output", "v.mp4", "--filter", "none"])
    assert args.output_video == "v.mp4"
    stills, pl = SM.prepare(args)
    assert [s["name"] for s in stills] == ["A", "B", "C"] and len(pl["frames"]) == 12
