"""Host side of the multi-model video (neuralstyletransferv1_amd/multi_model_video.py): the size rule, the walk-file
lookup, the pulse and ramp scalars, the plan against the reference's loop (tests/multi_model_ref.py render(), the
script's own float32 numpy expressions) over LAYOUT, and every exit-2 condition of the CLI.  No GPU."""
from __future__ import annotations

import functools
import json
import math

import numpy as np
import pytest

import multi_model_ref as MR
from neuralstyletransferv1_amd import multi_model_video as MM

L = MR.LAYOUT
CROSSFADE = int(L["crossfade_seconds"] * L["fps"])
# LAYOUT's three runs.  main: the issue's setting; its styled section (6 frames) lies wholly inside the 6-frame
# cross-fade window, so a fade-in without a cross-fade cannot occur in it: short_fade (a 2-frame cross-fade, a 1-frame
# fade-in) is the same layout where it does.  no_walk: the udnie directory without its walk file.
RUNS = {
    "main": (dict(L["weights"]), CROSSFADE),
    "no_walk": ({"tenharmsel": L["weights"]["tenharmsel"]}, CROSSFADE),
    "short_fade": (dict(L["weights"]), 2),
}


def test_size_rule():
    assert MM.fitted_size(1920, 1080, 1080) == (1080, 607)      # int(1080 * (1080 / 1920)) = int(607.5)
    assert MM.fitted_size(1080, 1920, 1080) == (1080, 1920)
    assert MM.fitted_size(64, 50, 48) == (48, 37)               # int(50 * 0.75) = int(37.5)
    assert MM.fitted_size(50, 64, 48, portrait=True) == (48, 61)  # int(64 * 0.96) = int(61.44): not style_morph's rule
    assert MM.fitted_size(64, 50, 48, portrait=False) == (48, 37)  # the longer side to `size`
    assert MM.fitted_size(50, 64, 48, portrait=False) == (37, 48)
    assert MM.fitted_size(50, 50, 48, portrait=False) == (48, 48)


def test_walk_file_lookup(tmp_path):
    d = tmp_path / "udnie"
    d.mkdir()
    assert MM.find_walk(d, "udnie") is None and MM.load_weights({"udnie": str(d)}) == {}
    (d / "walk.json").write_text(json.dumps({"walk": [0.1, 0.9], "weights": ["a", "b"]}))
    assert MM.find_walk(d, "udnie") == d / "walk.json"
    assert MM.load_weights({"udnie": str(d)}) == {"udnie": ["a", "b"]}
    (d / "walk_udnie.json").write_text(json.dumps({"walk": [], "weights": ["c"]}))  # `walk` is never read
    assert MM.find_walk(d, "udnie") == d / "walk_udnie.json"
    assert MM.load_weights({"udnie": str(d)}) == {"udnie": ["c"]}
    assert MM.find_walk(d, "mosaic") == d / "walk.json"  # another style's walk_<style>.json is not taken
    (d / "walk_udnie.json").write_text("{}")
    with pytest.raises(MM.UsageError, match="weights"):
        MM.load_weights({"udnie": str(d)})


def test_pulse_and_ramp_values():
    assert MM.smoothstep(0.0) == 0.0 and MM.smoothstep(1.0) == 1.0 and MM.smoothstep(0.5) == 0.5
    assert MM.smoothstep(1 / 3) == (1 / 3) * (1 / 3) * (3 - 2 * (1 / 3))
    # a pulse centre: exp(0) = 1 plus the neighbours' tails, capped at 1
    assert MM.gaussian_pulse(0.125, 4, 0.10) == 1.0 and MM.gaussian_pulse(0.875, 4, 0.10) == 1.0
    # t = 0: centres at 0.125, 0.375, 0.625, 0.875 with 2 * 0.1^2 = 0.02 below
    want = sum(math.exp(-(c * c) / 0.02) for c in (0.125, 0.375, 0.625, 0.875))
    assert MM.gaussian_pulse(0.0, 4, 0.10) == pytest.approx(want, rel=1e-12) and 0.458 < want < 0.459
    # midway between two centres: 2 exp(-0.125^2 / 0.02) = 0.9157 plus the tails at distances 0.375 and 0.625
    want = 2 * math.exp(-0.78125) + math.exp(-7.03125) + math.exp(-19.53125)
    assert MM.gaussian_pulse(0.25, 4, 0.10) == pytest.approx(want, rel=1e-9) and 0.9165 < want < 0.9166
    m, t = MM.pulse_blends(0.0)
    assert t == 0.5 and m == MM.gaussian_pulse(0.0, 4, 0.10) * 0.5  # tenharmsel runs an eighth ahead
    for p in (0.0, 0.2, 0.37, 1.0):
        assert MM.gaussian_pulse(p, 4, 0.1) == MR.gaussian_pulse(p, 4, 0.1)
    # the ramp: 6 frames over 3 rungs, two frames per rung, half a rung of progress inside each
    assert [MM.ramp_position(i, 6, 3) for i in range(6)] == [0, 0.25, 1, 1.25, 2, 2.25]
    # the defaults' 144 frames over 5 rungs: 28 frames per rung, the last 4 frames stay on rung 4
    assert MM.ramp_position(27, 144, 5) == 0 + (27 / 28) * 0.5 and MM.ramp_position(28, 144, 5) == 1
    assert MM.ramp_position(143, 144, 5) == 4 + (3 / 28) * 0.5
    # more rungs than frames: one frame per rung
    assert [MM.ramp_position(i, 3, 5) for i in range(3)] == [0, 1, 2]


def test_identity_crossfade_is_not_the_identity():
    """x * (1 - t) + x * t in float32, truncated, over the 6 steps of LAYOUT's cross-fade and every u8 value."""
    v = np.arange(256, dtype=np.float32)
    changed = 0
    for frames_from_end in range(CROSSFADE):
        t = MM.smoothstep(1 - (frames_from_end / CROSSFADE))
        changed += int((MR.trunc(v * np.float32(1 - t) + v * np.float32(t)) != np.arange(256)).sum())
    assert changed == 146


@functools.lru_cache(maxsize=None)
def _case(run):
    weights, crossfade = RUNS[run]
    weights = {k: list(v) for k, v in weights.items()}
    dirs = MR.layout_dirs("/layout")
    files = MR.layout_arrays(dirs, 12, 16)
    styled = {k: dirs[k] for k in ("udnie", "mosaic", "tenharmsel")}
    kw = dict(styled_start=L["styled_start"], styled_end=L["styled_end"], crossfade_frames=crossfade,
              hold_frames=L["hold_frames"], orig_blend=0.4, saturation=1.3)
    pl = MM.plan(dirs["orig"], styled, weights, L["total_frames"], lambda p: files.get(p) is not None,
                 lambda p: p in files, **kw)
    ref = MR.render(files, dirs["orig"], styled, weights, L["total_frames"], **kw)
    return files, pl, ref


@pytest.mark.parametrize("run", list(RUNS))
def test_plan_descriptors_equal_the_reference_loop(run):
    files, pl, ref = _case(run)
    assert [fr["frame"] for fr in pl] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]  # frame 11 has no original
    assert len(ref) == sum(fr["hold"] for fr in pl) == 22
    i = 0
    for fr in pl:
        assert len(set(fr["files"])) == len(fr["files"])  # every file once
        bank = np.stack([files[p] for p in fr["files"]])
        got = MR.evaluate(bank, fr["desc"])
        assert got.dtype == np.uint8
        for _ in range(fr["hold"]):
            assert np.array_equal(got, ref[i]), (run, fr["frame"])
            i += 1


def _descs(run):
    return {fr["frame"]: fr["desc"] for fr in _case(run)[1]}


def test_plan_covers_the_cases_the_layout_is_for():
    main, short, no_walk = _descs("main"), _descs("short_fade"), _descs("no_walk")
    S, P, N = MR.STYLED, MR.PLAIN, MR.NONE
    styled = [main[n] for n in range(4, 10)]
    assert all(d["base_kind"] == S and d["sat_on"] == 1 for d in styled)
    # one-rung and two-rung base: positions 0, 0.25, 1, 1.25, 2, 2.25; 1.25's high rung is missing, 2.25 has none above
    assert [d["base"]["hi"] >= 0 for d in styled] == [False, True, False, False, False, False]
    assert styled[1]["base"]["w_lo"] == 0.75 and styled[1]["base"]["w_hi"] == 0.25
    assert all(d["base"]["lo"] >= 0 for d in styled)
    files, pl, _ = _case("main")
    by_frame = {fr["frame"]: fr for fr in pl}
    # a missing high rung (frame 7): the low rung, udnie's second, alone
    assert by_frame[7]["files"][main[7]["base"]["lo"]].name == f"frame_0007_{MR.UDNIE[1]}.jpg"
    # a missing low rung (frame 8): the first rung that exists
    assert by_frame[8]["files"][main[8]["base"]["lo"]].name == f"frame_0008_{MR.UDNIE[0]}.jpg"
    # 0, 1 and 2 overlays; a missing overlay original (mosaic on 5, both on 6)
    assert [d["n_over"] for d in styled] == [2, 1, 0, 2, 2, 2]
    assert by_frame[5]["files"][main[5]["over"][0]["orig"]].parent.name == "tenharmsel"
    assert all(o["hi"] < 0 for d in styled for o in d["over"])
    # the unreadable tenharmsel rung of frame 9: that overlay is its copy of the original
    assert main[9]["over"][1]["lo"] < 0 and main[9]["over"][0]["lo"] >= 0
    # both fades on one frame, the cross-fade alone, the fade-in alone
    assert [(d["fin"] >= 0, d["cross_kind"]) for d in styled] == [(True, P)] * 3 + [(False, P)] * 3
    assert (short[4]["fin"] >= 0, short[4]["cross_kind"]) == (True, N)
    assert short[4]["fin_w"] == (1.0, 0.0) and main[5]["fin_w"] == (1 - MM.smoothstep(1 / 3), MM.smoothstep(1 / 3))
    # the intro cross-fades into ST(udnie, 0), which is the lo < 0 fallback there: the udnie directory's copy of the
    # original, the same pixels -- and the frame still differs from the plain original
    for n in (1, 2, 3):
        d = main[n]
        assert d["base_kind"] == P and d["sat_on"] == 0 and d["cross_kind"] == S and d["next"]["lo"] < 0
        assert by_frame[n]["files"][d["next"]["orig"]].parent.name == "udnie"
    orig1 = files[by_frame[1]["files"][0]]
    assert np.array_equal(orig1, files[by_frame[1]["files"][main[1]["next"]["orig"]]])
    assert (MR.evaluate(np.stack([files[p] for p in by_frame[1]["files"]]), main[1]) != orig1).any()
    assert main[3]["cross_w"] == (0.0, 1.0)
    # the outro: plain, no stage; the skipped frame
    assert all((main[n]["base_kind"], main[n]["sat_on"], main[n]["fin"], main[n]["cross_kind"]) == (P, 0, -1, N) for n in (10, 12))
    assert 11 not in main
    # no-udnie-walk mode: the styled section shows the originals, still saturated and faded
    for n in range(4, 10):
        d = no_walk[n]
        assert (d["base_kind"], d["n_over"], d["sat_on"], d["cross_kind"]) == (P, 0, 1, P)
    assert [no_walk[n]["fin"] >= 0 for n in range(4, 10)] == [True] * 3 + [False] * 3
    assert all(no_walk[n]["cross_kind"] == P for n in (1, 2, 3))
    # every scalar is a Python float (a np.float64 would promote the float32 frame arithmetic)
    for d in list(main.values()) + list(short.values()) + list(no_walk.values()):
        vals = list(d["keep"]) + list(d["over_w"]) + list(d["fin_w"]) + list(d["cross_w"]) + [d["sat"]]
        for s in [d["base"]] + d["over"] + ([d["next"]] if d["next"] else []):
            vals += [s["orig_w"], s["style_w"], s["w_lo"], s["w_hi"]]
        assert all(type(v) is float for v in vals)


def test_shifted_moves_every_index_and_keeps_the_absent_ones():
    d = _descs("main")[4]
    s = MM.shifted(d, 10)
    assert s["base"]["orig"] == d["base"]["orig"] + 10 and s["base"]["lo"] == d["base"]["lo"] + 10
    assert s["base"]["hi"] == -1 and s["fin"] == d["fin"] + 10 and s["next"]["orig"] == d["next"]["orig"] + 10
    assert s["next"]["lo"] == -1 and [o["lo"] for o in s["over"]] == [o["lo"] + 10 for o in d["over"]]
    assert d["base"]["orig"] == 0  # the plan's own descriptor is untouched
    assert MM.shifted(_descs("main")[10], 3)["next"] is None


# ---- exit status 2, before the device is touched (this file runs without one) ----
def _argv(dirs, out, *extra):
    return ["--orig_dir", str(dirs["orig"]), "--styled_udnie", str(dirs["udnie"]), "--styled_mosaic",
            str(dirs["mosaic"]), "--styled_tenharmsel", str(dirs["tenharmsel"]), "--output_dir", str(out),
            "--size", "48", "--fps", str(L["fps"]), "--crossfade_seconds", str(L["crossfade_seconds"]),
            "--hold_frames", str(L["hold_frames"]), "--styled_start", str(L["styled_start"]),
            "--styled_end", str(L["styled_end"]), "--total_frames", str(L["total_frames"]), *extra]


def test_prepare_accepts_the_layout(tmp_path):
    dirs = MR.write_layout(tmp_path / "in")
    args = MM.build_parser().parse_args(_argv(dirs, tmp_path / "out", "--portrait"))
    assert args.portrait is True and args.saturation == 1.3 and args.orig_blend == 0.4
    pl, target = MM.prepare(args)
    assert target == (48, 37) and [fr["frame"] for fr in pl] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]
    # the files' headers decide as the arrays of layout_arrays do
    assert [[p.relative_to(tmp_path / "in") for p in fr["files"]] for fr in pl] == \
           [[p.relative_to("/layout") for p in fr["files"]] for fr in _case("main")[1]]
    # --total_frames defaults to the number of originals: 11, so frame 12 is never reached
    argv = _argv(dirs, tmp_path / "out")
    del argv[argv.index("--total_frames"):argv.index("--total_frames") + 2]
    assert [fr["frame"] for fr in MM.prepare(MM.build_parser().parse_args(argv))[0]][-1] == 10
    defaults = MM.build_parser().parse_args(["--orig_dir", "a", "--styled_udnie", "b", "--output_dir", "c"])
    assert (defaults.styled_start, defaults.styled_end, defaults.fps, defaults.size, defaults.crossfade_seconds,
            defaults.hold_frames, defaults.total_frames, defaults.portrait) == (17, 160, 24, 1080, 2.0, 3, None, True)


def test_cli_refuses_images_of_differing_sizes(tmp_path, capsys):
    from PIL import Image
    dirs = MR.write_layout(tmp_path / "in")
    odd = dirs["udnie"] / f"frame_0005_{MR.UDNIE[0]}.jpg"
    Image.fromarray(np.zeros((30, 48, 3), np.uint8)).save(odd, format="JPEG")  # fits to 48x30, the others to 48x37
    assert MM.main(_argv(dirs, tmp_path / "out")) == 2
    assert odd.name in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_cli_refuses_a_short_tenharmsel_ladder(tmp_path, capsys):
    dirs = MR.write_layout(tmp_path / "in")
    (dirs["tenharmsel"] / "walk.json").write_text(json.dumps({"walk": [0.5], "weights": list(MR.TENHARMSEL[:5])}))
    assert MM.main(_argv(dirs, tmp_path / "out")) == 2
    assert "tenharmsel" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_cli_refuses_no_frames(tmp_path, capsys):
    dirs = MR.write_layout(tmp_path / "in")
    empty = tmp_path / "empty"
    empty.mkdir()
    argv = _argv(dict(dirs, orig=empty), tmp_path / "out")
    assert MM.main(argv) == 2
    assert "no frame_" in capsys.readouterr().err
    # an original there, but no frame the three sections name has one (the styled section reads the udnie directory's)
    (empty / "frame_0040_original.jpg").write_bytes((dirs["orig"] / "frame_0001_original.jpg").read_bytes())
    assert MM.main(argv + ["--styled_start", "20", "--styled_end", "30"]) == 2
    assert "no frames to write" in capsys.readouterr().err
    assert MM.main(_argv(dirs, tmp_path / "out", "--hold_frames", "0")) == 2
    assert not (tmp_path / "out").exists()


def test_run_log_keys(tmp_path):
    args = MM.build_parser().parse_args(["--orig_dir", "o", "--styled_udnie", "u", "--output_dir", "d", "--output",
                                         str(tmp_path / "clip.mp4")])
    p = MM.save_run_log(tmp_path / "clip.mp4", args, MM.styled_dirs_of(args), 432)
    log = json.loads(p.read_text())
    assert p.name == "clip_run.json" and log["script"] == "multi_model_video.py" and log["total_frames"] == 432
    assert log["duration_seconds"] == 18.0 and log["styled_dirs"] == {"udnie": "u"}
    assert log["parameters"] == {"orig_dir": "o", "styled_start": 17, "styled_end": 160, "fps": 24, "size": 1080,
                                 "portrait": True, "orig_blend": 0.4, "crossfade_frames": 48, "hold_frames": 3,
                                 "saturation": 1.3, "smoothness": 0.05}
