"""Torch7 .t7 fast-style nets on the engine (NST_ARCH_TORCH7_IN / _BN) against the independent torch-CPU interpreter
of the same file (tests/t7_ref.py).  Parity with OpenCV DNN itself is unpinned (no cv2, no published .t7 here).

Bars: the project's own (tests/test_gpu_parity.py): fp32 (and the split-fp16 mode) +-1 LSB on the frames with under
1 % of values differing and 1e-4 of the output's magnitude on the raw forward; bf16 SSIM >= BF16_SSIM_MIN; fp16
+-1 LSB on >= 99.9 % of values, never more than 3.

Shapes: 48x64 and 64x48 (one tile), 50x70 (ragged: output 52x72, fitted back), 136x200 (several tiles; the trunk map
shrinks 54x70 -> 34x50).  Every case is a batch of two different frames.
"""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

import t7_ref as R
import t7_write as W
from neuralstyletransferv1_amd import pipeline as P
from neuralstyletransferv1_amd import synthetic
from neuralstyletransferv1_amd._lib import NstError
from neuralstyletransferv1_amd.torch7 import Torch7Net
from oracle import nst_oracle as O
from test_gpu_parity import BF16_SSIM_MIN, F16_MAX_LSB, F16_WITHIN1_MIN, FP32_REL_TOL

pytestmark = pytest.mark.gpu

SHAPES = [(48, 64), (64, 48), (50, 70), (136, 200)]
# output-conv scale per norm kind, chosen on the CPU so the oracle's frames are not saturated (pre-tanh std ~0.35)
OUT_SCALE = {"in": 0.4, "bn": 0.6}
VARIANT = {"in": "in_legacy_2d_tv", "bn": "bn_std_legacy_2d"}
MAX_SATURATED = 0.10


@functools.lru_cache(maxsize=None)
def _file(kind):
    return W.make_file_bytes(VARIANT[kind], seed=0, out_scale=OUT_SCALE[kind])[0]


@functools.lru_cache(maxsize=None)
def _root(kind):
    return R.load(_file(kind))


@functools.lru_cache(maxsize=None)
def _net_cached(kind, tmp):
    p = tmp / f"{kind}.t7"
    p.write_bytes(_file(kind))
    return Torch7Net.from_t7(str(p)).cuda().eval()


@pytest.fixture(scope="module")
def t7dir(tmp_path_factory):
    return tmp_path_factory.mktemp("t7")


def _net(kind, dtype, t7dir):
    m = _net_cached(kind, t7dir)
    m.compute_dtype = dtype
    return m


def _frames(shape):
    return synthetic.make_frames(2, shape[0], shape[1], seed=100 + shape[0])


@functools.lru_cache(maxsize=None)
def _ref(kind, shape):
    """The oracle, once per case: (raw forward tanh * c, uint8 frames fitted to the content size), read-only."""
    fr = _frames(shape)
    y = R.forward(_root(kind), R.blob(fr))
    u8 = R.stylize_u8(_root(kind), fr)
    y.setflags(write=False)
    u8.setflags(write=False)
    sat = R.saturated_fraction(R.frames_of(y))
    assert sat < MAX_SATURATED, f"oracle frames saturated: {sat:.3f}"
    return y, u8


CASES = [(k, s) for k in ("in", "bn") for s in SHAPES]
IDS = [f"{k}-{s[0]}x{s[1]}" for k, s in CASES]


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
def test_fp32_frames_and_forward_vs_oracle(kind, shape, dtype, t7dir):
    yr, ref = _ref(kind, shape)
    fr = _frames(shape)
    net = _net(kind, dtype, t7dir)
    out = net.stylize_frames(torch.from_numpy(fr).cuda()).cpu().numpy()
    assert out.shape == fr.shape
    d = np.abs(out.astype(int) - ref.astype(int))
    y = net(torch.from_numpy(R.blob(fr)).cuda()).cpu().numpy()
    assert y.shape == yr.shape
    rel = np.abs(y - yr).max() / np.abs(yr).max()
    print(f"{kind} {shape} {dtype}: frames max {d.max()} LSB, differing {(d > 0).mean():.5f}; forward rel {rel:.3e}")
    assert d.max() <= 1 and (d > 0).mean() < 0.01, (d.max(), (d > 0).mean())
    assert rel <= FP32_REL_TOL, rel


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_bf16_ssim_vs_oracle(kind, shape, t7dir):
    """Measured on MI355X (both frames of each case): see DESIGN.md, "Torch7 .t7 nets"."""
    _, ref = _ref(kind, shape)
    out = _net(kind, "bf16", t7dir).stylize_frames(torch.from_numpy(_frames(shape)).cuda()).cpu().numpy()
    s = [O.ssim(out[i], ref[i]) for i in range(2)]
    print(f"{kind} {shape} bf16: ssim {s[0]:.5f} {s[1]:.5f}")
    assert min(s) >= BF16_SSIM_MIN, s


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_fp16_vs_oracle(kind, shape, t7dir):
    _, ref = _ref(kind, shape)
    out = _net(kind, "fp16", t7dir).stylize_frames(torch.from_numpy(_frames(shape)).cuda()).cpu().numpy()
    d = np.abs(out.astype(int) - ref.astype(int))
    print(f"{kind} {shape} fp16: max {d.max()} LSB, within 1 LSB {(d <= 1).mean():.6f}")
    assert d.max() <= F16_MAX_LSB and (d <= 1).mean() >= F16_WITHIN1_MIN, (d.max(), (d <= 1).mean())


@pytest.mark.parametrize("kind", ["in", "bn"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frame_alone_equals_frame_in_batch_and_runs_repeat(kind, dtype, t7dir):
    """Frames are independent (InstanceNormalization statistics are per frame) and the arithmetic has a fixed order:
    a frame alone equals the same frame inside a batch, and two runs are bit-identical (frames and raw forward)."""
    net = _net(kind, dtype, t7dir)
    for shape in ((50, 70), (136, 200)):
        f = torch.from_numpy(_frames(shape)).cuda()
        both = net.stylize_frames(f)
        assert torch.equal(both, net.stylize_frames(f))
        for i in range(2):
            assert torch.equal(net.stylize_frames(f[i:i + 1].contiguous())[0], both[i]), (shape, i)
        x = torch.from_numpy(R.blob(_frames(shape))).cuda()
        y = net(x)
        assert torch.equal(y, net(x))
        assert torch.equal(net(x[1:2].contiguous())[0], y[1])


@pytest.mark.parametrize("kind", ["in", "bn"])
def test_capture_u8_replay_matches_eager(kind, t7dir):
    """The whole forward (tail kernel, and at the ragged size the content-size fit) captures into a HIP graph; a
    replay over the refilled input buffer equals the eager forward of the new frames."""
    from neuralstyletransferv1_amd.engine import capture_u8
    eng = _net(kind, "bf16", t7dir).engine(torch.device("cuda", 0))
    for shape in ((136, 200), (50, 70)):
        a = torch.from_numpy(_frames(shape)).cuda()
        b = torch.from_numpy(synthetic.make_frames(2, shape[0], shape[1], seed=9)).cuda()
        frames = a.clone()
        replay, out = capture_u8(eng, frames, "caffe_bgr")
        replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eng.stylize_u8(a))
        frames.copy_(b)
        replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eng.stylize_u8(b))


@pytest.mark.parametrize("kind", ["in", "bn"])
def test_small_frame_raises_before_launch(kind, t7dir):
    """min(H, W) <= 40: the reflection needs pad < side.  Refused by the engine's plan, before any kernel runs."""
    net = _net(kind, "fp32", t7dir)
    eng = net.engine(torch.device("cuda", 0))
    for h, w in ((40, 64), (64, 40)):
        with pytest.raises(NstError):
            eng.output_hw(h, w)
        with pytest.raises(NstError):
            net.stylize_frames(torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda"))
        with pytest.raises(NstError):
            net(torch.zeros((1, 3, h, w), device="cuda"))
    assert eng.output_hw(41, 64) == (44, 64)
    with pytest.raises(NstError):  # the split-precision head is not built for these nets: a clear error
        _net(kind, "fp16m", t7dir).engine(torch.device("cuda", 0))
    torch.cuda.synchronize()


def test_cli_single_image_writes_the_engines_frame(tmp_path, t7dir):
    fr = synthetic.make_frames(1, 64, 96, seed=21)
    inp, outp, model = tmp_path / "in.png", tmp_path / "out.png", tmp_path / "a.t7"
    Image.fromarray(fr[0]).save(inp)
    model.write_bytes(_file("in"))
    assert P.main(["--input_image", str(inp), "--output_image", str(outp), "--model", str(model),
                   "--no-smooth_lightness", "--work_dir", str(tmp_path / "w")]) == 0
    want = _net("in", "fp32", t7dir).stylize_frames(torch.from_numpy(fr).cuda()).cpu().numpy()[0]
    assert np.array_equal(np.array(Image.open(outp)), want)
    d = np.abs(want.astype(int) - R.stylize_u8(_root("in"), fr)[0].astype(int))
    assert d.max() <= 1


def test_cli_blend_of_a_pth_slot_and_a_t7_slot(tmp_path):
    """--model a.pth --model_b b.t7: out = clamp(0.5 * out01_A + 0.5 * out01_B) with B's out01 = frame / 255 fitted to
    the content size (pipeline.py:1443, 1512-1516, 1872-1879), at a ragged size (B's output is 52x72)."""
    sd = synthetic.make_state_dict("johnson", 0)
    ck, model_b = tmp_path / "a.pth", tmp_path / "b.t7"
    torch.save(sd, ck)
    model_b.write_bytes(_file("bn"))
    fr = synthetic.make_frames(1, 50, 70, seed=33)
    inp, outp = tmp_path / "in.png", tmp_path / "out.png"
    Image.fromarray(fr[0]).save(inp)
    assert P.main(["--input_image", str(inp), "--output_image", str(outp), "--model", str(ck), "--model_b", str(model_b),
                   "--blend_models_weights", "0.5,0.5", "--io_preset", "imagenet_255", "--no-smooth_lightness",
                   "--work_dir", str(tmp_path / "w")]) == 0
    with torch.no_grad():
        ya = O.FORWARDS["johnson"](sd, O.encode(O.to_tensor01(fr), "imagenet_255"))
        a01 = O.fit_to_content(O.decode(ya, "imagenet_255"), 50, 70)
    b01 = R.out01(_root("bn"), fr)
    assert R.saturated_fraction(R.to_u8(b01)) < MAX_SATURATED
    acc = torch.zeros_like(a01)
    acc += np.float32(0.5) * a01
    acc += np.float32(0.5) * b01
    ref = R.to_u8(acc.clamp(0, 1))[0]
    d = np.abs(np.array(Image.open(outp)).astype(int) - ref.astype(int))
    print(f"blend: max {d.max()} LSB, differing {(d > 0).mean():.5f}")
    assert d.max() <= 1


def test_cli_bad_t7_in_slot_b_exits_2(tmp_path):
    ck, bad = tmp_path / "a.pth", tmp_path / "b.t7"
    torch.save(synthetic.make_state_dict("johnson", 0), ck)
    bad.write_bytes(_file("bn")[:50000])
    fr = synthetic.make_frames(1, 48, 64, seed=1)
    inp = tmp_path / "in.png"
    Image.fromarray(fr[0]).save(inp)
    with pytest.raises(SystemExit) as e:
        P.main(["--input_image", str(inp), "--output_image", str(tmp_path / "out.png"), "--model", str(ck),
                "--model_b", str(bad), "--work_dir", str(tmp_path / "w")])
    assert e.value.code == 2
    assert not (tmp_path / "out.png").exists()
