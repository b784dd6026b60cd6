"""The persistent conv kernels' tile walks at small, fast shapes (nst_set_grid_cap, a test seam).

The persistent launchers (conv_ws9, conv_ws2, conv_wst16, conv_wphase, conv_ws1s, the generic persistent form of
conv_impl.h) size their grid by the device: 256 CUs, x2 for ws9 and ws2.  A small frame has far fewer work items
(johnson 2x70x90: 36 for ws9, 30 for ws2, 6 for wst16), so without the seam no workgroup of the fast suite takes a
second work item, and the steady-state walk (double-buffered coordinate maps, the InstanceNorm table switch at a frame
boundary, the last iteration, the XCD remap with G / 8 > 1) runs in the 1080p / 4K tests only.  Engine.set_grid_cap(k)
launches at most k workgroups, so the same kernels, unchanged, walk here: every shape below has at least two tile
columns with a ragged last column and a ragged last row in every kernel of its path, and more than one frame.

  a. teacher-forced layer parity under caps 1 and 5 against oracle/bf16_layers.py, tests/layer_check.py's bars unchanged;
     the recorded grids prove the walk (n_work > blocks per kernel family);
  b. walk invariance: caps 1, 2, 5, 8, 16 give the uncapped run's outputs and captured buffers bit for bit;
  c. frame chunks (8 + 1 frames of the joined trunk conv) inside a two-workgroup walk;
  d. refusals and reset;
  f. the uncapped grid where the work exceeds the resident workgroups (8x360x640): CUs x each launcher's multiplier.
(e, the cap arithmetic without a GPU, is tests/test_host.py::test_capped_blocks.)

conv_out9 is no walk (one work item per wave); the cap reaches its slot count instead, so the number of row segments
changes.  Its accumulation order does not depend on the segment an output row falls in: output row o sums its nine
kernel rows ky = 0..8 in that order as input rows o-4 .. o+4 stream by (each row: kx, then the K blocks), into a ring
slot that was cleared after the slot's previous emission; the 8 lead-in rows of a segment only feed rows that are never
emitted.  So b holds conv_out9 to bit equality too.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import layer_check as LC
from neuralstyletransferv1_amd import _lib, synthetic
from neuralstyletransferv1_amd._lib import NstError

pytestmark = pytest.mark.gpu

SHAPES = {
    # ws9 10x3 tiles of 8x64 (76 = 9*8 + 4, 164 = 2*64 + 36); ws2 5x6 and 3x3 tiles; trunk 19x41: 3x2 tiles of 8x32
    # (41 = 32 + 9); wphase sources 19x41 and 38x82; output size == input size: the u8 path is checked too
    "johnson": (3, 76, 164, "imagenet_255"),
    # zero padding; trunk 38x45: 5x2 tiles; ConvTranspose phases
    "nst": (2, 72, 100, "raw_01"),
    # 48 / 96 / 192 channels: the narrow-input ws2, the 96 -> 48 wphase, the tanh out9 (InstanceNorm and FRN / TLU)
    "reconet": (3, 61, 90, "tanh"),
    "reconet_frn": (3, 61, 90, "tanh"),
}
WALK_MODES = (4, 5, 6, 7, 8)   # wst16, wphase, ws2, ws9, ws1s (nst_op_desc.kernel_mode)
# conv_out9.hip's instantiations: (strip width = 32 G, waves per workgroup NW) of the net's output conv
OUT9 = {"johnson": (96, 8), "nst": (96, 8), "reconet": (32, 8), "reconet_frn": (32, 8)}


@functools.lru_cache(maxsize=None)
def _net(arch, dtype, seed=11, ksel=()):
    m = synthetic.build_module(arch)
    m.load_state_dict(synthetic.make_state_dict(arch, seed))
    m = m.to("cuda").eval()
    m.compute_dtype = dtype
    m.kernel_select = frozenset(ksel)
    return m


@functools.lru_cache(maxsize=None)
def _frames(n, h, w):
    return synthetic.make_frames(n, h, w, seed=40 + h)


@contextlib.contextmanager
def _capped(eng, k):
    eng.set_grid_cap(k)
    try:
        yield
    finally:
        eng.set_grid_cap(0)


def _capture(eng, frames_u8):
    """-> (y f32, y u8, ops, caps) of one batch under the engine's current cap."""
    x = torch.from_numpy(frames_u8).to(eng.device)
    arch = {0: "johnson", 1: "nst"}[eng.arch]
    preset = SHAPES[arch][3]
    y, ops, caps = eng.forward_capture(x, "u8", preset, "f32")
    y8, ops8, _ = eng.forward_capture(x, "u8", preset, "u8")
    torch.cuda.synchronize()
    return y, y8, ops, caps, ops8


def _out9_items(slots, n, oh, ow, sw):
    """conv_out9.hip's launcher restated: work items = frames x row segments x column strips."""
    strips = -(-ow // sw)
    nseg = max(1, slots // max(1, n * strips))
    nseg = min(nseg, max(1, oh // 16))
    seg_len = -(-oh // nseg)
    nseg = -(-oh // seg_len)
    return n * nseg * strips


def _report(recs):
    for r in recs:
        print({k: (round(v, 7) if isinstance(v, float) else v) for k, v in r.items()})


@pytest.mark.parametrize("cap", [1, 5])
@pytest.mark.parametrize("arch,dtype,ksel", [
    ("johnson", "bf16", ()), ("johnson", "fp16", ()),
    ("johnson", "fp16m", ()),  # conv_ws1s and the split ws9 / ws2 variants
    ("nst", "bf16", ()), ("reconet", "bf16", ()), ("reconet_frn", "bf16", ()),
    # the generic persistent form (VAR_PERS of conv_impl.h): its only instantiations are the bf16 128 -> 128 trunk
    # convs (conv_bf16_wl.hip, 16x16 tiles: 2x3 on the 19x41 trunk), which serve the trunk when conv_wst16 is
    # deselected; the ReCoNet nets run no persistent generic kernel (their walking kernels are ws2 and wphase)
    ("johnson", "bf16", ("no_wstat",)),
], ids=lambda v: ("-".join(v) or "default") if isinstance(v, tuple) else None)
def test_layers_under_cap(arch, dtype, ksel, cap):
    """Every layer against the CPU oracle while one workgroup (cap 1) walks every work item of every frame in order,
    and while five do (cap 5: the johnson trunk's 18 items split 4/4/4/3/3, so the last iteration comes at a different
    step in different workgroups).  The recorded grids prove the walk: n_work > blocks for every walking kernel family
    present; conv_out9 is held to its launcher's arithmetic under the cap (at cap 1 one segment per strip instead of
    the uncapped run's oh / 16; at cap 5 the 5 x 8 wave slots still allow oh / 16 segments at these shapes, so the
    count is the uncapped one and only the restated arithmetic shows that the cap was applied)."""
    n, h, w, preset = SHAPES[arch]
    frames = _frames(n, h, w)
    net = _net(arch, dtype, ksel=ksel)
    eng = net.engine()
    _, base, _ = eng.forward_capture(torch.from_numpy(frames).to(eng.device), "u8", preset, "f32")
    with _capped(eng, cap):
        recs = LC.check_layers(net, frames, preset, acc=torch.float64)
    _report(recs)
    convs = [r for r in recs if r["mode"] >= 0]
    modes = {r["mode"] for r in convs}
    if arch == "johnson":
        assert {3, 5, 6, 7} <= modes and ((4 in modes) == (not ksel)) and ((8 in modes) == (dtype == "fp16m")), modes
    pers = [r for r in convs if r["launches"] > 0 and r["mode"] != 3]
    assert pers
    for r in pers:  # the cap reached every persistent launcher
        assert r["launches"] == 1 and r["blocks"] == min(r["n_work"], cap), r
    for m in WALK_MODES:
        if m in modes:
            assert any(r["n_work"] > r["blocks"] for r in pers if r["mode"] == m), (m, pers)
    generic = [r for r in pers if r["mode"] in (0, 1, 2)]  # the generic persistent form (VAR_PERS of conv_impl.h)
    assert bool(generic) == bool(ksel), generic
    if ksel:
        assert len(generic) == 10 and all(r["n_work"] > r["blocks"] for r in generic), generic
    # conv_out9: the cap changes the segment count (n_work = frames x segments x strips; frames and strips are fixed)
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    sw, nw = OUT9[arch]
    out9 = [r for r in convs if r["mode"] == 3]
    assert len(out9) == 1
    r = out9[0]
    d = base[r["op"]]
    assert d["grid"]["n_work"] == _out9_items(cus * nw, n, d["out_h"], d["out_w"], sw), d
    assert r["n_work"] == _out9_items(cap * nw, n, d["out_h"], d["out_w"], sw), (r, d)
    if cap == 1:
        assert r["n_work"] != d["grid"]["n_work"], (r, d["grid"])


@pytest.mark.parametrize("arch,dtype,ksel", [
    ("johnson", "bf16", ()), ("johnson", "fp16", ()), ("nst", "bf16", ()), ("nst", "fp16", ()),
    ("johnson", "bf16", ("no_wstat",)),  # the trunk on the generic persistent kernels (mode 0)
], ids=lambda v: ("-".join(v) or "default") if isinstance(v, tuple) else None)
def test_walk_invariance(arch, dtype, ksel):
    """Which workgroup computes a work item does not reach its arithmetic: every kernel writes per-tile partial sums
    that are reduced in fixed order, and conv_out9 sums each output row's taps in the same order in any segment (module
    docstring).  So under caps 1, 2, 5, 8, 16 (8 and 16: the G % 8 == 0 XCD remap with G / 8 = 1 and 2) the f32 and
    u8 outputs and every captured activation, residual stream and InstanceNorm table equal the uncapped run's bit for
    bit."""
    n, h, w, _ = SHAPES[arch]
    frames = _frames(n, h, w)
    eng = _net(arch, dtype, ksel=ksel).engine()
    y0, y80, ops0, caps0, _ = _capture(eng, frames)
    assert all(d["grid"]["blocks"] == d["grid"]["n_work"] for d in ops0 if d["grid"]["launches"] and
               d["kernel_mode"] != 3), "uncapped: one work item per workgroup at this shape"
    for cap in (1, 2, 5, 8, 16):
        with _capped(eng, cap):
            y, y8, ops, caps, _ = _capture(eng, frames)
        walked = [d for d in ops if d["grid"]["launches"] and d["kernel_mode"] != 3 and
                  d["grid"]["n_work"] > d["grid"]["blocks"]]
        assert walked and all(d["grid"]["blocks"] == cap for d in walked), (cap, [d["grid"] for d in ops])
        if ksel:
            assert sum(1 for d in walked if d["kernel_mode"] == 0) == 10, (cap, [d["grid"] for d in ops])
        assert torch.equal(y, y0), (cap, "f32 output", int((y != y0).sum()))
        assert torch.equal(y8, y80), (cap, "u8 output", int((y8 != y80).sum()))
        for i, (c, c0) in enumerate(zip(caps, caps0)):
            for key in ("act", "res", "stats"):
                if c0[key] is not None:
                    same = torch.equal(c[key], c0[key])
                    assert same, (cap, i, key, ops[i]["kernel_mode"], ops[i]["grid"],
                                  (c[key] != c0[key]).nonzero()[:4].tolist())


def test_frame_chunks_inside_a_walk():
    """9 frames under cap 2: the joined trunk kernel holds 8 frames' InstanceNorm tables per launch, so it runs chunks
    of 8 + 1 frames, the first walked by two workgroups across frame boundaries.  Frames 0, 7 and 8 equal their own
    single-frame uncapped runs bit for bit (per-frame InstanceNorm, deterministic kernels)."""
    eng = _net("johnson", "bf16").engine()
    frames = synthetic.make_frames(9, 40, 56, seed=31)
    with _capped(eng, 2):
        y, y8, ops, caps, _ = _capture(eng, frames)
    joined = [i for i, d in enumerate(ops) if d["kernel_mode"] == 4 and d["res_buf"] >= 0]
    assert joined
    for i, d in enumerate(ops):
        g = d["grid"]
        if d["kernel_mode"] not in WALK_MODES:
            continue
        if i in joined or d["kernel_mode"] == 5:  # the up-convs hold 8 frames' tables per launch too
            assert g["launches"] == 2, (i, g)
            (b0, w0), (b1, w1) = g["per_launch"]
            assert w0 == 8 * w1 and b0 == 2 and w0 > b0 and b1 == min(2, w1), (i, g)
        else:  # one launch, walked by two workgroups
            assert g["launches"] == 1 and g["blocks"] == 2 and g["n_work"] > 2, (i, d["kernel_mode"], g)
    for i in (0, 7, 8):
        ys, y8s, _, cs, _ = _capture(eng, frames[i:i + 1])
        assert torch.equal(ys[0], y[i]) and torch.equal(y8s[0], y8[i]), i
        for j, (c, c1) in enumerate(zip(caps, cs)):
            for key in ("act", "res", "stats"):
                if c[key] is not None:
                    assert torch.equal(c[key][i], c1[key][0]), (i, j, key)


def test_stream_split_sees_the_cap():
    """nst_forward with the batch split over the library's internal streams (3 frames as 2 + 1): every sub-batch is
    launched under the handle's cap (the record keeps the last sub-batch's grids: one frame's work items on two
    workgroups), and the frames equal the whole, uncapped batch's."""
    n, h, w, preset = SHAPES["johnson"]
    eng = _net("johnson", "bf16").engine()
    x = torch.from_numpy(_frames(n, h, w)).to(eng.device)
    want = eng.stylize_u8(x, preset)
    whole = [g["n_work"] for g in eng.op_grids()]
    eng.set_stream_split(2)
    try:
        with _capped(eng, 2):
            got = eng.stylize_u8(x, preset)
            grids = eng.op_grids()
    finally:
        eng.set_stream_split(1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    modes = [d["kernel_mode"] for d in eng.op_descs(1, h, w)]
    walking = [(g, k) for g, k, m in zip(grids, whole, modes) if m in WALK_MODES]
    assert len(walking) == 15
    for g, k in walking:
        assert g["launches"] == 1 and g["blocks"] == 2 and g["n_work"] * n == k and g["n_work"] > 2, (g, k)


# Workgroups per CU of each walking op's uncapped grid (blocks = CUs x k once the work exceeds it), by layer name.
# Recorded from a run of test_resident_grids on the commit before the launchers moved onto csrc/conv_launch.h, and
# cross-checked against the launchers' own arithmetic: conv_ws9 8 / NW = 2 (four-wave workgroups); conv_ws2
# OCC * 4 / NW per instantiation (bf16 32 -> 64: 4 * 4 / 8 = 2; 64 -> 128: 2 * 4 / 8 = 1; ReCoNet's 64 -> 96:
# 3 * 4 / 12 = 1; the split-precision ones: 2 * 4 / 8 = 1); conv_wst16, conv_wphase and conv_ws1s one workgroup per
# CU; the generic persistent kernel its occupancy (one 512-thread workgroup per CU: its LDS weight ring).
_TRUNK = [f"res{i}.conv{j}.conv2d" for i in range(1, 6) for j in (1, 2)]
_JOHNSON_K = {"conv1.conv2d": 2, "conv2.conv2d": 2, "conv3.conv2d": 1, **{name: 1 for name in _TRUNK},
              "deconv1.conv2d": 1, "deconv2.conv2d": 1}
RESIDENT_K = {
    ("johnson", "bf16", ()): _JOHNSON_K,
    ("johnson", "fp16m", ()): {**_JOHNSON_K, "conv2.conv2d": 1},  # the split-operand conv2: OCC 2
    ("johnson", "bf16", ("no_wstat",)): _JOHNSON_K,               # the trunk on the generic persistent kernel
    # conv_ws9 (48 channels padded to 64), the narrow-input conv_ws2 (64 -> 96), conv_wphase (96 -> 48)
    ("reconet", "bf16", ()): {"encoder.layers.0.layers.0.layers.1": 2, "encoder.layers.1.layers.0.layers.1": 1,
                              "decoder.layers.3.layers.0.layers.1": 1},
}
RESIDENT_SHAPE = (8, 360, 640)  # johnson's trunk: a 90x160 map in 8x32 tiles, 12 * 5 * 8 = 480 work items on 256 CUs


@pytest.mark.parametrize("arch,dtype,ksel", list(RESIDENT_K),
                         ids=lambda v: ("-".join(v) or "default") if isinstance(v, tuple) else None)
def test_resident_grids(arch, dtype, ksel):
    """The uncapped grid once the work exceeds the resident slots: CUs x the launcher's workgroups per CU (RESIDENT_K),
    for every walking op of the net.  The small shapes above never reach it (blocks = n_work there), and a slip in it,
    such as conv_ws9 losing its x2, changes speed and nothing else.  8 x 360 x 640 is the smallest batch of the common
    frame sizes at which every walking op of these nets has more work items than resident workgroups."""
    n, h, w = RESIDENT_SHAPE
    eng = _net(arch, dtype, ksel=ksel).engine()
    x = torch.from_numpy(_frames(n, h, w)).to(eng.device)
    eng.stylize_u8(x, SHAPES[arch][3])
    torch.cuda.synchronize()
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    names = eng.layer_names()
    want = RESIDENT_K[(arch, dtype, ksel)]
    seen = {}
    for d, g in zip(eng.op_descs(n, h, w), eng.op_grids()):
        if g["launches"] and d["kernel_mode"] != 3:  # conv_out9 reports its grid too, and does not walk
            print(names[d["layer"]], "mode", d["kernel_mode"], "kdt", d["kernel_dtype"], g, "CUs", cus)
            seen[names[d["layer"]]] = (d["kernel_mode"], g)
    assert set(seen) == set(want), (sorted(seen), sorted(want))
    for name, (mode, g) in seen.items():
        assert mode in WALK_MODES + (0,), (name, mode)
        for blocks, n_work in g["per_launch"]:
            assert n_work > blocks and blocks == cus * want[name], (name, mode, g, cus, want[name])
    modes = {m for m, _ in seen.values()}
    if arch == "johnson":
        assert {5, 6, 7} <= modes and ((4 in modes) == (not ksel)) and ((0 in modes) == bool(ksel)) and \
            ((8 in modes) == (dtype == "fp16m")), modes


def test_refusals_and_reset():
    eng = _net("johnson", "bf16").engine()
    with pytest.raises(NstError):
        eng.set_grid_cap(-1)
    L = _lib.lib()
    assert L.nst_set_grid_cap(None, 1) == _lib.NST_E_INVALID
    assert L.nst_op_last_grid(None, 0, None, None, None) == _lib.NST_E_INVALID
    assert L.nst_op_launch_grid(None, 0, 0, None, None) == _lib.NST_E_INVALID
    n, h, w, preset = SHAPES["johnson"]
    x = torch.from_numpy(_frames(n, h, w)).to(eng.device)
    fresh = _net("johnson", "bf16", 12).engine()  # another handle: never capped
    want = [d["grid"] for d in fresh.forward_capture(x, "u8", preset, "f32")[1]]
    eng.set_grid_cap(3)
    capped = [d["grid"] for d in eng.forward_capture(x, "u8", preset, "f32")[1]]
    eng.set_grid_cap(0)
    got = [d["grid"] for d in eng.forward_capture(x, "u8", preset, "f32")[1]]
    torch.cuda.synchronize()
    assert capped != want and max(g["blocks"] for g, d in zip(capped, eng.op_descs(n, h, w)) if d["kernel_mode"] != 3) == 3
    assert got == want
    # a launch index past the op's launches, an op past the program
    b, k, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.nst_op_launch_grid(eng._h, 0, got[0]["launches"], ctypes.byref(b), ctypes.byref(k)) == _lib.NST_E_INVALID
    assert L.nst_op_last_grid(eng._h, len(got), ctypes.byref(b), ctypes.byref(k), ctypes.byref(m)) == _lib.NST_E_INVALID
