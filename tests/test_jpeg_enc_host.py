"""The JPEG writer without a GPU: tests/jpeg_enc_ref.py (the arithmetic csrc/jpeg_enc.hip runs on the device,
restated in numpy) must write Pillow's files byte for byte, the new exports must reject bad arguments before any GPU
call, and the CLI flag must parse."""
import ctypes

import pytest

import jpeg_enc_ref as E
from jpeg_ref import content, encode
from neuralstyletransferv1_amd import _lib

# (h, w): (17, 33) has dummy luma blocks both ways, (40, 24) a partial chroma block row, (50, 70) an odd chroma row
# count; the small ones are all edge replication
SHAPES = [(1, 1), (2, 4), (3, 5), (8, 8), (9, 6), (16, 16), (17, 33), (40, 24), (50, 70), (31, 47)]
QUALITIES = (1, 30, 85, 95, 100)
KINDS = ("noise", "smooth")

_cache = {}


def _case(hw, q, kind):
    key = (hw, q, kind)
    if key not in _cache:
        rgb = content(kind, *hw)
        _cache[key] = (E.encode(rgb, q), encode(rgb, quality=q))
    return _cache[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pillow(hw, q, kind):
    got, want = _case(hw, q, kind)
    assert got.data == want


def test_cases_reach_the_hard_symbols():
    enc = [_case(hw, q, kind)[0] for hw in SHAPES for q in QUALITIES for kind in KINDS]
    assert any(e.zrl > 0 for e in enc), "no case emits a ZRL"
    assert any(e.stuffed > 0 for e in enc), "no case stuffs a 0xFF"
    assert any(e.pad_bits > 0 for e in enc), "no case ends on a padded byte"
    assert any(e.pad_bits == 0 for e in enc), "no case ends on a byte boundary"


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("hw", [(1, 1), (50, 70), (1080, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_equals_pillows(hw, q):
    want = encode(content("smooth", *hw), quality=q)
    hd = E.header(hw[0], hw[1], q)
    assert len(hd) == 623 and want[:len(hd)] == hd
    assert hd[-14:-12] == b"\xff\xda"  # up to and including SOS


def _bound(h, w):
    b = ctypes.c_size_t()
    rc = _lib.lib().nst_jpeg_enc_bound(h, w, ctypes.byref(b))
    return rc, b.value


def test_bound_follows_its_derivation():
    # 1,660 bits per block at most, every byte stuffed, 623 header bytes and EOI, rounded up to 16
    for h, w, blocks in ((1, 1, 6), (50, 70, 4 * 5 * 6), (1080, 1920, 48960)):
        rc, b = _bound(h, w)
        assert rc == 0
        raw = 623 + 2 * -(-blocks * 1660 // 8) + 2
        assert b == -(-raw // 16) * 16


def test_exports_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    out = ctypes.c_size_t()
    for h, w in ((0, 8), (8, 0), (-1, 8), (8, 65536)):
        assert _bound(h, w)[0] == _lib.NST_E_INVALID
        assert b"nst_jpeg_enc_bound" in L.nst_last_error()
        assert L.nst_jpeg_enc_workspace_bytes(1, h, w, ctypes.byref(out)) == _lib.NST_E_INVALID
    assert L.nst_jpeg_enc_bound(8, 8, None) == _lib.NST_E_INVALID
    assert L.nst_jpeg_enc_workspace_bytes(0, 8, 8, ctypes.byref(out)) == _lib.NST_E_INVALID
    assert L.nst_jpeg_enc_workspace_bytes(1, 8, 8, None) == _lib.NST_E_INVALID
    assert b"nst_jpeg_enc_workspace_bytes" in L.nst_last_error()
    assert L.nst_jpeg_enc_workspace_bytes(2, 50, 70, ctypes.byref(out)) == 0 and out.value > 0
    wsb = out.value
    # never dereferenced: every call below must fail before any GPU call (there is no GPU here)
    p = 0x1000
    ok = dict(frames=p, n=2, h=50, w=70, quality=85, out=p, out_stride=4096, sizes=p, workspace=p,
              workspace_bytes=wsb, stream=None)
    bad = [dict(frames=None), dict(out=None), dict(sizes=None), dict(workspace=None), dict(n=0), dict(n=-3),
           dict(h=0), dict(w=0), dict(quality=0), dict(quality=101), dict(out=p + 8), dict(out_stride=4104),
           dict(out_stride=0), dict(workspace_bytes=wsb - 1), dict(workspace_bytes=0)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.nst_jpeg_encode_u8(a["frames"], a["n"], a["h"], a["w"], a["quality"], a["out"], a["out_stride"],
                                  a["sizes"], a["workspace"], a["workspace_bytes"], a["stream"])
        assert rc == _lib.NST_E_INVALID, change
        assert b"nst_jpeg_encode_u8" in L.nst_last_error(), change


def test_jpeg_writer_flag_parses():
    from neuralstyletransferv1_amd import pipeline as P
    base = ["--input_video", "x", "--output_video", "y"]
    assert P.build_parser().parse_args(base).jpeg_writer == "pil"
    assert P.build_parser().parse_args(base + ["--jpeg_writer", "gpu"]).jpeg_writer == "gpu"
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(base + ["--jpeg_writer", "fast"])


def test_jpegio_has_no_cpu_path():
    import numpy as np
    import torch

    from neuralstyletransferv1_amd import jpegio
    with pytest.raises(_lib.NstError):
        jpegio.encode_jpeg_gpu(torch.from_numpy(np.zeros((1, 8, 8, 3), np.uint8)), 85)
