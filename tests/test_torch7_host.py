"""Torch7 .t7 support on the host: the reader, the matcher and the CLI's back-end selection (no GPU needed)."""
import numpy as np
import pytest
import torch

import t7_ref as R
import t7_write as W
from neuralstyletransferv1_amd import pipeline as P
from neuralstyletransferv1_amd import torch7 as T7
from neuralstyletransferv1_amd._lib import NstError


@pytest.fixture(scope="module")
def files():
    """variant -> (bytes, canonical parameters written)"""
    return {v: W.make_file_bytes(v, seed=3) for v in W.VARIANTS}


def _small_tree(versioned=True):
    """A few hundred bytes holding every construct of the format: nested tables, shared tensors, an empty tensor,
    numbers, strings, booleans, nil."""
    w = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    inner = W.Obj("nn.SpatialBatchNormalization", {"weight": w, "eps": 1e-5, "affine": True}, versioned)
    return W.Obj("nn.Sequential", {"modules": [W.Obj("nn.InstanceNormalization",
                                                      {"weight": w, "bn": inner, "name": "n", "gone": None,
                                                       "output": W.Empty(), "idx": torch.tensor([4, 5])}, versioned)],
                                   "train": False}, versioned)


@pytest.mark.parametrize("variant", sorted(W.VARIANTS))
def test_reader_round_trip(files, variant):
    """Every tensor, number and flag the writer put in comes back, through every header and layout variant."""
    data, Pw = files[variant]
    root = T7.read_t7_bytes(data)
    assert root.torch_class == "nn.Sequential"
    assert root.version == (0 if "legacy" in variant else 1)
    mods = root.get("modules")
    assert sorted(mods) == list(range(1, len(mods) + 1))
    assert mods[1].torch_class == "nn.SpatialReflectionPadding" and mods[1].get("pad_l") == 40
    conv = mods[2]
    w = conv.get("weight")
    assert w.dtype == torch.float32
    assert tuple(w.shape) == ((32, 243) if "2d" in variant else (32, 3, 9, 9))
    assert torch.equal(w.reshape(32, 3, 9, 9), Pw["down1.conv.weight"])
    assert torch.equal(conv.get("bias"), Pw["down1.conv.bias"])
    assert conv.get("train") is False and conv.get("output").numel() == 0
    assert mods[len(mods) - (1 if variant.endswith("tv") else 0)].get("constant_scalar") == 150.0
    assert (mods[len(mods)].torch_class == "nn.TotalVariation") == variant.endswith("tv")
    up = mods[16]
    assert up.torch_class == "nn.SpatialFullConvolution" and tuple(up.get("weight").shape) == (128, 64, 3, 3)


def test_shared_references_resolve_to_one_object(files):
    root = T7.read_t7_bytes(files["in"][0])
    norm = root.get("modules")[3]
    assert norm.torch_class == "nn.InstanceNormalization"
    assert norm.get("bn").get("weight") is norm.get("weight")
    assert norm.get("bn").get("bias") is norm.get("bias")
    small = T7.read_t7_bytes(W.dumps(_small_tree()))
    n = small.get("modules")[1]
    assert n.get("bn").get("weight") is n.get("weight")
    assert n.get("gone") is None and n.get("name") == "n" and n.get("idx").tolist() == [4, 5]
    assert n.get("weight").tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]


@pytest.mark.parametrize("versioned", [True, False])
def test_every_truncation_raises(versioned):
    data = W.dumps(_small_tree(versioned))
    assert len(data) < 2000
    T7.read_t7_bytes(data)
    for n in range(len(data)):
        with pytest.raises(NstError):
            T7.read_t7_bytes(data[:n])


def test_damaged_input_raises_cleanly():
    data = bytearray(W.dumps(_small_tree()))
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(300):  # any outcome but an NstError or a parsed object is a failure (no other exception, no over-read)
        d = bytearray(data)
        for _ in range(3):
            d[int(rng.integers(len(d)))] = int(rng.integers(256))
        try:
            T7.read_t7_bytes(bytes(d))
        except NstError:
            pass
    with pytest.raises(NstError):
        T7.read_t7_bytes(b"\x09\x00\x00\x00")  # unknown tag
    with pytest.raises(NstError):
        T7.read_t7("/nonexistent/dir/a.t7")


@pytest.mark.parametrize("variant", sorted(W.VARIANTS))
def test_matcher_canonical_weights(files, variant):
    data, Pw = files[variant]
    kind, M = T7.match_network(T7.read_t7_bytes(data))
    assert kind == W.VARIANTS[variant]["kind"]
    assert set(M) == set(Pw)
    for k, v in Pw.items():
        assert M[k].dtype == torch.float32 and M[k].shape == v.shape, k
        if k.endswith("running_var") and "std" in variant:
            continue  # derived: the next test
        assert torch.equal(M[k], v), k


def test_running_std_and_running_var_give_the_same_tables(files):
    """running_std = 1 / sqrt(var + eps) is stored in fp32 (relative rounding 2^-24), so var + eps comes back within
    2 * 2^-24 (plus the fp32 rounding of the result): 1e-6 relative with margin."""
    _, a = T7.match_network(T7.read_t7_bytes(files["bn_var"][0]))
    _, b = T7.match_network(T7.read_t7_bytes(files["bn_std_legacy_2d"][0]))
    assert set(a) == set(b)
    for k in a:
        if k.endswith("running_var"):
            eps = float(a[k[:-len("running_var")] + "eps"][0])
            rel = ((a[k].double() - b[k].double()).abs() / (a[k].double() + eps)).max()
            assert rel < 1e-6, (k, float(rel))
        else:
            assert torch.equal(a[k], b[k]), k


def _tree(kind="in", **kw):
    return W.build_tree(kind, W.make_params(kind, 1), **kw)


def _mods(tree):
    return tree.fields["modules"]


def _refused(tree, *words):
    with pytest.raises(NstError) as e:
        T7.match_network(T7.read_t7_bytes(W.dumps(tree)))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_matcher_refusals_name_the_mismatch():
    t = _tree()
    _mods(t)[4].fields["nOutputPlane"] = 48  # down2: 32 -> 48 channels
    _refused(t, "module 5", "nOutputPlane", "48")
    _refused(_tree(blocks=6), "module 16", "nn.SpatialFullConvolution", "nn.Sequential")
    t = _tree()
    for k in ("pad_l", "pad_r", "pad_t", "pad_b"):
        _mods(t)[0].fields[k] = 30
    _refused(t, "module 1", "pad_l", "30")
    t = _tree("in")
    _mods(t)[5] = _mods(_tree("bn"))[5]  # down2's norm from the BatchNorm net
    _refused(t, "module 6", "mixed norm kinds")
    t = _tree()
    _mods(t)[3] = W.Obj("nn.LeakyReLU", {"negval": 0.01})
    _refused(t, "module 4", "nn.ReLU", "nn.LeakyReLU")
    t = _tree()
    _mods(t)[10].fields["modules"][0].fields["modules"][1].fields["size"] = 1  # the first block's ShaveImage
    _refused(t, "module 11", "nn.ShaveImage", "size")
    _refused(W.Obj("nn.ConcatTable", {"modules": []}), "top level", "nn.Sequential")


def test_output_size_formula_matches_the_oracle():
    """4 * (h3 - 20) against the shapes the interpreter produces, H in 41..60 (W: 41..44, every residue mod 4)."""
    root = T7.read_t7_bytes(W.make_file_bytes("bn_var", 0)[0])
    for h in range(41, 61):
        w = 41 + h % 4
        y = R.forward(root, np.zeros((1, 3, h, w), np.float32))
        assert y.shape == (1, 3, T7.output_side(h), T7.output_side(w)), (h, w, y.shape)
        if h % 4 == 0:
            assert T7.output_side(h) == h


def _args(*argv):
    return P.build_parser().parse_args(list(argv) + ["--synthetic", "64x48"])


def test_prepare_selects_torch7_for_a_t7_file(files, tmp_path):
    p = tmp_path / "a.t7"
    p.write_bytes(files["in_legacy_2d_tv"][0])
    args = _args("--model", str(p))
    P.prepare(args)
    assert args.model_type == "torch7" and args.io_preset == "caffe_bgr"
    # slot B: the suffix selects the back end per slot, an explicit type wins
    args = _args("--model", "x.pth", "--model_b", str(p))
    assert P.slot_model_type(args, "b") == "torch7" and P.slot_model_type(args, "c") == "transformer"
    P.prepare(args)
    assert args.model_type == "transformer"
    args = _args("--model", "x.pth", "--model_b", str(p), "--model_b_type", "reconet")
    assert P.slot_model_type(args, "b") == "reconet"


@pytest.mark.parametrize("slot", ["a", "b"])
def test_prepare_exits_2_on_a_bad_t7(files, tmp_path, slot):
    good = tmp_path / "good.t7"
    good.write_bytes(files["bn_var"][0])
    for name, data in (("garbage.t7", b"not a torch file"), ("cut.t7", files["bn_var"][0][:100000]),
                       ("other.t7", W.dumps(W.build_tree("bn", W.make_params("bn", 0), blocks=4))), ("missing.t7", None)):
        bad = tmp_path / name
        if data is not None:
            bad.write_bytes(data)
        args = _args("--model", str(bad)) if slot == "a" else _args("--model", str(good), "--model_b", str(bad))
        with pytest.raises(SystemExit) as e:
            P.prepare(args)
        assert e.value.code == 2, name


def test_prepare_error_message_and_magenta(tmp_path, capfd):
    with pytest.raises(SystemExit) as e:
        P.prepare(_args("--model", str(tmp_path / "nope.t7")))
    assert e.value.code == 2
    out, err = capfd.readouterr()
    assert "[torch7][ERROR] Could not load .t7 network from" in out + err
    for extra in (["--model_type", "magenta"], ["--model_b", "magenta"], ["--model_b", "x.pth", "--model_b_type", "magenta"]):
        with pytest.raises(SystemExit) as e:
            P.prepare(_args("--model", "x.pth", *extra))
        assert e.value.code == 2


def test_torch7_ids_match_header():
    import os
    import re

    from conftest import REPO
    from neuralstyletransferv1_amd import _lib
    src = open(os.path.join(REPO, "include", "nst_hip.h")).read()
    for name in ("NST_ARCH_TORCH7_IN", "NST_ARCH_TORCH7_BN", "NST_PRESET_TORCH7"):
        assert re.search(rf"#define {name} {getattr(_lib, name)}\b", src), name
    assert _lib.NST_PRESET_TORCH7 not in _lib.PRESETS.values()  # not an --io_preset choice
