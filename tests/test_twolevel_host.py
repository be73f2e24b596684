"""TwoLevelFlows on the host (no device): the seeded mirror against the reference's recorded
state_dict, the integer restatement of the pad / pool / residual / patch split against the
reference's tensors (ties included), constructor errors, the IDF2 container and the grouped
stream-offset arithmetic."""
import os
import struct

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN


@pytest.fixture(scope="module")
def tiny(golden):
    return golden("twolevel_tiny.npz")


def _cfg(d):
    return yaml.safe_load(bytes(d["cfg_yaml"]).decode())


# ------------------------------------------------------------------ the mirror
def test_seeded_twolevel_mirror_equals_reference(tiny):
    from idfcodec import synthetic
    cfg = _cfg(tiny)
    before = yaml.safe_dump(cfg)
    model = synthetic.build_model(cfg)
    assert yaml.safe_dump(cfg) == before  # the sub-config dicts are copied, not popped
    sd = model.state_dict()
    ref = {k[3:]: tiny[k] for k in tiny.files if k.startswith("sd/")}
    assert list(sd) == list(ref)
    assert any(k.startswith("fine.blocks.") for k in sd) and any(
        k.startswith("rough.blocks.") for k in sd)
    for k in ref:
        assert np.array_equal(sd[k].numpy(), ref[k]), k
    assert [tuple(s) for s in model.latents_shape] == [tuple(s) for s in tiny["latents_shape"]]
    assert tuple(model.ratio) == tuple(tiny["ratio"])
    assert (model.H, model.W) == tuple(tiny["padded_hw"]) == (16, 16)
    assert (model.C, list(model.pad), model.batchsize) == (3, [1, 3], 3)
    assert type(model.fine).__name__ == type(model.rough).__name__ == "IDFlows"
    assert type(model.patching).__name__ == "Patching" and model.round.nbits == 8


def test_twolevel_config_restates_reference_yaml():
    from idfcodec import configs
    assert len(configs.CONFIGS) == 4 and list(configs.TWOLEVEL) == ["config_twolevel"]
    path = os.path.join(GOLDEN, "configs", "config_twolevel.yaml")
    assert configs.load_yaml(path) == configs.get_twolevel("config_twolevel")
    cfg = configs.get_twolevel()
    cfg["fine_flows"]["nflows"] = 1
    assert configs.get_twolevel()["fine_flows"]["nflows"] == 12  # a copy each time


def test_constructor_errors(tiny):
    import flows
    cfg = _cfg(tiny)
    cfg.pop("name")
    bad = dict(cfg, H=17, W=13)  # 18x16 over an 8x8 rough image: ratio 2.25
    with pytest.raises(ValueError, match="integer multiple"):
        flows.TwoLevelFlows(**bad)
    bad = dict(cfg, pad=[1, 4])  # 16x17
    with pytest.raises(ValueError, match="integer multiple"):
        flows.TwoLevelFlows(**bad)
    model = flows.TwoLevelFlows(**cfg)
    with pytest.raises(NotImplementedError, match="train"):
        model.forward(torch.zeros(1, 3, 15, 13), None)           # train defaults to True
    with pytest.raises(NotImplementedError, match="train"):
        model.forward(torch.zeros(1, 3, 15, 13), None, train=True)


# ------------------------------------------------------------------ the integer split
@pytest.mark.parametrize("which", ["2x2", "4x4"])
def test_integer_split_restatement_equals_reference(tiny, which):
    from idfcodec.twolevel import merge_host, split_host
    if which == "2x2":
        u8, pad, rx, px = tiny["image_u8"], (1, 3), tiny["rx"], tiny["px"]
        assert int(tiny["n_ties"]) >= 1
    else:
        u8, pad, rx, px = (tiny["set2/image_u8"], tuple(tiny["set2/pad"]), tiny["set2/rx"],
                           tiny["set2/px"])
        assert int(tiny["set2/n_ties"]) >= 1
    got_rx, got_px, got_pad = split_host(u8, pad, (8, 8), (8, 8))
    assert got_rx.dtype == got_px.dtype == np.float32
    assert np.array_equal(got_rx, rx)
    assert np.array_equal(got_px, px)
    if which == "2x2":
        assert np.array_equal(got_pad, tiny["x_pad"])
        # replicate(rx) + unpatch(px), cropped, is the dequantised source
        assert np.array_equal(merge_host(rx, px, pad, (16, 16)), tiny["input"])


def test_round_half_even_div():
    from idfcodec.twolevel import round_half_even_div
    s = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, -1, -2, -3, -5, -6, -7])
    assert round_half_even_div(s, 4).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 0, 0, -1, -1,
                                                  -2, -2]
    # a window that is no power of two: 18 pixels, ties at odd multiples of 9
    assert round_half_even_div(np.array([8, 9, 10, 27, 45]), 18).tolist() == [0, 0, 1, 2, 2]
    assert np.array_equal(round_half_even_div(s, 4), np.round(s / 4).astype(np.int64))


# ------------------------------------------------------------------ containers
def _stream(n_images, n_streams, group=1, seed=0, shapes=((12, 4, 4),)):
    from idfcodec.codec import Bitstream
    g = torch.Generator().manual_seed(seed)
    nw = torch.randint(0, 9, (n_streams,), generator=g).to(torch.int64)
    st = torch.randint(-(2 ** 62), 2 ** 62, (n_streams,), generator=g, dtype=torch.int64)
    w = torch.randint(-(2 ** 31), 2 ** 31 - 1, (int(nw.sum()),), generator=g, dtype=torch.int32)
    return Bitstream(n_images, [tuple(s) for s in shapes], st, nw, w,
                     meta={"n_subpixels": 7 * n_images, "conv": "dx3"}, group=group)


def _two(group=4):
    from idfcodec.twolevel import TwoLevelBitstream
    rough = _stream(2, 2, shapes=((3, 8, 8),), seed=1)
    fine = _stream(8, 8 // group, group=group, seed=2)
    return TwoLevelBitstream(rough, fine, 2, (3, 15, 13), (1, 3), (8, 8), (8, 8))


@pytest.mark.parametrize("group", [1, 2, 4])
def test_twolevel_container_roundtrip(group):
    from idfcodec.twolevel import TwoLevelBitstream
    t = _two(group)
    raw = t.to_bytes()
    assert raw[:4] == b"IDF2" and struct.unpack_from("<HH", raw, 4) == (1, 0)
    assert struct.unpack_from("<11I", raw, 8) == (2, 3, 15, 13, 1, 3, 8, 8, 8, 8, group)
    lr, lf = struct.unpack_from("<QQ", raw, 52)
    assert len(raw) == 68 + lr + lf
    assert raw[68:68 + lr] == t.rough.to_bytes()
    b = TwoLevelBitstream.from_bytes(raw)
    assert b.group == b.fine.group == group and b.rough.group == 1
    assert (b.n_images, b.image_shape, b.pad, b.rough_hw, b.fine_hw) == (
        2, (3, 15, 13), (1, 3), (8, 8), (8, 8))
    for a, c in ((b.rough, t.rough), (b.fine, t.fine)):
        assert torch.equal(a.states, c.states) and torch.equal(a.nwords, c.nwords)
        assert torch.equal(a.words, c.words) and a.meta["conv"] == "dx3"
        assert a.n_images == c.n_images and a.level_shapes == c.level_shapes
    assert b.bits() == t.bits() == t.rough.bits() + t.fine.bits()
    assert t.fine.bits() == 64 * (8 // group) + 32 * t.fine.total_words()
    assert b.bpd() == t.bits() / (2 * 3 * 15 * 13)  # the unpadded denominator
    assert b.to_bytes() == raw


def test_twolevel_container_rejects_bad_input():
    from idfcodec.twolevel import TwoLevelBitstream
    raw = _two(4).to_bytes()
    TwoLevelBitstream.from_bytes(raw)
    with pytest.raises(ValueError, match="not an IDF two-level"):
        TwoLevelBitstream.from_bytes(b"IDFB" + raw[4:])
    with pytest.raises(ValueError, match="version"):
        TwoLevelBitstream.from_bytes(raw[:4] + struct.pack("<H", 2) + raw[6:])
    with pytest.raises(ValueError, match="flags"):
        TwoLevelBitstream.from_bytes(raw[:6] + struct.pack("<H", 1) + raw[8:])
    for cut in (3, 40, 67, 68, 90, len(raw) - 1):
        with pytest.raises(ValueError):
            TwoLevelBitstream.from_bytes(raw[:cut])
    with pytest.raises(ValueError):
        TwoLevelBitstream.from_bytes(raw + b"\0")
    # a group the stream count does not fit
    with pytest.raises(ValueError):
        TwoLevelBitstream.from_bytes(raw[:48] + struct.pack("<I", 8) + raw[52:])
    with pytest.raises(ValueError):
        TwoLevelBitstream.from_bytes(raw[:48] + struct.pack("<I", 0) + raw[52:])


def test_grouped_bitstream_is_not_serialised_as_ungrouped():
    from idfcodec.codec import VERSION, Bitstream
    grouped = _stream(8, 2, group=4)
    with pytest.raises(ValueError, match="group"):
        grouped.to_bytes()
    plain = _stream(8, 8)
    raw = plain.to_bytes()
    assert VERSION == 2 and struct.unpack_from("<4sH", raw, 0) == (b"IDFB", 2)
    # the ungrouped layout, byte for byte: header, shapes, sub-pixel count, states, counts, words
    assert raw == (struct.pack("<4sHHIII", b"IDFB", 2, 7, 8, 1, 8) + struct.pack("<III", 12, 4, 4)
                   + struct.pack("<Q", 56) + plain.states.numpy().astype("<i8").tobytes()
                   + plain.nwords.numpy().astype("<u4").tobytes()
                   + plain.words.numpy().astype("<i4").tobytes())
    back = Bitstream.from_bytes(raw)
    assert back.group == 1 and back.n_streams == 8
    # inside the container the same bytes carry the group
    inner = grouped.to_bytes(grouped=True)
    assert Bitstream.from_bytes(inner, group=4).group == 4
    with pytest.raises(ValueError):
        Bitstream.from_bytes(inner, group=3)


# ------------------------------------------------------------------ grouped offsets
def test_grouped_stream_offsets():
    from idfcodec.codec import grouped_stream_offsets
    n0, n1, B = 96, 192, 12
    assert grouped_stream_offsets([n0, n1], B, 1) == (
        [n0 * b for b in range(B)] + [B * n0 + n1 * b for b in range(B + 1)])
    assert grouped_stream_offsets([n0, n1], B, 4) == [
        0, 4 * n0, 8 * n0, 12 * n0, 12 * n0 + 4 * n1, 12 * n0 + 8 * n1, 12 * n0 + 12 * n1]
    assert grouped_stream_offsets([n0, n1], B, 12) == [0, 12 * n0, 12 * (n0 + n1)]
    for G in (1, 4, 12):
        off = grouped_stream_offsets([n0, n1], B, G)
        assert len(off) == 2 * B // G + 1 and off[-1] == B * (n0 + n1)
        # every grouped boundary is a boundary of the ungrouped table
        assert set(off) <= set(grouped_stream_offsets([n0, n1], B, 1))
    for G in (5, 8, 24, 0, -1):
        with pytest.raises(ValueError, match="group"):
            grouped_stream_offsets([n0, n1], B, G)


def test_lanes_hold_whole_groups():
    """Decode lanes split a batch only into sub-batches of whole stream groups."""
    from idfcodec.codec import ImageCodec
    c = ImageCodec(None, lanes=2)
    assert c._n_lanes(48) == 2 and c._n_lanes(48, 4) == 2
    assert c._n_lanes(48, 16) == 1      # lanes of 24 would split a group of 16
    assert c._n_lanes(48, 48) == 1
    assert c._lane_sizes(48, 2, 4) == [24, 24]


def test_check_bitstream_counts_grouped_streams():
    from types import SimpleNamespace
    from idfcodec.codec import ImageCodec
    c = ImageCodec.__new__(ImageCodec)
    c.engine = SimpleNamespace(levels=[SimpleNamespace(z=12, h=4, w=4)], conv_family="dx3",
                               can_run=lambda conv: True)
    c.check_bitstream(_stream(8, 2, group=4))
    c.check_bitstream(_stream(8, 8))
    with pytest.raises(ValueError, match="streams"):
        c.check_bitstream(_stream(8, 8, group=4))
    with pytest.raises(ValueError, match="group"):
        c.check_bitstream(_stream(8, 2, group=3))
