"""The 16-bit predictive coder on the host: csrc/idf_deep.h's model (idf_deep_prep_host,
idf_deep_decode_host) against tests/deep_ref.py and the C oracle, and the IDFD container.  No GPU.

A file holds one channel count, so the hand-made images -- grey 13 x 11, 3-channel 9 x 20 and grey
8 x 8 at tile 8 x 8 -- make two files: the two grey images and the 3-channel one; both digests are
pinned in tests/golden/idfd_hand.sha256."""
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

import deep_ref as R
from conftest import GOLDEN
from deep_cases import KINDS, hand_units, random_unit


@pytest.fixture(scope="module")
def unit_set():
    rng = np.random.default_rng(16)
    units = [random_unit(rng, KINDS[i % 5], int(rng.integers(1, 17)), int(rng.integers(1, 17)))
             for i in range(300)]
    return units + hand_units()


def test_prep_host_equals_the_reference_field_for_field(unit_set, oracle):
    from idfcodec import deep
    shifts, n_esc = set(), 0
    for u in unit_set:
        want = R.model(u)
        got = deep.host_prep(u)
        assert got["shift"] == want["shift"], u.shape
        assert got["sel"] == want["sel"]
        assert (got["min"], got["max"]) == (want["min"], want["max"])
        assert np.array_equal(got["esc"], want["esc"])
        assert np.array_equal(got["low"], want["low"])
        for k in ("x", "mean", "scale"):
            assert np.array_equal(got[k], want[k]), k
        off = np.array([0, u.size], dtype=np.int64)
        _, words, nw, status = oracle.encode_streams(off, got["x"], got["mean"], got["scale"])
        assert int(status[0]) == 0                      # the window argument of csrc/idf_deep.h
        shifts.add(got["shift"])
        n_esc += len(got["esc"])
    assert shifts == set(range(9))                      # the set covers every shift
    assert n_esc > 0


def test_escape_at_the_first_sample():
    from idfcodec import deep
    u = hand_units()[-1]
    got = deep.host_prep(u)
    assert len(got["esc"]) >= 1 and int(got["esc"][0]) == int(u[0, 0])
    assert R.model(u)["esc_mask"][0, 0]


def test_decode_host_returns_the_samples(unit_set):
    from idfcodec import deep
    for u in unit_set[::3] + hand_units():
        m, state, words = R.encode(u)
        out, final, status = deep.host_decode(*u.shape, m["shift"], m["sel"], state, words,
                                              m["low"], m["esc"])
        assert status == 0 and final == R.L
        assert np.array_equal(out, u)


def test_decode_host_flags_a_damaged_unit():
    from idfcodec import deep
    rng = np.random.default_rng(5)
    u = random_unit(rng, "gauss", 16, 16)
    m, state, words = R.encode(u)
    assert len(words) >= 2
    for w in (words[:-1], np.concatenate([words, words[:1]])):
        got = deep.host_decode(16, 16, m["shift"], m["sel"], state, w, m["low"], m["esc"])
        want = R.decode(m["shift"], m["sel"], state, w, m["low"], m["esc"], 16, 16)
        assert got[2] != 0 or got[1] != R.L
        assert (got[1], got[2]) == (want[1], want[2]) and np.array_equal(got[0], want[0])
    out, _, status = deep.host_decode(16, 16, 9, m["sel"], state, words, m["low"], m["esc"])
    assert status & R.OUT_OF_WINDOW


def test_unit_class_follows_the_rule():
    from idfcodec import deep
    n = 64
    assert deep.unit_class([5], [5], [n], [0], [100], [0])[0] == deep.CLASS_CONSTANT
    # 21 + 4 * 26 = 125 < 128 packs; 21 + 4 * 26 + 2 = 127 packs; 21 + 4 * 26 + 4 = 129 does not
    assert deep.unit_class([1], [2], [n], [0], [26], [0])[0] == deep.CLASS_PACKED
    assert deep.unit_class([1], [2], [n], [0], [26], [1])[0] == deep.CLASS_PACKED
    assert deep.unit_class([1], [2], [n], [0], [26], [2])[0] == deep.CLASS_RAW
    # the low-bit words count: at s = 1 two of them, 21 + 4 * 24 + 4 * 2 + 2 = 127 < 128
    assert deep.unit_class([1], [2], [n], [1], [24], [1])[0] == deep.CLASS_PACKED
    assert deep.unit_class([1], [2], [54], [0], [21], [1])[0] == deep.CLASS_PACKED   # 107 < 108
    assert deep.unit_class([1], [2], [53], [0], [21], [0])[0] == deep.CLASS_PACKED   # 105 < 106
    assert deep.unit_class([1], [2], [52], [0], [21], [0])[0] == deep.CLASS_RAW      # 105 > 104
    assert deep.unit_class([1], [2], [54], [0], [21], [3])[0] == deep.CLASS_RAW      # 111 > 108
    assert int(deep.packed_bytes(54, 0, 21, 1)) == 107    # always odd: no unit ever ties
    for u in hand_units():
        k, m, state, words = R.unit_class(u)
        if m is None:
            assert k == R.CONSTANT
            continue
        got = deep.unit_class([m["min"]], [m["max"]], [u.size], [m["shift"]], [len(words)],
                              [len(m["esc"])])[0]
        assert got == k


# ------------------------------------------------------------------ the container
def bitstream_of(images, th, tw):
    """The DeepTiledBitstream of a list of uint16 [C, H, W] images, its fields from deep_ref."""
    from idfcodec import deep
    units = R.units_of(images, th, tw)
    coded = [R.unit_class(u) for u in units]
    cls = np.array([c[0] for c in coded])
    pk = [c for c in coded if c[0] == R.PACKED]
    cat = lambda parts, dt: np.concatenate([np.asarray(p, dtype=dt) for p in parts]
                                           or [np.zeros(0, dt)])  # noqa: E731
    raw = cat([u.reshape(-1) for u, k in zip(units, cls) if k == R.RAW], "<u2")
    return deep.DeepTiledBitstream(
        [i.shape[1:] for i in images], images[0].shape[0], (th, tw), cls == R.CONSTANT,
        cls == R.PACKED,
        np.array([u.flat[0] for u, k in zip(units, cls) if k == R.CONSTANT], dtype=np.uint16),
        torch.from_numpy(raw.view(np.uint8).copy()),
        np.array([c[1]["shift"] for c in pk], dtype=np.uint8),
        np.array([c[1]["sel"] for c in pk], dtype=np.uint32),
        np.array([c[2] for c in pk], dtype=np.uint64),
        np.array([len(c[3]) for c in pk], dtype=np.int64),
        np.array([len(c[1]["esc"]) for c in pk], dtype=np.int64),
        torch.from_numpy(cat([c[3] for c in pk], np.uint32).view(np.int32).copy()),
        torch.from_numpy(cat([c[1]["low"] for c in pk], np.uint32).view(np.int32).copy()),
        cat([c[1]["esc"] for c in pk], np.uint16))


@pytest.fixture(scope="module")
def hand_files():
    a, b, c = R.hand_images()
    return {"grey": ([a, c], R.write_file([a, c], 8, 8)), "rgb": ([b], R.write_file([b], 8, 8))}


def test_hand_files_match_the_pinned_digests(hand_files):
    with open(os.path.join(GOLDEN, "idfd_hand.sha256")) as f:
        want = {name: digest for digest, name in (line.split() for line in f)}
    assert set(want) == set(hand_files)
    for name, (_, buf) in hand_files.items():
        assert hashlib.sha256(buf).hexdigest() == want[name], name


def test_hand_files_hold_every_class_shift_and_an_escape(hand_files):
    from idfcodec import deep
    classes, shifts, n_esc = set(), set(), 0
    for _, buf in hand_files.values():
        bs = deep.DeepTiledBitstream.from_bytes(buf)
        classes |= set(bs.classes.tolist())
        shifts |= set(bs.shift.tolist())
        n_esc += len(bs.escapes)
    assert classes == {deep.CLASS_CONSTANT, deep.CLASS_PACKED, deep.CLASS_RAW}
    assert {0, 3, 8} <= shifts and n_esc > 0


def test_container_round_trip_and_bound(hand_files):
    from idfcodec import DeepTiledBitstream, deep_section_bound
    for images, buf in hand_files.values():
        bs = bitstream_of(images, 8, 8)
        assert bs.to_bytes() == buf                         # the codec's writer, deep_ref's file
        back = DeepTiledBitstream.from_bytes(buf)
        assert back.to_bytes() == buf
        assert back.sizes == [tuple(i.shape[1:]) for i in images]
        assert np.array_equal(back.classes, bs.classes)
        assert len(buf) <= deep_section_bound(back.sizes, back.C, (8, 8))
        assert 8 * len(buf) > back.bits()
    # nothing but raw units: the bound is met within the pads
    rng = np.random.default_rng(3)
    noise = [rng.integers(0, 65536, (2, 9, 17)).astype(np.uint16)]
    buf = R.write_file(noise, 8, 8)
    bound = deep_section_bound([(9, 17)], 2, (8, 8))
    assert bound - 4 - 2 * 2 <= len(buf) <= bound


def test_from_bytes_rejects_what_does_not_fit(hand_files):
    from idfcodec import DeepTiledBitstream as B
    _, buf = hand_files["grey"]
    for n in range(len(buf)):                               # every truncation
        with pytest.raises(ValueError):
            B.from_bytes(buf[:n])
    with pytest.raises(ValueError, match="trailing"):
        B.from_bytes(buf + b"\0")
    with pytest.raises(ValueError, match="not an IDF"):
        B.from_bytes(b"IDFM" + buf[4:])
    with pytest.raises(ValueError, match="version"):
        B.from_bytes(buf[:4] + struct.pack("<H", 2) + buf[6:])
    with pytest.raises(ValueError, match="flags"):
        B.from_bytes(buf[:6] + struct.pack("<H", 8) + buf[8:])
    # where the parts lie: header 24, sizes 16, U = 5 units: one bitmap byte, K = 1: one more
    bs = B.from_bytes(buf)
    U, K = bs.n_units, int(bs.constant.sum())
    assert (U, K) == (5, 1)
    o_raw = 24 + 16 + 1 + 1 + 2 * K
    (n_raw,) = struct.unpack_from("<Q", buf, o_raw)
    o_sect = o_raw + 8 + n_raw
    (n_sect,) = struct.unpack_from("<Q", buf, o_sect)
    (P,) = struct.unpack_from("<I", buf, o_sect + 8)
    assert P == int(bs.packed.sum()) == 3 and o_sect + 8 + n_sect == len(buf)

    def patched(at, fmt, v):
        return buf[:at] + struct.pack(fmt, v) + buf[at + struct.calcsize(fmt):]
    with pytest.raises(ValueError, match="constant bits past"):
        B.from_bytes(patched(40, "<B", buf[40] | 0x80))
    with pytest.raises(ValueError, match="packed bits past"):
        B.from_bytes(patched(41, "<B", buf[41] | 0x80))
    with pytest.raises(ValueError, match="raw bytes"):
        B.from_bytes(patched(o_raw, "<Q", n_raw + 2))
    with pytest.raises(ValueError):                         # a constant bit more: every count moves
        B.from_bytes(patched(40, "<B", buf[40] | (1 << 3)))
    with pytest.raises(ValueError, match="packed units"):
        B.from_bytes(patched(o_sect + 8, "<I", P + 1))
    with pytest.raises(ValueError, match="shift of 9"):
        B.from_bytes(patched(o_sect + 12, "<B", 9))
    with pytest.raises(ValueError, match="pad"):
        B.from_bytes(patched(o_sect + 12 + P, "<B", 1))
    o_nw = o_sect + 12 + 4 + 12 * P
    with pytest.raises(ValueError, match="counts name"):    # a word count that disagrees
        B.from_bytes(patched(o_nw, "<I", int(bs.nwords[0]) + 1))
    with pytest.raises(ValueError, match="counts name"):    # an escape count that disagrees
        B.from_bytes(patched(o_nw + 4 * P, "<I", int(bs.nesc[0]) + 2))
    with pytest.raises(ValueError, match="more escapes"):
        B.from_bytes(patched(o_nw + 4 * P, "<I", 1000))
    with pytest.raises(ValueError, match="counts name"):    # a shift that moves the low-bit run
        B.from_bytes(patched(o_sect + 12, "<B", (int(bs.shift[0]) + 4) % 9))
    with pytest.raises(ValueError, match="packed section"):
        B.from_bytes(patched(o_sect, "<Q", n_sect + 4) + b"\0" * 4)


def test_codec_refuses_bad_arguments_without_a_device():
    from idfcodec import DeepTiledCodec, deep
    with pytest.raises(ValueError):
        DeepTiledCodec(0)
    with pytest.raises(ValueError):
        DeepTiledCodec(1, tile=(0, 8))
    with pytest.raises(ValueError, match="width"):
        DeepTiledCodec(1, tile=(8, deep.tw_max() + 1))
    codec = DeepTiledCodec(1, tile=(8, 8))
    assert (codec.C, codec.tile_hw) == (1, (8, 8))
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="not uint16"):
        deep.source_views16([torch.zeros(1, 4, 4, dtype=torch.uint8)], 1, dev, "chw")
    with pytest.raises(ValueError, match="channels"):
        deep.source_views16([torch.zeros(2, 4, 4, dtype=torch.uint16)], 1, dev, "chw")
    with pytest.raises(ValueError, match="contiguous"):
        deep.source_views16([torch.zeros(1, 4, 8, dtype=torch.uint16)[:, :, ::2]], 1, dev)
    v = deep.source_views16([torch.zeros(4, 6, 3, dtype=torch.uint16)], 3, dev, "hwc")[0]
    rows = deep.unit_rows([(0, 4, 6, 0, 0)], [v], 3)
    assert rows.shape == (3, 8) and rows[1, 0] - rows[0, 0] == 2
    assert tuple(rows[0, 5:]) == (0, 2 * 18, 2 * 3)


def test_host_calls_check_their_arguments():
    import ctypes
    from idfcodec import _lib
    L = _lib.lib()
    z = (ctypes.c_uint16 * 4)()
    assert L.idf_deep_prep_host(None, 2, 2, *([z] * 9)) == 1
    assert L.idf_deep_prep_host(z, 0, 2, *([z] * 9)) == 1
    assert L.idf_deep_decode_host(2, 2, 0, 0, 1 << 32, None, 0, None, None, 0, None, z, z) == 1
    assert L.idf_deep_decode_host(2, 2, 0, 0, 1 << 32, None, -1, None, None, 0, z, z, z) == 1
    # the device calls, as far as they go without a device: counts, tile sizes, NULLs, odd rows
    row = (ctypes.c_int64 * 8)(2, 4, 4, 0, 0, 0, 8, 2)
    p = ctypes.cast(z, ctypes.c_void_p)
    assert L.idf_deep_prep_u16(None, 0, 8, 8, *([None] * 14)) == 0
    assert L.idf_deep_prep_u16(None, -1, 8, 8, p, row, *([p] * 12)) == 1
    assert L.idf_deep_prep_u16(None, 1, 0, 8, p, row, *([p] * 12)) == 1
    assert L.idf_deep_prep_u16(None, 1, 8, 8, p, row, *([p] * 11), None) == 1
    for i, v in ((0, 3), (6, 7), (7, 1), (6, -2)):
        bad = (ctypes.c_int64 * 8)(*row)
        bad[i] = v
        assert L.idf_deep_prep_u16(None, 1, 8, 8, p, bad, *([p] * 12)) == 1
        assert L.idf_tile_gather_raw_strided_u16(None, 1, 8, 8, p, bad, p, p) == 1
        assert L.idf_tile_scatter_raw_strided_u16(None, 1, 8, 8, p, p, p, p, bad) == 1
    assert L.idf_tile_gather_raw_strided_u16(None, 0, 8, 8, None, None, None, None) == 0
    assert L.idf_tile_gather_raw_strided_u16(None, 1, 8, 8, p, row, None, p) == 1
    assert L.idf_tile_scatter_raw_strided_u16(None, 1, 8, 0, p, p, p, p, row) == 1
    assert L.idf_deep_decode_u16(None, 0, 8, 8, *([None] * 18)) == 0
    assert L.idf_deep_decode_u16(None, -1, 8, 8, *([p] * 18)) == 1
    assert L.idf_deep_decode_u16(None, 1, 8, 8, *([p] * 17), None) == 1
    assert L.idf_deep_decode_u16(None, 1, 8, L.idf_deep_tw_max() + 1, *([p] * 18)) \
        == _lib.IDF_ERR_UNSUPPORTED


# ------------------------------------------------------------------ the tool's 16-bit files
def test_tool_reads_and_writes_16_bit_files(tmp_path, hand_files):
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(8)
    grey, rgb = (rng.integers(0, 65536, s).astype(np.uint16) for s in ((5, 7, 1), (4, 6, 3)))
    grey[0, 0, 0] = 0x0102                                  # the byte order shows
    for i, a in enumerate((grey, rgb)):
        path = tool.write_image16(str(tmp_path), i, a)
        assert path.endswith(".pgm" if a.shape[2] == 1 else ".ppm")
        assert tool.is_deep_source(path)
        assert np.array_equal(tool.read_image16(path), a)
    with open(tmp_path / "image_0000.pgm", "rb") as f:
        data = f.read()
    assert data.startswith(b"P5\n7 5\n65535\n") and data[13:15] == b"\x01\x02"  # big-endian
    with open(tmp_path / "m.pgm", "wb") as f:               # a 12-bit maxval, a comment
        f.write(b"P5\n# twelve bits\n2 1\n4095\n" + bytes([0x0f, 0xff, 0x00, 0x01]))
    assert tool.is_deep_source(str(tmp_path / "m.pgm"))
    assert tool.read_image16(str(tmp_path / "m.pgm")).reshape(-1).tolist() == [4095, 1]
    with open(tmp_path / "b.pgm", "wb") as f:
        f.write(b"P5\n2 1\n255\n\x01\x02")
    assert not tool.is_deep_source(str(tmp_path / "b.pgm"))
    np.save(tmp_path / "p.npy", grey[:, :, 0])
    np.save(tmp_path / "q.npy", np.zeros((3, 3), np.uint8))
    np.save(tmp_path / "chw.npy", np.ascontiguousarray(rgb.transpose(2, 0, 1)))
    assert tool.is_deep_source(str(tmp_path / "p.npy"))
    assert not tool.is_deep_source(str(tmp_path / "q.npy"))
    assert np.array_equal(tool.read_image16(str(tmp_path / "p.npy")), grey)
    assert np.array_equal(tool.read_image16(str(tmp_path / "chw.npy")), rgb)
    with pytest.raises(SystemExit):
        tool._deep_or_not([str(tmp_path / "p.npy"), str(tmp_path / "q.npy")])
    bs, may_be_raw, sealed = tool.read_file(hand_files["grey"][1], None)
    assert type(bs).__name__ == "DeepTiledBitstream" and may_be_raw and not sealed
