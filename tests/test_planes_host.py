"""Plane sets on the host (no device): the IDFM container and every refusal of its reader, its
layout frozen by a digest, the class rule of the extra planes' units, the plane section's size
bound, derived and not measured, the arguments of model.tiled_planes, and the argument rules of
the two byte-run entry points."""
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from idfcodec import planes  # the module under test: every test here needs it
from test_predict_host import MIXED, PACKED, _pred
from test_safe_host import RECTS, SIZES, _safe

L = 1 << 32
NB = [h * w for h, w in RECTS]        # a unit's bytes per entry: 1, 256, 16, 80, 80, 40
N_HDR = 28 + 8 * len(SIZES)           # the header and the size table


def _hand(Cb=3, Ce=1, ways=1, base="predict"):
    """A PlaneSetBitstream over SIZES (6 entries of 16x16 tiles): unit u is constant, packed or
    raw as u % 3 is 0, 1 or 2; constant number k holds 255 - 3 k, raw byte j of unit u is
    (5 * u + j) % 253, packed unit number p holds p + 1 words 777 * p + j, sel 0x89ABCDE0 + p
    and states L + 100 * p + w."""
    U = 6 * Ce
    cls = np.arange(U) % 3
    nb = np.repeat(NB, Ce)
    raw = [(np.arange(nb[u], dtype=np.int64) + 5 * u) % 253 for u in range(U) if cls[u] == 2]
    raw = np.concatenate(raw).astype(np.uint8) if raw else np.zeros(0, np.uint8)
    K, P = int((cls == 0).sum()), int((cls == 1).sum())
    states = (np.uint64(L) + np.uint64(100) * np.arange(P, dtype=np.uint64)[:, None]
              + np.arange(ways, dtype=np.uint64)[None, :])
    words = np.array([777 * p + j for p in range(P) for j in range(p + 1)], dtype=np.int32)
    b = None
    if Cb:
        b = _pred(MIXED, PACKED) if base == "predict" else _safe(MIXED)
    return planes.PlaneSetBitstream(
        b, list(SIZES), Cb + Ce, Cb, (16, 16), cls == 0, cls == 1,
        (255 - 3 * np.arange(K)).astype(np.uint8), torch.from_numpy(raw),
        np.arange(P, dtype=np.uint32) + np.uint32(0x89ABCDE0),
        states if ways > 1 else states[:, 0], np.arange(P, dtype=np.int64) + 1,
        torch.from_numpy(words), ways)


# ------------------------------------------------------------------ the container
@pytest.mark.parametrize("ways", [1, 8])
@pytest.mark.parametrize("Cb,Ce", [(0, 1), (0, 2), (3, 1), (3, 2), (3, 0)])
def test_container_round_trip_and_layout(Cb, Ce, ways):
    bs = _hand(Cb, Ce, ways)
    buf = bs.to_bytes()
    base = bs.base.to_bytes() if Cb else b""
    want = (struct.pack("<4sHHIIIII", b"IDFM", 1, ways if ways > 1 else 0, 3, Cb + Ce, Cb, 16, 16)
            + b"".join(struct.pack("<II", *s) for s in SIZES) + struct.pack("<Q", len(base)))
    assert buf[:len(want)] == want and len(want) == N_HDR + 8
    o = len(want)
    assert buf[o:o + len(base)] == base                 # the base file, untouched
    o += len(base)
    U = 6 * Ce
    cls = np.arange(U) % 3
    K, P = int((cls == 0).sum()), int((cls == 1).sum())
    cmap = np.packbits(cls == 0, bitorder="little").tobytes()
    pmap = np.packbits((cls == 1)[cls != 0], bitorder="little").tobytes()
    assert buf[o:o + len(cmap) + len(pmap)] == cmap + pmap
    assert len(cmap) == -(-U // 8) and len(pmap) == -(-(U - K) // 8)
    o += len(cmap) + len(pmap)
    assert buf[o:o + K] == bytes(255 - 3 * k for k in range(K))
    o += K
    (n_raw,) = struct.unpack_from("<Q", buf, o)
    assert n_raw == int(np.repeat(NB, Ce)[cls == 2].sum()) == bs.raw.numel()
    assert buf[o + 8:o + 8 + n_raw] == bs.raw.numpy().tobytes()
    o += 8 + n_raw
    n_sect, got_p = struct.unpack_from("<QI", buf, o)
    nw = np.arange(P) + 1
    assert got_p == P and n_sect == 4 + (8 + 8 * ways) * P + 4 * int(nw.sum())
    assert len(buf) == o + 8 + n_sect
    st = np.frombuffer(buf, "<u8", P * ways, o + 12 + 4 * P).reshape(P, ways)
    assert np.array_equal(st, np.asarray(bs.states).reshape(P, ways))   # unit-major, way-minor
    assert len(bs.plane_section()) == planes.plane_section_bytes(U, K, n_raw, nw, ways)
    assert len(buf) == N_HDR + 8 + len(base) + len(bs.plane_section())

    got = planes.PlaneSetBitstream.from_bytes(buf)
    assert got.to_bytes() == buf
    assert (got.Cs, got.Cb, got.Ce, got.tile_hw, got.sizes) == (Cb + Ce, Cb, Ce, (16, 16), SIZES)
    assert got.predict_ways == ways and got.n_images == 3 and got.n_units == U
    assert np.array_equal(got.classes, np.where(cls == 0, planes.CLASS_CONSTANT, np.where(
        cls == 1, planes.CLASS_PACKED, planes.CLASS_RAW)))
    assert np.array_equal(got.values, bs.values) and torch.equal(got.raw, bs.raw)
    assert np.array_equal(got.sel, bs.sel) and np.array_equal(got.states, bs.states)
    assert np.array_equal(got.nwords, bs.nwords) and torch.equal(got.words, bs.words)
    assert (got.base is None) == (Cb == 0)
    assert got.layout.C == Cb + Ce
    assert got.n_subpixels() == (Cb + Ce) * sum(H * W for H, W in SIZES)
    plane_bits = 8 * K + 8 * n_raw + 8 * (8 + 8 * ways) * P + 32 * int(nw.sum())
    assert got.bits() == (bs.base.bits() if Cb else 0) + plane_bits
    assert got.bpd() == got.bits() / got.n_subpixels()


def test_the_base_is_read_by_its_magic():
    from idfcodec.predict import PredictiveTiledBitstream
    from idfcodec.safe import SafeTiledBitstream
    assert isinstance(planes.PlaneSetBitstream.from_bytes(_hand().to_bytes()).base,
                      PredictiveTiledBitstream)
    buf = _hand(base="safe").to_bytes()
    got = planes.PlaneSetBitstream.from_bytes(buf)
    assert isinstance(got.base, SafeTiledBitstream) and got.to_bytes() == buf


def test_layout_is_frozen():
    with open(os.path.join(GOLDEN, "idfm_hand.sha256")) as f:
        want = dict(line.split()[::-1] for line in f.read().splitlines() if line.strip())
    assert hashlib.sha256(_hand(3, 1, 1).to_bytes()).hexdigest() == want["rgba_one_way"]
    assert hashlib.sha256(_hand(0, 2, 8).to_bytes()).hexdigest() == want["grey_alpha_8_ways"]


def _patch(buf, o, fmt, *v):
    return buf[:o] + struct.pack(fmt, *v) + buf[o + struct.calcsize(fmt):]


def test_reader_refuses_a_bad_header():
    R = planes.PlaneSetBitstream.from_bytes
    buf = _hand().to_bytes()
    with pytest.raises(ValueError, match="not an IDF plane set"):
        R(b"IDFP" + buf[4:])
    with pytest.raises(ValueError, match="version 2"):
        R(_patch(buf, 4, "<H", 2))
    for flags in (1, 3, 4, 128, 0x8000):
        with pytest.raises(ValueError, match="flags"):
            R(_patch(buf, 6, "<H", flags))
    for o in (8, 12, 20, 24):           # n_images, Cs, tile_h, tile_w
        with pytest.raises(ValueError, match="zero size"):
            R(_patch(buf, o, "<I", 0))
    with pytest.raises(ValueError, match="zero size"):
        R(_patch(buf, 28 + 8, "<I", 0))  # H of image 1
    with pytest.raises(ValueError, match="4 channels names 5 base planes"):
        R(_patch(buf, 16, "<I", 5))
    for n in (0, 10, 27):
        with pytest.raises(ValueError, match=r"truncated .*\(header\)"):
            R(buf[:n])
    with pytest.raises(ValueError, match=r"truncated .*\(image sizes\)"):
        R(buf[:N_HDR + 7])


def test_reader_refuses_a_bad_base():
    R = planes.PlaneSetBitstream.from_bytes
    bs = _hand()
    buf = bs.to_bytes()
    n_base = len(bs.base.to_bytes())
    with pytest.raises(ValueError, match=r"truncated .*\(base file\)"):
        R(buf[:N_HDR + 8 + n_base - 1])
    # Cb and the base's presence go together
    with pytest.raises(ValueError, match="0 base planes holds a base file"):
        R(_patch(buf, 16, "<I", 0))
    grey = _hand(0, 1).to_bytes()
    with pytest.raises(ValueError, match="1 base planes holds a base file of 0 bytes"):
        R(_patch(grey, 16, "<I", 1))
    # a base of another C, of another tile size, over other sizes
    with pytest.raises(ValueError, match="disagrees with the header"):
        R(_patch(_patch(buf, 12, "<I", 3), 16, "<I", 2))
    o_b = N_HDR + 8
    with pytest.raises(ValueError, match="disagrees with the header"):
        R(_patch(buf, 20, "<I", 32))
    with pytest.raises(ValueError, match="disagrees with the header"):
        R(_patch(buf, o_b + 24 + 8, "<I", 18))      # the base's own H of image 1
    with pytest.raises(ValueError, match="unknown magic"):
        R(buf[:o_b] + b"IDFC" + buf[o_b + 4:])
    # the writer refuses the same
    bad = _hand()
    bad.base.sizes = [(1, 1), (18, 16), (5, 40)]
    with pytest.raises(ValueError, match="disagrees"):
        bad.to_bytes()
    bad = _hand()
    bad.base = None
    with pytest.raises(ValueError, match="holds no base file"):
        bad.to_bytes()


def test_reader_refuses_a_bad_plane_section():
    R = planes.PlaneSetBitstream.from_bytes
    bs = _hand(0, 2, 1)                 # 12 units: 4 constant, 4 packed, 4 raw
    buf = bs.to_bytes()
    o_c = N_HDR + 8
    o_p, o_v = o_c + 2, o_c + 3
    o_raw = o_v + 4
    n_raw = bs.raw.numel()
    o_sect = o_raw + 8 + n_raw
    assert struct.unpack_from("<Q", buf, o_raw)[0] == n_raw
    assert struct.unpack_from("<QI", buf, o_sect) == (4 + 16 * 4 + 4 * 10, 4)
    for cut, what in ((o_c + 1, "constant bitmap"), (o_p, "packed bitmap"), (o_v + 3, "constants"),
                      (o_raw + 7, "constants"), (o_raw + 8 + n_raw - 1, "raw bytes"),
                      (o_sect + 7, "raw bytes"), (o_sect + 8 + 3, "packed section"),
                      (len(buf) - 1, "packed section")):
        with pytest.raises(ValueError, match=rf"truncated .*\({what}\)"):
            R(buf[:cut])
    with pytest.raises(ValueError, match="1 trailing bytes"):
        R(buf + b"\0")
    with pytest.raises(ValueError, match="constant bits past"):
        R(_patch(buf, o_c + 1, "<B", buf[o_c + 1] | 0x10))     # bit 12 of 12 units
    # all eight coded units packed leaves no raw unit: the raw length no longer fits
    with pytest.raises(ValueError, match=f"names {n_raw} raw bytes, its raw units hold 0"):
        R(_patch(buf, o_p, "<B", 0xFF))
    with pytest.raises(ValueError, match="raw bytes, its raw units hold"):
        R(_patch(buf, o_raw, "<Q", n_raw + 1))
    # one constant more: the counts behind it no longer fit
    with pytest.raises(ValueError, match="raw units hold|packed units|truncated|bits past"):
        R(_patch(buf, o_c, "<B", buf[o_c] | 0x02))
    with pytest.raises(ValueError, match="names 5 packed units, its bitmap 4"):
        R(_patch(buf, o_sect + 8, "<I", 5))
    with pytest.raises(ValueError, match="too short for its count"):
        R(_patch(buf[:o_sect + 8 + 3], o_sect, "<Q", 3))
    with pytest.raises(ValueError, match="too short for the tables"):
        R(_patch(buf[:o_sect + 8 + 40], o_sect, "<Q", 40))
    o_nw = o_sect + 8 + 4 + 4 * 4 + 8 * 4
    with pytest.raises(ValueError, match="word counts name 11 words"):
        R(_patch(buf, o_nw, "<I", 2))
    # the flags say 8 ways, the section holds one state a unit
    with pytest.raises(ValueError, match="packed section"):
        R(_patch(buf, 6, "<H", 8))


def test_packed_bits_past_the_coded_units_are_refused():
    R = planes.PlaneSetBitstream.from_bytes
    buf = _hand(0, 1, 1).to_bytes()     # 6 units, 2 constant: 4 coded units, 4 bits
    o_p = N_HDR + 8 + 1
    with pytest.raises(ValueError, match="packed bits past"):
        R(_patch(buf, o_p, "<B", buf[o_p] | 0x10))


def test_writer_refuses_parts_that_do_not_fit():
    for field, value, msg in (("values", np.zeros(1, np.uint8), "constants"),
                              ("raw", torch.zeros(3, dtype=torch.uint8), "raw bytes"),
                              ("nwords", np.array([1, 1, 1]), "tables"),
                              ("words", torch.zeros(2, dtype=torch.int32), "words"),
                              ("predict_ways", 4, "predict_ways"),
                              ("constant", np.ones(5, bool), "flags")):
        bad = _hand()
        setattr(bad, field, value)
        with pytest.raises(ValueError, match=msg):
            bad.to_bytes()
    bad = _hand()
    bad.packed = np.ones(6, bool)
    with pytest.raises(ValueError, match="packs a unit it holds as a constant"):
        bad.to_bytes()
    bad = _hand(ways=8)
    bad.states = bad.states[:, :7]
    with pytest.raises(ValueError, match="states"):
        bad.to_bytes()


# ------------------------------------------------------------------ the class rule and the bound
def test_split_channels():
    assert planes.split_channels(1, 3) == (0, 1) and planes.split_channels(2, 3) == (0, 2)
    assert planes.split_channels(3, 3) == (3, 0) and planes.split_channels(4, 3) == (3, 1)
    assert planes.split_channels(5, 3) == (3, 2) and planes.split_channels(1, 1) == (1, 0)
    for bad in (0, -1, 1.5, "4", True, None):
        with pytest.raises(ValueError, match="channels"):
            planes.split_channels(bad, 3)


@pytest.mark.parametrize("ways", [1, 8, 64])
def test_class_rule_constant_then_packed_then_raw(ways):
    K, P, R = planes.CLASS_CONSTANT, planes.CLASS_PACKED, planes.CLASS_RAW
    fixed = 8 + 8 * ways
    nb = fixed + 4 * 10 + 1
    # constant beats packed, whatever the stream; then packed iff status 0 and strictly smaller
    got = planes.unit_class([7, 7, 0, 0, 0, 0], [7, 7, 9, 9, 9, 9], [0, 16, 0, 0, 0, 16],
                            [0, 99, 10, 11, 10, 0], [nb, nb, nb, nb, nb - 1, nb], ways)
    assert got.tolist() == [K, K, P, R, R, R]       # 4: a tie goes to raw; 5: a failed status
    # min == max is the whole test of the constant class: one byte apart is not constant
    assert planes.unit_class([0], [1], [0], [0], [fixed + 1], ways).tolist() == [P]
    assert planes.unit_class([0], [1], [0], [0], [fixed], ways).tolist() == [R]
    assert planes.unit_class([255], [255], [0], [0], [1], ways).tolist() == [K]
    # a unit of one byte is always constant: the packed and raw classes start at two bytes
    assert planes.unit_bytes([(1, 1), (2, 3)], 2).tolist() == [1, 1, 6, 6]


def test_plane_section_stays_within_its_bound():
    """Derived: a constant unit's byte, a packed unit's fields and words (the class rule) and a
    raw unit's bytes are each at most the unit's bytes; the rest is the bitmaps and 20 bytes."""
    from idfcodec.tiled import TileLayout
    rng = np.random.default_rng(7)
    for trial in range(200):
        ways = int(rng.choice([1, 8, 16, 32, 64]))
        Ce = int(rng.integers(1, 4))
        th, tw = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sizes = [(int(rng.integers(1, 150)), int(rng.integers(1, 150)))
                 for _ in range(int(rng.integers(1, 4)))]
        nb = planes.unit_bytes(TileLayout(sizes, Ce, (th, tw)).rects, Ce)
        U = len(nb)
        const = rng.random(U) < 0.3
        # word counts from none to past what the class rule lets a packed unit have, and often
        # exactly the most it lets: (nb - overhead - 1) // 4
        most = (nb - (8 + 8 * ways) - 1) // 4
        nw = (np.maximum(most, 0) * 1.5 * rng.random(U)).astype(np.int64)
        top = (rng.random(U) < 0.3) & (most >= 0)
        nw[top] = most[top]
        cls = planes.unit_class(np.where(const, 5, 0), np.where(const, 5, 9), np.zeros(U), nw,
                                nb, ways)
        pk = cls == planes.CLASS_PACKED
        assert np.array_equal(pk, ~const & (nw <= most))
        assert np.array_equal(cls == planes.CLASS_CONSTANT, const)
        size = planes.plane_section_bytes(U, int(const.sum()),
                                          int(nb[cls == planes.CLASS_RAW].sum()), nw[pk], ways)
        assert size <= planes.plane_section_bound(sizes, Ce, th, tw)
    # and it is tight up to the bitmaps' rounding: all raw
    assert planes.plane_section_bytes(6, 0, sum(NB), [], 1) == \
        planes.plane_section_bound(SIZES, 1, 16, 16)
    assert planes.plane_section_bound(SIZES, 0, 16, 16) == 20


# ------------------------------------------------------------------ the interface
def _model(th=16, C=3):
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", 2, 1, th, th, C, _dense(8, 1), _dense(8, 1), 2))


def test_tiled_planes_checks_its_arguments():
    import idfcodec
    from idfcodec.integrity import SealedCodec
    from idfcodec.predict import PredictiveTileCodec
    from idfcodec.safe import SafeTiledCodec
    from idfcodec.tiled import TiledCodec
    assert idfcodec.PlaneSetCodec is planes.PlaneSetCodec
    assert idfcodec.PlaneSetBitstream is planes.PlaneSetBitstream
    model = _model()
    for make in (TiledCodec, SafeTiledCodec, PredictiveTileCodec,
                 lambda m: PredictiveTileCodec(m, colour=True)):
        base = make(model)
        pc = model.tiled_planes(4, base=base)
        assert isinstance(pc, planes.PlaneSetCodec) and pc.base is base
        assert (pc.Cs, pc.Cb, pc.Ce, pc.predict_ways) == (4, 3, 1, 1)
    base = PredictiveTileCodec(model)
    assert (model.tiled_planes(1, base=base).Cb, model.tiled_planes(2, base=base).Ce) == (0, 2)
    assert model.tiled_planes(3, base=base).Ce == 0
    assert model.tiled_planes(5, base=base, predict_ways=8).predict_ways == 8
    for bad in (0, -2, 2.0, "4"):
        with pytest.raises(ValueError, match="channels"):
            model.tiled_planes(bad, base=base)
    with pytest.raises(ValueError, match="sealed base"):
        model.tiled_planes(4, base=SealedCodec(base))
    with pytest.raises(ValueError, match="another model"):
        model.tiled_planes(4, base=PredictiveTileCodec(_model()))
    with pytest.raises(TypeError, match="tiled codec"):
        model.tiled_planes(4, base=model)
    for bad in (4, 128, 0, 2, "8"):
        with pytest.raises(ValueError, match="predict_ways"):
            model.tiled_planes(4, base=base, predict_ways=bad)
    big = _model(256)
    assert big.tiled_planes(4, base=PredictiveTileCodec(big)).predict_ways == 1
    with pytest.raises(ValueError, match="LDS"):
        big.tiled_planes(4, base=PredictiveTileCodec(big), predict_ways=8)


def test_check_bitstream_refuses_files_of_another_geometry():
    from idfcodec.predict import PredictiveTileCodec
    from idfcodec.safe import SafeTiledCodec
    model = _model()
    base = PredictiveTileCodec(model)
    model.tiled_planes(4, base=base).check_bitstream(_hand(3, 1))
    model.tiled_planes(2, base=base).check_bitstream(_hand(0, 2, 8))
    m8 = _model(8)
    with pytest.raises(ValueError, match=r"tiles \(16, 16\) does not match"):
        planes.PlaneSetCodec(m8, 2, PredictiveTileCodec(m8)).check_bitstream(_hand(0, 2))
    m4 = _model(16, 4)
    with pytest.raises(ValueError, match="does not fit the model's C 4"):
        planes.PlaneSetCodec(m4, 4, PredictiveTileCodec(m4)).check_bitstream(_hand(3, 1))
    with pytest.raises(ValueError, match="4 channels, the codec codes 5"):
        model.tiled_planes(5, base=base).check_bitstream(_hand(3, 1))
    with pytest.raises(ValueError, match="base"):
        model.tiled_planes(4, base=SafeTiledCodec(model)).check_bitstream(_hand(3, 1))


def test_file_tool_tells_plane_sets_by_their_channels(tmp_path):
    import importlib.util
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    px = np.arange(5 * 7 * 4, dtype=np.uint8).reshape(5, 7, 4)
    paths = {k: str(tmp_path / k) for k in ("g.pgm", "c.ppm", "rgba.npy", "ga.npy", "hw.npy",
                                            "rgb.npy")}
    with open(paths["g.pgm"], "wb") as f:
        f.write(b"P5\n7 5\n255\n" + px[..., 0].tobytes())
    with open(paths["c.ppm"], "wb") as f:
        f.write(b"P6\n7 5\n255\n" + px[..., :3].tobytes())
    np.save(paths["rgba.npy"], px)                                  # [H, W, 4]
    np.save(paths["ga.npy"], px[..., :2].transpose(2, 0, 1))        # [2, H, W]
    np.save(paths["hw.npy"], px[..., 0])
    np.save(paths["rgb.npy"], px[..., :3].transpose(2, 0, 1))
    have = {k: tool.file_channels(p, 3) for k, p in paths.items()}
    assert have == {"g.pgm": 1, "c.ppm": 3, "rgba.npy": 4, "ga.npy": 2, "hw.npy": 1, "rgb.npy": 3}
    # files of the model's own channel count keep their path
    assert tool.plane_set_channels([paths["c.ppm"], paths["rgb.npy"]], 3) is None
    assert tool.plane_set_channels([paths["g.pgm"], paths["hw.npy"]], 3) == 1
    assert tool.plane_set_channels([paths["rgba.npy"]], 3) == 4
    with pytest.raises(SystemExit, match="one channel count"):
        tool.plane_set_channels([paths["g.pgm"], paths["rgba.npy"]], 3)
    a, layout = tool.read_image_stored(paths["rgba.npy"], 4)
    assert layout == "hwc" and np.array_equal(a, px)
    a, layout = tool.read_image_stored(paths["ga.npy"], 2)
    assert layout == "chw" and a.shape == (2, 5, 7)
    # an IDFM file is read by its magic before the other containers' readers see it
    assert _hand().to_bytes()[:4] == planes.MAGIC == b"IDFM"


def test_entry_points_check_their_arguments_without_a_device():
    from idfcodec import _lib
    lib = _lib.lib()
    one = 1 << 12       # any non-null value: nothing is launched
    assert lib.idf_segment_range_u8(None, -1, one, one, one) == 1
    assert lib.idf_segment_fill_u8(None, -1, one, one, one, one) == 1
    assert lib.idf_segment_range_u8(None, 1 << 31, one, one, one) == 1
    assert lib.idf_segment_fill_u8(None, 1 << 31, one, one, one, one) == 1
    for k in range(3):
        a = [one] * 3
        a[k] = None
        assert lib.idf_segment_range_u8(None, 1, *a) == 1
    for k in range(4):
        a = [one] * 4
        a[k] = None
        assert lib.idf_segment_fill_u8(None, 1, *a) == 1
    # a count of 0 launches nothing and reads no pointer
    assert lib.idf_segment_range_u8(None, 0, None, None, None) == 0
    assert lib.idf_segment_fill_u8(None, 0, None, None, None, None) == 0
    assert _lib.ERR_NAMES[1] == "IDF_ERR_ARG"
