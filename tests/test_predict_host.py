"""The predictive coder of escaped tiles on the host (no device): the numpy reference decodes its
own encoding, the header's literals are the issue's formulas, the sel rule at its edges, the IDFP
container and every refusal of its reader, and the size bound, derived and not measured."""
import hashlib
import struct

import numpy as np
import pytest
import torch

import predict_ref as ref
from idfcodec import predict  # the module under test: every test here needs it
from test_safe_host import C, RAW, RECTS, SIZES, _hand_bitstream

# (C, h, w): 1x1, 1x16, 16x1, 5x5, full tiles of 16x16 and 12x8, and the 40x33 tile
SHAPES = [(1, 1, 1), (3, 1, 16), (4, 16, 1), (3, 5, 5), (3, 16, 16), (1, 12, 8), (1, 40, 33)]


def contents(shape, seed=0):
    """name -> uint8 [C, h, w]: constants, a smooth ramp, vertical and horizontal 0 / 255 steps
    (c >= max, c <= min, delta = 510) and uniform noise."""
    Cc, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.arange(Cc).reshape(Cc, 1, 1)
    rng = np.random.default_rng(seed + 131 * h + w)
    full = lambda v: np.broadcast_to(v, shape).astype(np.uint8).copy()  # noqa: E731
    return {"zeros": full(0), "ones": full(255),
            "ramp": full((3 * yy + 2 * xx + 40 * ch) % 256),
            "vstep": full(np.where(xx >= (w + 1) // 2, 255, 0)),
            "hstep": full(np.where(yy >= (h + 1) // 2, 0, 255)),
            "noise": rng.integers(0, 256, shape, dtype=np.uint8)}


# ------------------------------------------------------------------ the model
def test_header_literals_are_the_formulas():
    scale, t = predict.tables()
    assert scale.dtype == np.float32 and np.array_equal(scale, ref.SCALE)
    assert np.array_equal(t, ref.T)
    assert float(scale[0]) * 256 == 0.5 and abs(float(scale[15]) * 256 - 90.5097) < 1e-3
    assert (np.diff(t) > 0).all()


def test_predict_neighbours_med_and_buckets():
    p = np.array([[[10, 20, 30], [40, 0, 255], [255, 255, 0]]], dtype=np.uint8)
    pred, k = ref.predict(p)
    # (0,0): 128; row 0: the left byte; column 0: the byte above
    assert pred[0, 0].tolist() == [128, 10, 20] and pred[0, :, 0].tolist() == [128, 10, 40]
    assert (k[0, 0] == 0).all() and (k[0, :, 0] == 0).all()
    # (1,1): a 40, b 20, c 10 <= min -> max = 40; delta 30 + 10 = 40 -> 1 + floor(log2 41) = 6
    assert pred[0, 1, 1] == 40 and k[0, 1, 1] == 6
    # (1,2): a 0, b 30, c 20: between -> a + b - c = 10; delta 20 + 10 -> 1 + 4
    assert pred[0, 1, 2] == 10 and k[0, 1, 2] == 5
    # (2,1): a 255, b 0, c 40: between -> 215;  (2,2): a 255, b 255, c 0 <= min -> 255, delta 510
    assert pred[0, 2, 1] == 215 and pred[0, 2, 2] == 255 and k[0, 2, 2] == 7
    flat = np.full((1, 4, 4), 9, np.uint8)
    assert (ref.predict(flat)[1][0, 1:, 1:] == 1).all()       # delta 0 -> bucket 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_decodes_its_own_encoding(shape):
    for name, p in contents(shape).items():
        if shape[1] * shape[2] > 400 and name not in ("ramp", "noise"):
            continue  # the serial decoder calls the oracle per probe: two contents at 40x33
        sel, state, words = ref.encode(p)
        out, final, status = ref.decode(sel, state, words, *shape)
        assert np.array_equal(out, p) and final == ref.L and status == 0, name
        x, mean, scale = ref.arrays(p, sel)
        assert x[-1] == p[0, 0, 0] / 256 and mean[-1] == 0.5    # pixel 0 is the last symbol
        assert set(scale.tolist()) <= set(ref.SCALE.tolist())


def test_sel_rule_edges():
    T = [int(t) for t in ref.T]
    assert ref.choose_j(0, 0) == 0 and ref.choose_j(10 ** 9, 0) == 0       # an empty bucket
    assert ref.choose_j(0, 5) == 0
    # an exact tie 1024 * S == n * T[j] takes j; one more takes j + 1
    for j in (0, 3, 14):
        assert ref.choose_j(T[j], 1024) == j
        assert ref.choose_j(T[j] + 1, 1024) == j + 1
    assert ref.choose_j(255 * 1024, 1024) == 15
    # every nibble 15: a checkerboard of 0 / 255 misses by 255 everywhere but on the borders
    yy, xx = np.mgrid[0:16, 0:16]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[None]
    sel = ref.choose_sel(board)
    assert sel >> 28 == 15 and sel & 15 == 15
    # constant bytes: bucket 0 pays only for the first pixel, bucket 1 nothing, the rest are empty
    assert ref.choose_sel(np.full((1, 16, 16), 128, np.uint8)) == 0


def test_device_rule_is_the_reference_rule():
    """is_packed: status 0 and 16 + 4 * nwords < bytes; a tie stores raw."""
    from idfcodec.predict import entry_bytes, is_packed
    assert entry_bytes(RECTS, C).tolist() == RAW
    got = is_packed([0, 0, 0, 16, 0], [7, 8, 0, 0, 2], [48, 48, 16, 48, 3])
    assert got.tolist() == [True, False, False, False, False]


def test_launchers_refuse_bad_arguments_before_any_launch():
    """IDF_ERR_ARG (1) for a NULL pointer where n > 0, C outside 1..4, a tile size below 1 and a
    negative count; n == 0 is IDF_OK without a launch.  None of these reaches the device."""
    from idfcodec._lib import lib
    L = lib()
    one = 8  # any non-NULL address: the calls below return before it is read
    prep = lambda n, C, th, tw, p=one: L.idf_predict_prep_u8(  # noqa: E731
        None, n, C, th, tw, p, p, p, p, p, p)
    dec = lambda n, C, th, tw, p=one: L.idf_predict_decode_u8(  # noqa: E731
        None, n, C, th, tw, p, p, p, p, p, p, p, p, p, p)
    for call in (prep, dec):
        assert call(0, 3, 16, 16, None) == 0
        assert call(1, 3, 16, 16, None) == 1
        assert call(-1, 3, 16, 16) == 1
        for C, th, tw in ((0, 16, 16), (5, 16, 16), (3, 0, 16), (3, 16, 0), (3, -1, 16)):
            assert call(1, C, th, tw) == 1 and call(0, C, th, tw) == 1
    assert dec(1, 3, 16, 32769) == 4                    # IDF_ERR_UNSUPPORTED: a row lives in LDS
    assert L.idf_predict_tables(None, None) == 1
    # each pointer alone
    for i in range(6):
        args = [one] * 6
        args[i] = None
        assert L.idf_predict_prep_u8(None, 1, 3, 16, 16, *args) == 1
    for i in range(10):
        args = [one] * 10
        args[i] = None
        assert L.idf_predict_decode_u8(None, 1, 3, 16, 16, *args) == 1


# ------------------------------------------------------------------ the container
MIXED = [True, False, True, False, False, True]
PACKED = [False, False, True, False, False, True]     # entry 0 raw, 2 and 5 packed


def _pred(escaped, packed):
    """A PredictiveTiledBitstream over SIZES: raw byte j of entry e is (7 * e + j) % 251, packed
    entry number p holds p + 2 words 1000 * p + j, sel 0x01234567 + p, state L + 5 + p."""
    from idfcodec.predict import PredictiveTiledBitstream
    escaped, packed = np.asarray(escaped, dtype=bool), np.asarray(packed, dtype=bool)
    K = int((~escaped).sum())
    raw = [np.arange(RAW[e], dtype=np.int64) + 7 * e for e in range(6) if escaped[e] and
           not packed[e]]
    raw = (np.concatenate(raw) % 251).astype(np.uint8) if raw else np.zeros(0, np.uint8)
    P = int(packed.sum())
    nw = np.arange(P, dtype=np.int64) + 2
    words = np.array([1000 * p + j for p in range(P) for j in range(p + 2)], dtype=np.int32)
    return PredictiveTiledBitstream(
        _hand_bitstream(K) if K else None, list(SIZES), C, (16, 16), escaped, packed,
        torch.from_numpy(raw), np.arange(P, dtype=np.uint32) + 0x01234567,
        np.arange(P, dtype=np.uint64) + np.uint64((1 << 32) + 5), nw, torch.from_numpy(words))


@pytest.mark.parametrize("escaped,packed", [(MIXED, PACKED), (MIXED, [False] * 6), (MIXED, MIXED),
                                            ([True] * 6, [True] * 6), ([False] * 6, [False] * 6)])
def test_idfp_round_trip_and_layout(escaped, packed):
    from idfcodec.predict import PredictiveTiledBitstream
    pbs = _pred(escaped, packed)
    buf = pbs.to_bytes()
    E, P, K = sum(escaped), sum(packed), 6 - sum(escaped)
    assert buf[:4] == b"IDFP"
    o = 24 + 8 * len(SIZES)
    assert buf[o] == sum(1 << e for e in range(6) if escaped[e])
    esc = [e for e in range(6) if escaped[e]]
    n_pmap = -(-E // 8)
    if E:
        assert buf[o + 1] == sum(1 << i for i, e in enumerate(esc) if packed[e])
    o += 1 + n_pmap
    n_raw = sum(RAW[e] for e in esc if not packed[e])
    assert struct.unpack_from("<Q", buf, o)[0] == n_raw == pbs.raw.numel()
    o += 8 + n_raw
    n_words = sum(p + 2 for p in range(P))
    assert struct.unpack_from("<QI", buf, o) == (4 + 16 * P + 4 * n_words, P)
    if P:
        assert struct.unpack_from("<I", buf, o + 12)[0] == 0x01234567
        assert struct.unpack_from("<Q", buf, o + 12 + 4 * P)[0] == (1 << 32) + 5
        assert struct.unpack_from("<I", buf, o + 12 + 12 * P)[0] == 2
        assert struct.unpack_from("<II", buf, o + 12 + 16 * P) == (0, 1)
    o += 8 + 4 + 16 * P + 4 * n_words
    inner = pbs.stream.to_bytes() if K else b""
    assert struct.unpack_from("<Q", buf, o)[0] == len(inner) and buf[o + 8:] == inner
    got = PredictiveTiledBitstream.from_bytes(buf)
    assert got.to_bytes() == buf
    assert got.escaped.tolist() == list(escaped) and got.packed.tolist() == list(packed)
    assert got.n_packed == P and got.n_kept == K
    assert np.array_equal(got.sel, pbs.sel) and np.array_equal(got.states, pbs.states)
    assert np.array_equal(got.nwords, pbs.nwords) and torch.equal(got.words, pbs.words)
    assert torch.equal(got.raw, pbs.raw)
    assert got.bits() == (pbs.stream.bits() if K else 0) + 8 * n_raw + 128 * P + 32 * n_words


def test_idfp_bytes_are_frozen():
    assert hashlib.sha256(_pred(MIXED, PACKED).to_bytes()).hexdigest() == \
        "cbdaa07fe420b1c402ae6e41a5e4fac0521fac36b6753031fd3ff00402a69cc7"


def test_idfp_packed_bitmap_of_more_than_one_byte():
    from idfcodec.predict import PredictiveTiledBitstream
    sizes = [(16, 16 * 11)]                      # 11 tiles, 10 escaped, 9 packed bits in 2 bytes
    escaped = np.array([True] * 4 + [False] + [True] * 6)
    packed = escaped.copy()
    packed[0] = False
    nw = np.zeros(9, dtype=np.int64)
    pbs = PredictiveTiledBitstream(_hand_bitstream(1), sizes, C, (16, 16), escaped, packed,
                                   torch.zeros(768, dtype=torch.uint8), np.zeros(9, np.uint32),
                                   np.full(9, 1 << 32, np.uint64), nw,
                                   torch.zeros(0, dtype=torch.int32))
    buf = pbs.to_bytes()
    o = 24 + 8
    assert buf[o:o + 2] == bytes([0xEF, 0x07]) and buf[o + 2:o + 4] == bytes([0xFE, 0x03])
    assert PredictiveTiledBitstream.from_bytes(buf).packed.tolist() == packed.tolist()


def _patched(raw, fmt, offset, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_idfp_errors():
    from idfcodec.predict import PredictiveTiledBitstream as PB
    pbs = _pred(MIXED, PACKED)
    buf = pbs.to_bytes()
    o_map = 24 + 8 * len(SIZES)
    o_raw = o_map + 2                                       # the u64 raw length
    o_sect = o_raw + 8 + RAW[0]                             # the u64 section length
    n_sect = 4 + 16 * 2 + 4 * 5
    o_inner = o_sect + 8 + n_sect
    assert struct.unpack_from("<Q", buf, o_sect)[0] == n_sect

    def refused(b, text):
        with pytest.raises(ValueError, match=text):
            PB.from_bytes(b)

    refused(b"IDFS" + buf[4:], "not an IDF")
    refused(buf[:10], "truncated .*header")
    refused(buf[:30], "truncated .*image sizes")
    refused(buf[:o_map], "truncated .*escape bitmap")
    refused(buf[:o_map + 1], "truncated .*packed bitmap")
    refused(buf[:o_raw + 4], "truncated .*packed bitmap")   # the raw length is cut
    refused(buf[:o_raw + 8 + 1], "truncated .*raw bytes")
    refused(buf[:o_sect + 4], "truncated .*raw bytes")      # the section length is cut
    refused(buf[:o_sect + 8 + 10], "truncated .*packed section")
    refused(buf[:o_inner + 4], "truncated .*packed section")  # the inner length is cut
    refused(buf[:-1], "inner bytes")
    refused(buf + b"\0", "inner bytes")                     # trailing bytes
    # bitmap bits past N (6 tiles) and past E (3 escaped)
    refused(_patched(buf, "<B", o_map, buf[o_map] | 0x40), "escape bits past")
    refused(_patched(buf, "<B", o_map + 1, buf[o_map + 1] | 0x08), "packed bits past")
    # a raw length that is not the raw tiles'
    refused(_patched(buf, "<Q", o_raw, RAW[0] + 1), "raw bytes")
    # P against the bitmap
    refused(_patched(buf, "<I", o_sect + 8, 3), "names 3 packed tiles, its bitmap 2")
    # a word count against the section's length
    refused(_patched(buf, "<I", o_sect + 8 + 4 + 12 * 2, 3), "word counts")
    # a section too short for its count, and for its tables
    short = buf[:o_sect] + struct.pack("<Q", 2) + b"\0\0" + buf[o_inner:]
    refused(short, "too short for its count")
    short = buf[:o_sect] + struct.pack("<QI", 4, 2) + buf[o_inner:]
    refused(short, "too short for the tables")
    # a packed bit flipped: the raw length no longer fits
    refused(_patched(buf, "<B", o_map + 1, buf[o_map + 1] ^ 1), "raw bytes")
    # an inner stream over another number of entries
    other = _pred(MIXED, PACKED)
    other.stream = _hand_bitstream(2)
    with pytest.raises(ValueError, match="keeps 3 tiles"):
        other.to_bytes()
    # every nibble pattern is a valid sel
    ok = PB.from_bytes(_patched(buf, "<I", o_sect + 12, 0xFFFFFFFF))
    assert int(ok.sel[0]) == 0xFFFFFFFF
    # writer checks
    bad = _pred(MIXED, PACKED)
    bad.packed = np.array([False, True, True, False, False, True])
    with pytest.raises(ValueError, match="packs a tile it keeps"):
        bad.to_bytes()
    bad = _pred(MIXED, PACKED)
    bad.nwords = bad.nwords + 1
    with pytest.raises(ValueError, match="words"):
        bad.to_bytes()


# ------------------------------------------------------------------ the size bound
def _bound_case(rng, sizes, th, tw, n_lvl, max_ratio):
    """test_safe_host's random file, its escaped entries then packed or not by is_packed on random
    word counts around each entry's break-even."""
    from idfcodec.predict import PredictiveTiledBitstream, entry_bytes, is_packed
    from idfcodec.safe import raw_offsets
    from test_safe_host import _bound_case as safe_case
    sbs, K = safe_case(rng, sizes, th, tw, n_lvl, 1, max_ratio)
    rects = sbs.rects()
    esc = np.flatnonzero(sbs.escaped)
    n_bytes = entry_bytes([rects[e] for e in esc], C)
    nw = np.maximum((n_bytes - 16) // 4 + rng.integers(-3, 4, len(esc)), 0)
    status = np.where(rng.random(len(esc)) < 0.1, 8, 0)
    hit = is_packed(status, nw, n_bytes)
    assert (hit == ((status == 0) & (16 + 4 * nw < n_bytes))).all()
    packed = np.zeros(len(sbs.escaped), dtype=bool)
    packed[esc[hit]] = True
    _, n_raw = raw_offsets(sbs.escaped & ~packed, rects, C)
    P = int(hit.sum())
    return PredictiveTiledBitstream(
        sbs.stream, list(sizes), C, (th, tw), sbs.escaped, packed,
        torch.zeros(n_raw, dtype=torch.uint8), np.zeros(P, np.uint32),
        np.full(P, 1 << 32, np.uint64), nw[hit].astype(np.int64),
        torch.zeros(int(nw[hit].sum()), dtype=torch.int32)), K, P


@pytest.mark.parametrize("n_lvl", [1, 2, 3])
@pytest.mark.parametrize("max_ratio", [1.0, 0.5])
def test_packed_size_bound_holds_for_any_word_counts(n_lvl, max_ratio):
    """A packed entry costs fewer bytes than it holds, so the file stays within the safe bound
    plus what the container adds: the packed bitmap, the section's length and its count."""
    from idfcodec.predict import PredictiveTiledBitstream, file_size_bound_packed
    from idfcodec.safe import file_size_bound
    rng = np.random.default_rng(7 * n_lvl)
    seen = set()
    for sizes, (th, tw) in (([(1, 1), (16, 16), (17, 16), (5, 40), (37, 21)], (16, 16)),
                            ([(64, 64)], (16, 16)), ([(25, 9), (12, 8)], (12, 8)),
                            ([(1, 1)], (16, 16))):
        for _ in range(6):
            pbs, K, P = _bound_case(rng, sizes, th, tw, n_lvl, max_ratio)
            N = len(pbs.escaped)
            src = sum(C * H * W for H, W in sizes)
            bound = file_size_bound(sizes, C, th, tw, n_lvl, kept=bool(K)) + -(-N // 8) + 8 + 4
            assert file_size_bound_packed(sizes, C, th, tw, n_lvl, kept=bool(K)) == bound
            buf = pbs.to_bytes()
            assert len(buf) <= bound, (sizes, K, P, N)
            assert pbs.bits() <= 8 * src
            assert PredictiveTiledBitstream.from_bytes(buf).to_bytes() == buf
            seen.add("packed" if P else "none")
    assert seen == {"packed", "none"}


def test_exports_and_cached_codec():
    import idfcodec
    from idfcodec import safe, synthetic
    from idfcodec.configs import _dense, _flows
    assert idfcodec.PredictiveTileCodec is predict.PredictiveTileCodec
    assert idfcodec.PredictiveTiledBitstream is predict.PredictiveTiledBitstream
    assert issubclass(predict.PredictiveTileCodec, safe.SafeTiledCodec)
    assert predict.MAGIC == b"IDFP" and predict.ENTRY_BYTES == 16
    model = synthetic.build_model(_flows("IDFlows", 2, 1, 8, 8, 3, _dense(8, 1), _dense(8, 1), 2))
    pc = predict.PredictiveTileCodec(model, max_batch=3)
    assert pc.tile_hw == (8, 8) and pc.max_batch == 3 and pc.ways == 1


def test_file_tool_reads_idfp_by_magic():
    import importlib.util
    import os
    from conftest import REPO
    from idfcodec.predict import PredictiveTiledBitstream
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pbs = _pred(MIXED, PACKED)
    got, safe = tool.read_container(pbs.to_bytes(), None)
    assert safe and isinstance(got, PredictiveTiledBitstream)
    assert got.to_bytes() == pbs.to_bytes()
