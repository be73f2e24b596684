"""The colour mode of the predictive coder on the host (no device), in two parts.

The reference tests (round trip, two tables, choice by content, wrap) pin down the numpy
restatement tests/colour_ref.py and nothing of the product: they pass whatever idfcodec holds, and
are here so that the device tests compare against a reference that is itself held to the model.

The product tests need the feature: the cost rule and the stream choice of idfcodec.predict, the
launchers' refusals, the IDFQ container with every refusal of its reader, its size bound, the
codec's refusal of C < 3 and the file tool."""
import functools
import struct

import numpy as np
import pytest
import torch

import colour_ref as cref
import predict_ref as ref
from idfcodec import predict  # the module under test: every test here needs it
from test_predict_host import MIXED, PACKED, _pred, contents
from test_safe_host import C, RAW, SIZES

RECTS = [(1, 1), (1, 16), (16, 1), (5, 5), (12, 8), (16, 16), (40, 33)]
CHOICE_RECTS = [(16, 16), (12, 8), (40, 33)]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("Cc", [3, 4])
@pytest.mark.parametrize("h,w", RECTS, ids=lambda v: str(v))
def test_reference_decodes_its_own_colour_encoding(Cc, h, w):
    cases = dict(contents((Cc, h, w)))
    cases["correlated"] = cref.correlated(h, w, 0, Cc)
    cases["independent"] = cref.independent(h, w, 0, Cc)
    for name, p in cases.items():
        sel, sel2, state, words = cref.encode(p)
        out, final, status = cref.decode(sel, sel2, state, words, Cc, h, w)
        assert np.array_equal(out, p) and final == ref.L and status == 0, name
        t = cref.transform(p)
        assert np.array_equal(cref.inverse(t), p)
        assert np.array_equal(t[1], p[1]) and np.array_equal(t[3:], p[3:])
        x, mean, scale = cref.arrays(p, sel, sel2)
        assert x[-1] == t[0, 0, 0] / 256 and mean[-1] == 0.5    # pixel 0 is the last symbol
        # the symbols are predict_ref's of t wherever the two tables agree
        xr, mr, _ = ref.arrays(t, sel)
        assert np.array_equal(x, xr) and np.array_equal(mean, mr)


def test_two_tables_come_from_their_plane_groups():
    p = cref.correlated(16, 16, 1, 4)
    t = cref.transform(p)
    sel, sel2 = cref.choose_sels(p)
    # the rule of predict_ref on each group's planes alone (stacking keeps planes apart)
    assert sel == ref.choose_sel(t[[1, 3]]) and sel2 == ref.choose_sel(t[[0, 2]])
    _, _, scale = cref.arrays(p, sel, sel2)
    per_plane = scale[::-1].reshape(4, 16, 16)
    _, k = ref.predict(t)
    for pl, table in enumerate((sel2, sel, sel2, sel)):
        assert np.array_equal(per_plane[pl], ref.SCALE[(table >> (4 * k[pl])) & 15])


@functools.lru_cache(maxsize=None)
def _choice(gen, h, w, seed):
    return cref.choice(getattr(cref, gen)(h, w, seed))


@pytest.mark.parametrize("h,w", CHOICE_RECTS, ids=lambda v: str(v))
def test_reference_chooses_by_content(h, w):
    for seed in range(3):
        kind, cost = _choice("correlated", h, w, seed)
        plain = cref.choice(cref.correlated(h, w, seed), colour=False)
        assert kind == "colour" and cost < plain[1], (seed, cost, plain)
        kind, cost = _choice("independent", h, w, seed)
        assert kind == "plain", (seed, kind, cost)
        assert (kind, cost) == cref.choice(cref.independent(h, w, seed), colour=False)
    for gen in (cref.correlated, cref.independent, cref.noise):
        assert cref.choice(gen(1, 1, 0)) == ("raw", 3)


def test_colour_cost_is_twenty_bytes_and_a_tie_stays_plain():
    assert predict.ENTRY_BYTES_COLOUR == cref.ENTRY_BYTES_COLOUR == 20
    assert predict.MAGIC_COLOUR == b"IDFQ"
    # 20 + 4 * nw_c < 16 + 4 * nw_p  <=>  nw_c + 1 < nw_p
    got = predict.is_colour([10, 10, 10, 0, 1, 2], [8, 9, 10, 0, 0, 0])
    assert got.tolist() == [True, False, False, False, False, True]


def test_stream_choice_is_the_cost_rule_per_entry():
    """choose_streams: stream 2k is entry k's plain candidate, 2k + 1 its colour candidate; the
    cheaper is picked (a tie stays plain) and packed iff its cost is below the entry's bytes (a
    tie stores raw) and its status is 0."""
    #        plain/colour words: colour wins, tie -> plain, plain wins, colour wins but raw, status
    nw = [10, 8, 10, 9, 3, 9, 10, 8, 10, 8]
    status = [0, 0, 0, 0, 0, 0, 0, 0, 0, 16]
    counts = [53, 57, 28, 52, 53]
    col, pick, hit = predict.choose_streams(nw, status, counts)
    assert col.tolist() == [True, False, False, True, True]
    assert pick.tolist() == [1, 2, 4, 7, 9]
    # costs 52, 56, 28, 52, 52 against 53, 57, 28, 52, 53; the last stream is flagged
    assert hit.tolist() == [True, True, False, False, False]


def test_wrap_is_mod_256():
    h, w = 8, 16
    half = np.arange(w) >= w // 2
    p = np.zeros((3, h, w), dtype=np.uint8)
    p[0][:, ~half], p[1][:, ~half] = 255, 0
    p[0][:, half], p[1][:, half] = 0, 255
    p[2] = p[1]
    t = cref.transform(p)
    assert (t[0][:, ~half] == (255 - 0 + 128) % 256).all() and (t[0][:, ~half] == 127).all()
    assert (t[0][:, half] == (0 - 255 + 128) % 256).all() and (t[0][:, half] == 129).all()
    assert (t[2] == 128).all() and np.array_equal(t[1], p[1])
    sel, sel2, state, words = cref.encode(p)
    out, final, status = cref.decode(sel, sel2, state, words, 3, h, w)
    assert np.array_equal(out, p) and final == ref.L and status == 0


def test_launchers_refuse_bad_arguments_before_any_launch():
    """IDF_ERR_ARG (1) as for the plain entry points, and for C < 3 wherever a colour entry is
    named.  None of these reaches the device."""
    from idfcodec._lib import lib
    L = lib()
    one = 8  # any non-NULL address: the calls below return before it is read
    prep = lambda n, Cc, th, tw, p=one: L.idf_predict_prep2_u8(  # noqa: E731
        None, n, Cc, th, tw, p, p, p, p, p, p)
    dec = lambda n, q, Cc, th, tw, p=one: L.idf_predict_decode2_u8(  # noqa: E731
        None, n, q, Cc, th, tw, p, p, p, p, p, p, p, p, p, p, p, p)
    inv = lambda n, Cc, th, tw, p=one: L.idf_predict_colour_inverse_u8(  # noqa: E731
        None, n, Cc, th, tw, p, p, p, p)
    for call in (prep, inv):
        assert call(0, 3, 16, 16, None) == 0
        assert call(1, 3, 16, 16, None) == 1
        assert call(-1, 3, 16, 16) == 1
        for Cc, th, tw in ((0, 16, 16), (1, 16, 16), (2, 16, 16), (5, 16, 16), (3, 0, 16),
                           (3, 16, 0)):
            assert call(1, Cc, th, tw) == 1 and call(0, Cc, th, tw) == 1
    assert dec(0, 0, 3, 16, 16, None) == 0
    assert dec(1, 0, 3, 16, 16, None) == 1 and dec(1, 1, 3, 16, 16, None) == 1
    assert dec(-1, 0, 3, 16, 16) == 1
    assert dec(1, 2, 3, 16, 16) == 1 and dec(1, -1, 3, 16, 16) == 1     # n_colour outside [0, n]
    for Cc in (1, 2):
        assert dec(1, 1, Cc, 16, 16) == 1                               # a colour entry of C < 3
    assert dec(1, 1, 3, 16, 32769) == 4
    # sel2 and the flags may be NULL only where no entry is a colour entry
    args = [one] * 12
    args[5] = args[6] = None
    assert L.idf_predict_decode2_u8(None, 1, 1, 3, 16, 16, *args) == 1


# ------------------------------------------------------------------ the container
COLOUR = [False, False, True, False, False, False]      # of the packed entries 2 and 5, entry 2


def _col(escaped=MIXED, packed=PACKED, colour=COLOUR):
    """test_predict_host._pred with colour flags; colour entry number q holds sel2 0x89ABCDEF + q"""
    pbs = _pred(escaped, packed)
    pbs.colour = np.asarray(colour, dtype=bool)
    pbs.sel2 = np.arange(int(pbs.colour.sum()), dtype=np.uint32) + np.uint32(0x89ABCDEF)
    return pbs


@pytest.mark.parametrize("escaped,packed,colour", [
    (MIXED, PACKED, COLOUR), (MIXED, PACKED, [False] * 6), (MIXED, PACKED, PACKED),
    (MIXED, [False] * 6, [False] * 6), ([True] * 6, [True] * 6, [True, False] * 3),
    ([False] * 6, [False] * 6, [False] * 6)])
def test_idfq_round_trip_and_layout(escaped, packed, colour):
    from idfcodec.predict import PredictiveTiledBitstream
    pbs = _col(escaped, packed, colour)
    plain = _pred(escaped, packed).to_bytes()
    buf = pbs.to_bytes()
    E, P, Q, K = sum(escaped), sum(packed), sum(colour), 6 - sum(escaped)
    assert buf[:4] == b"IDFQ"
    n_cmap = -(-P // 8)
    assert len(buf) == len(plain) + n_cmap + 4 + 4 * Q
    o = 24 + 8 * len(SIZES) + 1 + -(-E // 8)
    assert buf[4:o] == plain[4:o]                       # the header, escape and packed bitmaps
    pk = [e for e in range(6) if packed[e]]
    if P:
        assert buf[o] == sum(1 << i for i, e in enumerate(pk) if colour[e])
    o += n_cmap
    n_raw = sum(RAW[e] for e in range(6) if escaped[e] and not packed[e])
    assert struct.unpack_from("<Q", buf, o)[0] == n_raw
    o += 8 + n_raw
    n_words = sum(p + 2 for p in range(P))
    assert struct.unpack_from("<QI", buf, o) == (4 + 16 * P + 4 + 4 * Q + 4 * n_words, P)
    o += 12 + 16 * P
    assert struct.unpack_from("<I", buf, o)[0] == Q
    if Q:
        assert struct.unpack_from("<I", buf, o + 4)[0] == 0x89ABCDEF
    if P:
        assert struct.unpack_from("<II", buf, o + 4 + 4 * Q) == (0, 1)      # the first words
    got = PredictiveTiledBitstream.from_bytes(buf)
    assert got.to_bytes() == buf
    assert got.colour.tolist() == list(colour) and got.packed.tolist() == list(packed)
    assert got.n_colour == Q and np.array_equal(got.sel2, pbs.sel2)
    assert np.array_equal(got.sel, pbs.sel) and torch.equal(got.words, pbs.words)
    assert got.bits() == _pred(escaped, packed).bits() + 32 * Q
    assert got.bits() == ((pbs.stream.bits() if K else 0) + 8 * n_raw + 128 * (P - Q) + 160 * Q
                          + 32 * n_words)


def test_idfp_still_parses_and_writes_as_before():
    from idfcodec.predict import PredictiveTiledBitstream
    buf = _pred(MIXED, PACKED).to_bytes()
    got = PredictiveTiledBitstream.from_bytes(buf)
    assert got.colour is None and got.sel2 is None and got.n_colour == 0
    assert got.to_bytes() == buf and buf[:4] == b"IDFP"
    # positional construction without the new fields
    assert _pred(MIXED, PACKED).colour is None


def _patched(raw, fmt, offset, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_idfq_errors():
    from idfcodec.predict import PredictiveTiledBitstream as PB
    buf = _col().to_bytes()
    o_map = 24 + 8 * len(SIZES)
    o_cmap = o_map + 2
    o_raw = o_cmap + 1                                      # the u64 raw length
    o_sect = o_raw + 8 + RAW[0]                             # the u64 section length
    n_sect = 4 + 16 * 2 + 4 + 4 * 1 + 4 * 5
    o_q = o_sect + 8 + 4 + 16 * 2                           # the u32 Q
    o_inner = o_sect + 8 + n_sect
    assert struct.unpack_from("<Q", buf, o_sect)[0] == n_sect
    assert struct.unpack_from("<I", buf, o_q)[0] == 1 and buf[o_cmap] == 1

    def refused(b, text):
        with pytest.raises(ValueError, match=text):
            PB.from_bytes(b)

    refused(b"IDFR" + buf[4:], "not an IDF")
    refused(buf[:10], "truncated .*header")
    refused(buf[:o_map], "truncated .*escape bitmap")
    refused(buf[:o_map + 1], "truncated .*packed bitmap")
    refused(buf[:o_cmap], "truncated .*colour bitmap")
    refused(buf[:o_raw + 4], "truncated .*colour bitmap")   # the raw length is cut
    refused(buf[:o_raw + 8 + 1], "truncated .*raw bytes")
    refused(buf[:o_sect + 8 + 10], "truncated .*packed section")
    refused(buf[:o_inner + 4], "truncated .*packed section")  # the inner length is cut
    refused(buf[:-1], "inner bytes")
    refused(buf + b"\0", "inner bytes")
    # a colour bit past the 2 packed entries
    refused(_patched(buf, "<B", o_cmap, buf[o_cmap] | 0x04), "colour bits past")
    # Q against the bitmap, either way
    refused(_patched(buf, "<I", o_q, 2), "names 2 colour tiles, its bitmap 1")
    refused(_patched(buf, "<B", o_cmap, 3), "names 1 colour tiles, its bitmap 2")
    refused(_patched(buf, "<B", o_cmap, 0), "names 1 colour tiles, its bitmap 0")
    # a word count against the section's length
    refused(_patched(buf, "<I", o_sect + 8 + 4 + 12 * 2, 3), "word counts")
    # a section too short for Q, and for its second tables
    short = buf[:o_sect] + struct.pack("<Q", 4 + 32) + buf[o_sect + 8:o_q] + buf[o_inner:]
    refused(short, "too short for the count of its second tables")
    short = (buf[:o_sect] + struct.pack("<Q", 4 + 32 + 4) + buf[o_sect + 8:o_q + 4]
             + buf[o_inner:])
    refused(short, "too short for the second tables")
    # the packed bit of the colour entry cleared: its colour bit now lies past the packed entries
    refused(_patched(buf, "<B", o_map + 1, buf[o_map + 1] & ~0x02), "raw bytes|colour bits past")
    # an IDFP body under the IDFQ magic and the reverse
    with pytest.raises(ValueError):
        PB.from_bytes(b"IDFQ" + _pred(MIXED, PACKED).to_bytes()[4:])
    with pytest.raises(ValueError):
        PB.from_bytes(b"IDFP" + buf[4:])
    # writer checks: a colour flag on an entry that is not packed, a row too many, C < 3
    bad = _col(colour=[True, False, True, False, False, False])
    with pytest.raises(ValueError, match="does not pack"):
        bad.to_bytes()
    bad = _col()
    bad.sel2 = np.zeros(2, np.uint32)
    with pytest.raises(ValueError, match="second tables"):
        bad.to_bytes()
    bad = _col()
    bad.colour = bad.colour[:5]
    with pytest.raises(ValueError, match="colour flags"):
        bad.to_bytes()
    assert C >= 3


def test_a_colour_file_of_one_plane_is_refused():
    from idfcodec.predict import PredictiveTiledBitstream as PB
    P1 = PB(None, [(16, 16)], 1, (16, 16), np.array([True]), np.array([True]),
            torch.zeros(0, dtype=torch.uint8), np.zeros(1, np.uint32),
            np.full(1, 1 << 32, np.uint64), np.zeros(1, np.int64),
            torch.zeros(0, dtype=torch.int32), None, np.array([False]), np.zeros(0, np.uint32))
    buf = P1.to_bytes()                                  # no colour entry: a valid IDFQ file
    assert PB.from_bytes(buf).n_colour == 0
    o_cmap = 24 + 8 + 2
    with pytest.raises(ValueError, match="C 1 flags colour"):
        PB.from_bytes(_patched(buf, "<B", o_cmap, 1))
    P1.colour, P1.sel2 = np.array([True]), np.zeros(1, np.uint32)
    with pytest.raises(ValueError, match="C 1 flags colour"):
        P1.to_bytes()


# ------------------------------------------------------------------ the size bound
@pytest.mark.parametrize("n_lvl", [1, 2])
def test_colour_size_bound_is_the_stated_arithmetic(n_lvl):
    """An entry costs at most its plain cost, which is below its bytes, so the IDFQ file stays
    within the IDFP bound plus the colour bitmap (at most ceil(N / 8) bytes) and the u32 Q."""
    from idfcodec.predict import PredictiveTiledBitstream, file_size_bound_packed
    from test_predict_host import _bound_case
    rng = np.random.default_rng(11 * n_lvl)
    for sizes, (th, tw) in (([(1, 1), (16, 16), (17, 16), (5, 40), (37, 21)], (16, 16)),
                            ([(64, 64)], (16, 16)), ([(25, 9), (12, 8)], (12, 8))):
        for _ in range(4):
            pbs, K, P = _bound_case(rng, sizes, th, tw, n_lvl, 1.0)
            N = len(pbs.escaped)
            plain = file_size_bound_packed(sizes, C, th, tw, n_lvl, kept=bool(K))
            bound = file_size_bound_packed(sizes, C, th, tw, n_lvl, kept=bool(K), colour=True)
            assert bound == plain + -(-N // 8) + 4
            # the packed entries whose words leave room for sel2 become colour entries
            n_bytes = predict.entry_bytes([pbs.rects()[e] for e in np.flatnonzero(pbs.packed)], C)
            room = 20 + 4 * pbs.nwords < n_bytes
            pbs.colour = np.zeros(N, dtype=bool)
            pbs.colour[np.flatnonzero(pbs.packed)[room]] = True
            pbs.sel2 = np.zeros(int(room.sum()), np.uint32)
            buf = pbs.to_bytes()
            assert len(buf) <= bound and pbs.bits() <= 8 * sum(C * H * W for H, W in sizes)
            assert PredictiveTiledBitstream.from_bytes(buf).to_bytes() == buf


# ------------------------------------------------------------------ the interface
def _model(Cc):
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", 2, 1, 8, 8, Cc, _dense(8, 1), _dense(8, 1), 2))


def test_colour_needs_three_planes():
    with pytest.raises(ValueError, match="C >= 3"):
        predict.PredictiveTileCodec(_model(1), colour=True)
    assert predict.PredictiveTileCodec(_model(1)).colour is False
    pc = predict.PredictiveTileCodec(_model(3), max_batch=3, colour=True)
    assert pc.colour and pc.max_batch == 3 and pc.tile_hw == (8, 8)


def test_file_tool_reads_idfq_by_magic():
    import importlib.util
    import os
    from conftest import REPO
    from idfcodec.predict import PredictiveTiledBitstream
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pbs = _col()
    got, safe = tool.read_container(pbs.to_bytes(), None)
    assert safe and isinstance(got, PredictiveTiledBitstream) and got.n_colour == 1
    assert got.to_bytes() == pbs.to_bytes()
