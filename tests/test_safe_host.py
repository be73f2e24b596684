"""The raw-tile escape on the host (no device): the IDFS container and every refusal of its
reader, the keep rule on hand-made word counts / status flags / sizes, the entry -> inner-index
and entry -> raw-offset maps, and the size bound, derived from the rule and not measured."""
import math
import struct

import numpy as np
import pytest
import torch

SIZES = [(1, 1), (17, 16), (5, 40)]     # 1 + 2 + 3 tiles at 16x16
# in-image part of every entry: 1x1 | 16x16, 1x16 | 5x16, 5x16, 5x8
RECTS = [(1, 1), (16, 16), (1, 16), (5, 16), (5, 16), (5, 8)]
C = 3
RAW = [C * h * w for h, w in RECTS]     # 3, 768, 48, 240, 240, 120


def _hand_bitstream(N, n_lvl=2, ways=1):
    """Stream (l, e) holds nw = (3 * l + e) % 4 words of value 100 * (l * N + e) + j."""
    from idfcodec.codec import Bitstream
    nw = [(3 * l + e) % 4 for l in range(n_lvl) for e in range(N)]
    words = [100 * k + j for k, n in enumerate(nw) for j in range(n)]
    states = [(1 << 32) + k for k in range(n_lvl * N * ways)]
    t = lambda a, dt: torch.tensor(a, dtype=dt)  # noqa: E731
    return Bitstream(N, [(6, 8, 8), (12, 4, 4)][:n_lvl], t(states, torch.int64),
                     t(nw, torch.int64), t(words, torch.int32),
                     meta={"n_subpixels": N * 3 * 16 * 16, "conv": "f32"},
                     host_nwords=t(nw, torch.int64), ways=ways)


def _safe(escaped, ways=1):
    """A SafeTiledBitstream over SIZES: raw byte j of escaped entry e is (7 * e + j) % 251."""
    from idfcodec.safe import SafeTiledBitstream
    escaped = np.asarray(escaped, dtype=bool)
    K = int((~escaped).sum())
    raw = [np.arange(RAW[e], dtype=np.int64) + 7 * e for e in range(6) if escaped[e]]
    raw = (np.concatenate(raw) % 251).astype(np.uint8) if raw else np.zeros(0, np.uint8)
    return SafeTiledBitstream(_hand_bitstream(K, ways=ways) if K else None, list(SIZES), C,
                              (16, 16), escaped, torch.from_numpy(raw))


MIXED = [True, False, True, False, False, True]


# ------------------------------------------------------------------ the container
def test_entry_rects_are_the_in_image_parts():
    from idfcodec.safe import entry_rects
    assert entry_rects(SIZES, 16, 16) == RECTS
    assert entry_rects([(37, 21)], 16, 16) == [(16, 16), (16, 5), (16, 16), (16, 5), (5, 16),
                                               (5, 5)]
    assert entry_rects([(25, 9), (12, 8)], 12, 8) == [(12, 8), (12, 1), (12, 8), (12, 1), (1, 8),
                                                      (1, 1), (12, 8)]


@pytest.mark.parametrize("escaped", [MIXED, [False] * 6, [True] * 6])
def test_idfs_round_trip_and_layout(escaped):
    from idfcodec.safe import SafeTiledBitstream
    sbs = _safe(escaped)
    K = 6 - sum(escaped)
    buf = sbs.to_bytes()
    inner = sbs.stream.to_bytes() if K else b""
    raw = sbs.raw.numpy().tobytes()
    bitmap = bytes([sum(1 << i for i, e in enumerate(escaped) if e)])   # 6 of its 8 bits used
    want = (struct.pack("<4sHHIIII", b"IDFS", 1, 0, 3, 3, 16, 16)
            + b"".join(struct.pack("<II", *s) for s in SIZES) + bitmap
            + struct.pack("<Q", len(raw)) + raw + struct.pack("<Q", len(inner)) + inner)
    assert buf == want
    assert len(raw) == sum(r for r, e in zip(RAW, escaped) if e)
    back = SafeTiledBitstream.from_bytes(buf)
    assert back.sizes == SIZES and back.C == 3 and back.tile_hw == (16, 16)
    assert back.escaped.tolist() == list(escaped) and back.n_kept == K
    assert back.reasons is None
    assert torch.equal(back.raw, sbs.raw)
    assert (back.stream is None) == (K == 0)
    assert back.to_bytes() == buf
    assert back.bits() == sbs.bits() == (sbs.stream.bits() if K else 0) + 8 * len(raw)
    nsub = 3 * (1 + 17 * 16 + 5 * 40)
    assert sbs.n_subpixels() == nsub and sbs.bpd() == sbs.bits() / nsub
    assert sbs.escaped_share() == len(raw) / nsub
    if K == 0:
        assert sbs.escaped_share() == 1.0 and sbs.bits() == 8 * nsub


@pytest.mark.parametrize("escaped,digest", [
    (MIXED, "cf947318d617b98b86656ccd124664646973948ac9410b3af42debf025a07abe"),
    ([False] * 6, "0f3679bc562f6b34bfa4a56a243c38ae1bc40403df38b5b2d9ac9611a0b82337"),
    ([True] * 6, "a625b0785bd3aa35dc0be09f4d66516e70e14a2d284f651cbb43cac619772036")])
def test_idfs_bytes_are_frozen(escaped, digest):
    """The digests of the hand-built containers, taken before TileLayout wrote their header."""
    import hashlib
    assert hashlib.sha256(_safe(escaped).to_bytes()).hexdigest() == digest


def test_idfs_bitmap_of_more_than_one_byte():
    """9 tiles: two bitmap bytes, the second holding one bit."""
    from idfcodec.safe import SafeTiledBitstream, entry_rects
    sizes = [(48, 48)]
    escaped = np.array([False] * 8 + [True])
    raw = torch.arange(768, dtype=torch.int64).remainder(256).to(torch.uint8)
    sbs = SafeTiledBitstream(_hand_bitstream(8), sizes, 3, (16, 16), escaped, raw)
    assert entry_rects(sizes, 16, 16) == [(16, 16)] * 9
    buf = sbs.to_bytes()
    assert buf[32:34] == b"\x00\x01"
    back = SafeTiledBitstream.from_bytes(buf)
    assert back.escaped.tolist() == escaped.tolist() and back.to_bytes() == buf
    with pytest.raises(ValueError, match="past"):
        SafeTiledBitstream.from_bytes(buf[:33] + b"\x03" + buf[34:])


def test_idfs_ways_follow_the_inner_stream():
    from idfcodec.safe import SafeTiledBitstream
    sbs = _safe(MIXED, ways=8)
    back = SafeTiledBitstream.from_bytes(sbs.to_bytes())
    assert back.stream.ways == 8 and back.stream.states.numel() == 2 * 3 * 8
    assert back.bits() == 64 * 48 + 32 * int(back.stream.nwords.sum()) + 8 * (3 + 48 + 120)


def _patched(raw, fmt, offset, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_idfs_errors():
    from idfcodec.safe import SafeTiledBitstream
    sbs = _safe(MIXED)
    buf = sbs.to_bytes()
    n_raw = 3 + 48 + 120
    o_map = 24 + 8 * len(SIZES)
    o_rawlen = o_map + 1
    o_raw = o_rawlen + 8
    o_len = o_raw + n_raw
    o_inner = o_len + 8
    assert struct.unpack_from("<Q", buf, o_rawlen)[0] == n_raw
    assert struct.unpack_from("<Q", buf, o_len)[0] == len(buf) - o_inner
    assert SafeTiledBitstream.from_bytes(buf).n_kept == 3
    cases = {
        "magic": _patched(buf, "<4s", 0, b"IDFT"),
        "version": _patched(buf, "<H", 4, 2),
        "flags": _patched(buf, "<H", 6, 1),
        "zero n_images": _patched(buf, "<I", 8, 0),
        "zero C": _patched(buf, "<I", 12, 0),
        "zero tile_h": _patched(buf, "<I", 16, 0),
        "zero tile_w": _patched(buf, "<I", 20, 0),
        "zero H": _patched(buf, "<I", 24 + 8, 0),
        "zero W": _patched(buf, "<I", 24 + 4, 0),
        "empty": b"",
        "truncated header": buf[:20],
        "truncated sizes": buf[:24 + 8],
        "truncated bitmap": buf[:o_map],
        "truncated raw length": buf[:o_rawlen + 4],
        "truncated raw bytes": buf[:o_raw + 10],
        "truncated inner length": buf[:o_len + 4],
        "no inner": buf[:o_inner],
        "truncated inner": buf[:-4],
        "trailing bytes": buf + b"\0\0\0\0",
        "inner length too small": _patched(buf, "<Q", o_len, len(buf) - o_inner - 4),
        "inner length too large": _patched(buf, "<Q", o_len, len(buf) - o_inner + 4),
        "inner cut short": buf[:o_len] + struct.pack("<Q", 10) + buf[o_inner:o_inner + 10],
        "inner magic": _patched(buf, "<4s", o_inner, b"IDFX"),
        "raw length too small": _patched(buf, "<Q", o_rawlen, n_raw - 1),
        "raw length too large": _patched(buf, "<Q", o_rawlen, n_raw + 1),
        "bitmap bit 6, past N": _patched(buf, "<B", o_map, buf[o_map] | 0x40),
        "bitmap bit 7, past N": _patched(buf, "<B", o_map, buf[o_map] | 0x80),
        # one more entry escaped: the raw length no longer fits (and K != the inner count)
        "bitmap and raw length disagree": _patched(buf, "<B", o_map, buf[o_map] | 0x02),
        "K = 0 with an inner stream": None,
    }
    all_raw = _safe([True] * 6).to_bytes()
    cases["K = 0 with an inner stream"] = (all_raw[:-8] + struct.pack("<Q", len(buf) - o_inner)
                                           + buf[o_inner:])
    for name, bad in cases.items():
        with pytest.raises(ValueError):
            SafeTiledBitstream.from_bytes(bad)
            pytest.fail(name)
    # K differs from the inner stream's entry count
    for K in (2, 4):
        sbs.stream = _hand_bitstream(K)
        with pytest.raises(ValueError, match="keeps"):
            sbs.to_bytes()
        inner = sbs.stream.to_bytes()
        with pytest.raises(ValueError, match="keeps 3 tiles"):
            SafeTiledBitstream.from_bytes(buf[:o_len] + struct.pack("<Q", len(inner)) + inner)
    # to_bytes refuses raw bytes that are not the escaped tiles'
    sbs = _safe(MIXED)
    sbs.raw = sbs.raw[:-1]
    with pytest.raises(ValueError, match="raw bytes"):
        sbs.to_bytes()


# ------------------------------------------------------------------ the keep rule
def _nwords_for(bits, n_lvl=2, ways=1):
    """Word counts, level-major, with entry e costing exactly bits[e] (all of it in level 0)."""
    fixed = n_lvl * (64 * ways + 32)
    assert all((b - fixed) % 32 == 0 and b >= fixed for b in bits)
    return [(b - fixed) // 32 for b in bits] + [0] * (len(bits) * (n_lvl - 1))


def test_entry_bits_counts_states_words_and_table_fields():
    from idfcodec.safe import entry_bits
    nw = [5, 0, 7, 1, 2, 3]          # levels 0, 1 of entries 0..2
    assert entry_bits(nw, 3).tolist() == [2 * 96 + 32 * 6, 2 * 96 + 32 * 2, 2 * 96 + 32 * 10]
    assert entry_bits(nw, 3, ways=8).tolist() == [2 * 544 + 32 * 6, 2 * 544 + 32 * 2,
                                                  2 * 544 + 32 * 10]


def test_keep_rule_size_ties_and_edge_tiles():
    from idfcodec.safe import REASON_SIZE, keep_rule
    raw_bits = [8 * r for r in RAW]          # 24, 6144, 384, 1920, 1920, 960
    ok = [0] * 12
    # every entry at exactly its raw size: all kept (the 1x1 entry cannot: two levels' states
    # and table fields alone are 192 bits > 24)
    nw = _nwords_for([192] + raw_bits[1:])
    got = keep_rule(nw, ok, RECTS, C, 1, 1.0)
    assert got.tolist() == [REASON_SIZE, 0, 0, 0, 0, 0]
    # one word more: escaped, each against its own in-image size and not the whole tile's
    for e in range(1, 6):
        bits = list(raw_bits)
        bits[0] = 192
        bits[e] += 32
        got = keep_rule(_nwords_for(bits), ok, RECTS, C, 1, 1.0)
        assert got.tolist() == [REASON_SIZE] + [REASON_SIZE if k == e else 0 for k in range(1, 6)]
    # the words spread over the levels count the same
    nw = _nwords_for(raw_bits[1:2] * 6)
    spread = [n - 3 for n in nw[:6]] + [3] * 6
    assert keep_rule(spread, ok, [(16, 16)] * 6, C, 1, 1.0).tolist() == [0] * 6
    spread[7] += 1
    assert keep_rule(spread, ok, [(16, 16)] * 6, C, 1, 1.0).tolist() == [0, 2, 0, 0, 0, 0]
    # a tie at another ratio: 0.5 * 6144 = 3072 keeps, 3104 does not; 2.0 keeps 12288
    full = [(16, 16)] * 3
    assert keep_rule(_nwords_for([3072, 3104, 192]), [0] * 6, full, C, 1, 0.5).tolist() == [0, 2, 0]
    assert keep_rule(_nwords_for([12288, 12320, 192]), [0] * 6, full, C, 1, 2.0).tolist() == \
        [0, 2, 0]
    # inf never escapes for size, not even the 1x1 entry
    assert keep_rule(_nwords_for([1 << 20] * 6), ok, RECTS, C, 1, math.inf).tolist() == [0] * 6
    # ways: 64 bits per state and way
    nw8 = _nwords_for([6144, 6144 + 32, 1088], ways=8)
    assert keep_rule(nw8, [0] * 6, full, C, 8, 1.0).tolist() == [0, 2, 0]
    assert keep_rule(nw8, [0] * 6, full, C, 1, 1.0).tolist() == [0, 0, 0]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            keep_rule(nw8, [0] * 6, full, C, 8, bad)


def test_keep_rule_status_flags():
    from idfcodec import _lib
    from idfcodec.safe import REASON_SIZE, REASON_STATUS, keep_rule
    full = [(16, 16)] * 4
    nw = _nwords_for([192] * 4)
    WL = _lib.STREAM_WORDS_LEFT
    assert WL == 32
    # WORDS_LEFT alone keeps, at either level
    assert keep_rule(nw, [WL, 0, 0, 0, 0, 0, WL, 0], full, C).tolist() == [0] * 4
    flags = (_lib.STREAM_SCALE_ZERO, _lib.STREAM_FREQ_ZERO, _lib.STREAM_NEG_CDF,
             _lib.STREAM_UNDERFLOW, _lib.STREAM_OUT_OF_WINDOW, 64, 1 << 30)
    for f in flags:
        for lvl in (0, 1):
            for e in range(4):
                st = [0] * 8
                st[lvl * 4 + e] = f
                want = [REASON_STATUS if k == e else 0 for k in range(4)]
                assert keep_rule(nw, st, full, C).tolist() == want, (f, lvl, e)
                st[lvl * 4 + e] |= WL        # beside WORDS_LEFT it escapes as well
                assert keep_rule(nw, st, full, C).tolist() == want
                assert keep_rule(nw, st, full, C, 1, math.inf).tolist() == want
    # both reasons at once
    big = _nwords_for([192, 6144 + 32, 192, 192])
    st = [0, 0, 0, 0, 0, 16, 0, 0]
    assert keep_rule(big, st, full, C).tolist() == [0, REASON_STATUS | REASON_SIZE, 0, 0]


# ------------------------------------------------------------------ the maps
def test_inner_index_and_raw_offsets():
    from idfcodec.safe import inner_index, raw_offsets
    assert inner_index(MIXED) == [-1, 0, -1, 1, 2, -1]
    assert raw_offsets(MIXED, RECTS, C) == ([0, -1, 3, -1, -1, 51], 171)
    assert inner_index([False] * 6) == list(range(6))
    assert raw_offsets([False] * 6, RECTS, C) == ([-1] * 6, 0)
    assert inner_index([True] * 6) == [-1] * 6
    assert raw_offsets([True] * 6, RECTS, C) == ([0, 3, 771, 819, 1059, 1299], 1419)
    assert 1419 == 3 * (1 + 17 * 16 + 5 * 40)     # all escaped: the source bytes, no more
    assert raw_offsets(MIXED, RECTS, 1) == ([0, -1, 1, -1, -1, 17], 57)
    assert inner_index([]) == [] and raw_offsets([], [], C) == ([], 0)


# ------------------------------------------------------------------ the size bound
def _bound_case(rng, sizes, th, tw, n_lvl, ways, max_ratio):
    """Random word counts around each entry's allowed size -> the file the keep rule builds."""
    from idfcodec.codec import Bitstream
    from idfcodec.safe import (SafeTiledBitstream, entry_rects, inner_index, keep_rule,
                               raw_offsets)
    rects = entry_rects(sizes, th, tw)
    N = len(rects)
    per_level = np.array([[int(max_ratio * C * h * w * 8) // 32 // n_lvl for h, w in rects]] * n_lvl)
    fixed = 2 * ways + 1     # words' worth of states and table field per level
    nw = np.maximum(per_level + rng.integers(-fixed - 3, 4, (n_lvl, N)), 0).reshape(-1)
    status = np.where(rng.random(n_lvl * N) < 0.1, 16, 0) | np.where(
        rng.random(n_lvl * N) < 0.3, 32, 0)
    reasons = keep_rule(nw, status, rects, C, ways, max_ratio)
    escaped = reasons != 0
    kept = [e for e in range(N) if not escaped[e]]
    K = len(kept)
    assert inner_index(escaped) == [kept.index(e) if e in kept else -1 for e in range(N)]
    inner = None
    if K:
        knw = nw.reshape(n_lvl, N)[:, kept].reshape(-1)
        inner = Bitstream(K, [(6, 8, 8), (12, 4, 4), (48, 2, 2)][:n_lvl],
                          torch.full((n_lvl * K * ways,), 1 << 32, dtype=torch.int64),
                          torch.from_numpy(knw.astype(np.int64)),
                          torch.zeros(int(knw.sum()), dtype=torch.int32),
                          meta={"n_subpixels": K * C * th * tw, "conv": "f32"}, ways=ways)
    _, n_raw = raw_offsets(escaped, rects, C)
    return SafeTiledBitstream(inner, list(sizes), C, (th, tw), escaped,
                              torch.zeros(n_raw, dtype=torch.uint8), reasons), K


@pytest.mark.parametrize("n_lvl,ways", [(1, 1), (2, 1), (3, 1), (2, 8)])
@pytest.mark.parametrize("max_ratio", [1.0, 0.5])
def test_size_bound_holds_for_any_word_counts(n_lvl, ways, max_ratio):
    """max_ratio <= 1: the file is at most the source plus its fixed headers, bits() at most the
    source's bits -- for any word counts and flags, because the rule counts every byte an entry
    adds."""
    from idfcodec.safe import SafeTiledBitstream, file_size_bound
    rng = np.random.default_rng(100 * n_lvl + ways)
    seen = set()
    for sizes, (th, tw) in (([(1, 1), (16, 16), (17, 16), (5, 40), (37, 21)], (16, 16)),
                            ([(64, 64)], (16, 16)), ([(25, 9), (12, 8)], (12, 8)),
                            ([(1, 1)], (16, 16))):
        for _ in range(6):
            sbs, K = _bound_case(rng, sizes, th, tw, n_lvl, ways, max_ratio)
            N = len(sbs.escaped)
            src = sum(C * H * W for H, W in sizes)
            buf = sbs.to_bytes()
            bound = src + 24 + 8 * len(sizes) + -(-N // 8) + 16 + (36 + 12 * n_lvl if K else 0)
            assert file_size_bound(sizes, C, th, tw, n_lvl, kept=bool(K)) == bound
            assert len(buf) <= bound, (sizes, K, N)
            assert sbs.bits() <= 8 * src
            assert sbs.bits() == (sbs.stream.bits() if K else 0) + 8 * sbs.raw.numel()
            assert SafeTiledBitstream.from_bytes(buf).to_bytes() == buf
            seen.add("none" if K == 0 else "all" if K == N else "some")
    assert "some" in seen and "none" in seen      # the 1x1 image alone is always escaped


def test_size_bound_is_reached_by_the_all_raw_file():
    from idfcodec.safe import file_size_bound
    sbs = _safe([True] * 6)
    assert len(sbs.to_bytes()) == file_size_bound(SIZES, C, 16, 16, 2, kept=False) \
        == 1419 + 24 + 24 + 1 + 16


def test_exports_and_cached_codec():
    import idfcodec
    from idfcodec import safe, synthetic, tiled
    from idfcodec.configs import _dense, _flows
    assert idfcodec.SafeTiledCodec is safe.SafeTiledCodec
    assert idfcodec.SafeTiledBitstream is safe.SafeTiledBitstream
    assert idfcodec.TiledCodec is tiled.TiledCodec
    assert issubclass(safe.SafeTiledCodec, tiled.TiledCodec)
    assert (safe.REASON_STATUS, safe.REASON_SIZE, safe.REASON_VERIFY) == (1, 2, 4)
    model = synthetic.build_model(_flows("IDFlows", 2, 1, 8, 8, 3, _dense(8, 1), _dense(8, 1), 2))
    sc = safe.SafeTiledCodec(model, max_batch=3, ways=8)
    assert sc.tile_hw == (8, 8) and sc.max_batch == 3 and sc.ways == 8
    with pytest.raises(ValueError):
        safe.SafeTiledCodec(model, max_batch=0)
    with pytest.raises(TypeError):
        safe.SafeTiledCodec(torch.nn.Identity())


def test_file_tool_picks_the_codec_by_magic():
    import importlib.util
    import os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from idfcodec.safe import SafeTiledBitstream
    from idfcodec.tiled import TiledBitstream
    sbs = _safe(MIXED)
    got, safe = tool.read_container(sbs.to_bytes(), None)
    assert safe and isinstance(got, SafeTiledBitstream) and got.to_bytes() == sbs.to_bytes()
    tbs = TiledBitstream(_hand_bitstream(6), list(SIZES), 3, (16, 16))
    got, safe = tool.read_container(tbs.to_bytes(), None)
    assert not safe and isinstance(got, TiledBitstream) and got.to_bytes() == tbs.to_bytes()
    with pytest.raises(ValueError):
        tool.read_container(b"IDFB" + bytes(40), None)
