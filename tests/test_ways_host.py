"""N-way interleaved rANS streams on the CPU: the format's serial restatement
(tests/rans_ways_ref.py) pinned to the C oracle, the Bitstream container with ways, and the
refusals of the paths that code ways = 1 only."""
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rans_ways_ref as R

WAYS = (8, 16, 32, 64)
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 129, 700)
SHAPES = [(6, 4, 4), (12, 2, 2)]


# ------------------------------------------------------------------ the format
@pytest.mark.parametrize("ways", WAYS)
def test_restatement_pinned_to_c_oracle(oracle, ways):
    """Way j of an N-way stream is the C oracle's encode of x[j::N]: same final state, same
    number of words; the serial decoder returns x, ends with every state at L and has read
    every word."""
    g = np.random.default_rng(100 + ways)
    most_pushed = 0
    for n in LENGTHS:
        x, mean, scale = R.inputs(g, n)
        S, words, pushed = R.encode(x, mean, scale, ways)
        assert len(S) == ways and sum(pushed) == words.size <= n
        for j in range(ways):
            st, w = oracle.encode(1 << 32, x[j::ways], mean[j::ways], scale[j::ways])
            assert S[j] == st and pushed[j] == w.size, (n, j)
        S2, out, left = R.decode(S, words, n, mean, scale, ways)
        assert np.array_equal(out, x) and left == 0 and S2 == [1 << 32] * ways, n
        if ways == 64 and n == 700:  # one step's pushes: the prefix count is no corner case
            start, freq = oracle.cdf_freq(x, mean, scale)
            St = [1 << 32] * ways
            for t in range(0, n, ways):
                cnt = 0
                for i in range(t, min(t + ways, n)):
                    j, f = i % ways, int(freq[i])
                    if St[j] >= f << 40:
                        cnt += 1
                        St[j] >>= 32
                    St[j] = ((St[j] // f) << 24) + St[j] % f + int(start[i])
                most_pushed = max(most_pushed, cnt)
            assert St == S
    if ways == 64:
        assert most_pushed >= 2


def test_c_round_is_half_away_from_zero():
    assert [R.c_round(v) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999, -1023.5)] == [
        1.0, 2.0, 3.0, -1.0, -3.0, 2.0, -1024.0]


# ------------------------------------------------------------------ Bitstream
def _bs(ways=1, n_img=2, n_states=None, seed=0, conv="dx3"):
    from idfcodec.codec import Bitstream
    g = torch.Generator().manual_seed(seed)
    ns = len(SHAPES) * n_img
    nw = torch.randint(0, 9, (ns,), generator=g).to(torch.int64)
    n_states = ns * ways if n_states is None else n_states
    st = torch.randint(-(2 ** 62), 2 ** 62, (n_states,), generator=g, dtype=torch.int64)
    w = torch.randint(-(2 ** 31), 2 ** 31 - 1, (int(nw.sum()),), generator=g, dtype=torch.int32)
    return Bitstream(n_img, list(SHAPES), st, nw, w, meta={"n_subpixels": 96 * n_img, "conv": conv},
                     ways=ways)


@pytest.mark.parametrize("ways", [8, 64])
def test_container_roundtrip_with_ways(ways):
    from idfcodec.codec import Bitstream
    b = _bs(ways)
    raw = b.to_bytes()
    magic, ver, flags, n_img, n_lvl, n_str = struct.unpack_from("<4sHHIII", raw, 0)
    assert (magic, ver, n_img, n_lvl) == (b"IDFB", 2, 2, 2)
    assert n_str == 4 == b.n_streams           # the header counts streams, not states
    assert flags >> 4 == {8: 3, 64: 6}[ways] and flags & 0xF == 7
    r = Bitstream.from_bytes(raw)
    assert r.ways == ways and r.n_streams == 4 and r.states.numel() == 4 * ways
    assert torch.equal(r.states, b.states) and torch.equal(r.nwords, b.nwords)
    assert torch.equal(r.words, b.words) and r.meta["conv"] == "dx3"
    assert r.to_bytes() == raw
    assert len(raw) == 20 + 24 + 8 + 8 * 4 * ways + 4 * 4 + 4 * b.total_words()


def test_one_way_container_is_byte_identical_to_the_earlier_layout():
    """ways = 1 writes what the code before the ways field wrote: the header packed by hand
    from the same tensors, flags = the conv code alone."""
    b = _bs(1)
    hdr = struct.pack("<4sHHIII", b"IDFB", 2, 7, 2, 2, 4)
    want = (hdr + b"".join(struct.pack("<III", *s) for s in SHAPES) + struct.pack("<Q", 192)
            + b.states.numpy().astype("<i8").tobytes() + b.nwords.numpy().astype("<u4").tobytes()
            + b.words.numpy().astype("<i4").tobytes())
    assert b.to_bytes() == want


@pytest.mark.parametrize("code", [1, 2] + list(range(7, 16)))
def test_unknown_ways_codes_are_refused(code):
    from idfcodec.codec import Bitstream
    raw = bytearray(_bs(8).to_bytes())
    struct.pack_into("<H", raw, 6, 7 | code << 4)
    with pytest.raises(ValueError, match="unknown bitstream flags"):
        Bitstream.from_bytes(bytes(raw))


def test_flags_above_the_ways_field_are_refused():
    from idfcodec.codec import Bitstream
    raw = bytearray(_bs(8).to_bytes())
    struct.pack_into("<H", raw, 6, 7 | 3 << 4 | 1 << 8)
    with pytest.raises(ValueError, match="unknown bitstream flags"):
        Bitstream.from_bytes(bytes(raw))


def test_bits_streams_and_select_with_ways():
    b = _bs(8, n_img=3)
    assert b.n_streams == 6 and b.states.numel() == 48
    assert b.bits() == 64 * 48 + 32 * b.total_words()
    assert _bs(1, n_img=3).bits() == 64 * 6 + 32 * _bs(1, n_img=3).total_words()
    s = b.select([2, 0])
    assert s.ways == 8 and s.n_images == 2 and s.n_streams == 4
    rows = b.states.view(6, 8)
    assert torch.equal(s.states.view(4, 8), rows[[2, 0, 5, 3]])  # whole rows of ways
    assert s.nwords.tolist() == b.nwords[[2, 0, 5, 3]].tolist()
    off = b.word_offsets().tolist()
    want = torch.cat([b.words[off[k]:off[k] + int(b.nwords[k])] for k in (2, 0, 5, 3)])
    assert torch.equal(s.words, want)
    with pytest.raises(ValueError, match="ways"):
        _bs(1).__class__(2, list(SHAPES), torch.zeros(12, dtype=torch.int64),
                         torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                         meta={"conv": "dx3"}, ways=3).to_bytes()


def _codec():
    from idfcodec.codec import ImageCodec
    c = ImageCodec.__new__(ImageCodec)
    c.engine = SimpleNamespace(levels=[SimpleNamespace(z=z, h=h, w=w) for z, h, w in SHAPES],
                               conv_family="dx3", can_run=lambda conv: True)
    return c


def test_check_bitstream_with_ways():
    c = _codec()
    c.check_bitstream(_bs(1))
    c.check_bitstream(_bs(8))
    c.check_bitstream(_bs(64))
    with pytest.raises(ValueError, match="states"):   # a wrong state count
        c.check_bitstream(_bs(8, n_states=4))
    with pytest.raises(ValueError, match="states"):
        c.check_bitstream(_bs(8, n_states=33))
    with pytest.raises(ValueError, match="ways"):
        b = _bs(8)
        b.ways = 4
        c.check_bitstream(b)
    with pytest.raises(ValueError, match="ways"):
        b = _bs(8)
        b.ways = 0
        c.check_bitstream(b)


def test_encode_refuses_unknown_ways():
    from idfcodec.codec import check_ways
    assert [check_ways(w) for w in (1, 8, 16, 32, 64)] == [1, 8, 16, 32, 64]
    for w in (0, 2, 4, 12, 128, -8, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="ways"):
            check_ways(w)
    with pytest.raises(ValueError, match="ways"):
        _codec()._encode_guarded(lambda: None, 2, None, True, ways=4)


def test_interleave_levels_moves_rows_of_ways():
    from idfcodec import dist
    a, b = _bs(8, n_img=2, seed=1), _bs(8, n_img=1, seed=2)
    st, nw, w = dist.interleave_levels(torch.cat([a.states, b.states]),
                                       torch.cat([a.nwords, b.nwords]),
                                       torch.cat([a.words, b.words]), 2, 2, [2, 1], ways=8)
    ra, rb = a.states.view(4, 8), b.states.view(2, 8)
    assert torch.equal(st.view(6, 8), torch.stack([ra[0], ra[1], rb[0], ra[2], ra[3], rb[1]]))
    assert nw.tolist() == [int(v) for v in (a.nwords[0], a.nwords[1], b.nwords[0], a.nwords[2],
                                            a.nwords[3], b.nwords[1])]
    with pytest.raises(ValueError, match="ways"):
        dist.interleave_levels(torch.cat([a.states, b.states]), torch.cat([a.nwords, b.nwords]),
                               torch.cat([a.words, b.words]), 2, 2, [2, 1], ways=16)


def test_tiled_container_carries_ways():
    from idfcodec.tiled import TiledBitstream
    t = TiledBitstream(_bs(8), [(4, 8)], 3, (4, 4))
    assert t.state_bits_per_subpixel() == 64 * 32 / (3 * 4 * 8)
    r = TiledBitstream.from_bytes(t.to_bytes())   # the inner IDFB records ways
    assert r.stream.ways == 8 and torch.equal(r.stream.states, t.stream.states)


# ------------------------------------------------------------------ refusals
def test_twolevel_codec_refuses_ways():
    from idfcodec.twolevel import TwoLevelBitstream, TwoLevelCodec
    c = TwoLevelCodec.__new__(TwoLevelCodec)
    for rough, fine in ((_bs(8), _bs(1)), (_bs(1), _bs(8))):
        t = TwoLevelBitstream(rough, fine, 2, (3, 15, 13), (1, 3), (8, 8), (8, 8))
        with pytest.raises(ValueError, match="ways"):
            c.check_bitstream(t)
        with pytest.raises(ValueError, match="ways"):
            c.decode(t)


def test_residual_codec_refuses_ways():
    from idfcodec.residual import ResidualBitstream, ResidualCodec
    c = ResidualCodec.__new__(ResidualCodec)
    r = ResidualBitstream(_bs(8), torch.zeros(1, dtype=torch.int32), 2, (3, 8, 8), (2, 2), 16)
    with pytest.raises(ValueError, match="ways"):
        c.decode(r)


def test_dist_exchanges_refuse_ways():
    """The check comes before any collective: no process group is needed."""
    from idfcodec import dist
    b = _bs(8)
    with pytest.raises(ValueError, match="ways"):
        dist.gather_bitstream(b)
    with pytest.raises(ValueError, match="ways"):
        dist.scatter_bitstream(b)
    with pytest.raises(ValueError, match="ways"):
        dist.agree_shards(b)
    with pytest.raises(ValueError, match="ways"):
        dist.shard_streams(b.states, b.nwords, b.words, 2, 2, 0, 1)
