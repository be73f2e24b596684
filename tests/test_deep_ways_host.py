"""The 16-bit coder's interleaved states on the host: csrc/idf_deep.h's order and step rule
(idf_deep_prep_ways_host, idf_deep_decode_ways_host) against tests/deep_ways_ref.py, and the IDFD
container at N ways.  No GPU.  Everything is integer-exact or exact in f32: every comparison is
equality."""
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

import deep_ref as R
import deep_ways_ref as W
from conftest import GOLDEN

BIG = ((40, 40), (24, 70), (64, 64))


def units_of_shape(h, w):
    """the units a shape is tested with"""
    out = [("diagonals", W.ramp_unit(h, w, 3, True)), ("noisy", W.noisy_unit(h, w))]
    if (h, w) in ((24, 70), (9, 40)):
        out.append(("mixed", W.mixed_unit(h, w)))
    return out


@pytest.fixture(scope="module")
def coded(oracle):
    """{(N, shape, kind): (unit, model, states, words)} over WAYS x SHAPES, coded once"""
    return {(N, s, kind): (u, *W.encode(u, N))
            for N in W.WAYS for s in W.SHAPES for kind, u in units_of_shape(*s)}


def test_the_units_cover_what_they_are_chosen_for(coded):
    for N in W.WAYS:
        for s in BIG:                       # the ramp with the two anti-diagonals
            u, m, S, words = coded[N, s, "diagonals"]
            assert m["shift"] == 0 and len(m["esc"]) == 45 and len(words) > 128
            assert not np.array_equal(m["esc"], m["esc_raster"])
            assert sorted(m["esc"].tolist()) == sorted(m["esc_raster"].tolist())
            perm, step = W.perm_steps(*s, N)
            per_step = np.bincount(step[m["esc_mask"].reshape(-1)[perm]])
            assert 8 <= per_step.max() <= 12
            assert W.unit_class(u, N)[0] == R.PACKED
        assert coded[N, (9, 40), "noisy"][1]["shift"] == 3
        u, m, S, words = coded[N, (24, 70), "mixed"]        # escapes and low bits in one unit
        assert m["shift"] == 2 and len(m["esc"]) == 39 and W.unit_class(u, N)[0] == R.PACKED
    # the geometry: win < N, win > N, hin < N, a partial last band, bands sharing a step
    assert any(w < 8 for _, w in W.SHAPES) and any(w > 64 for _, w in W.SHAPES)
    assert any(h < 8 for h, _ in W.SHAPES) and any(h % 8 for h, _ in W.SHAPES)
    t, _ = W.pw.steps_slots(1, 24, 70, 8)
    assert len({int(y) // 8 for y, x in zip(*np.nonzero(t == 70))}) == 2    # two bands, one step
    assert len({int(y) // 8 for y in range(24)}) == 3


@pytest.mark.parametrize("N", W.WAYS)
def test_prep_host_equals_the_reference_field_for_field(coded, N):
    from idfcodec import deep
    for (n_, s, kind), (u, m, S, words) in coded.items():
        if n_ != N:
            continue
        got = deep.host_prep(u, N)
        assert got["shift"] == m["shift"] and got["sel"] == m["sel"], (s, kind)
        assert (got["min"], got["max"]) == (m["min"], m["max"])
        assert np.array_equal(got["esc"], m["esc"]), (s, kind)     # wavefront order
        assert np.array_equal(got["low"], m["low"]), (s, kind)     # where they always were
        assert np.array_equal(got["low"], deep.host_prep(u)["low"])
        for k in ("x", "mean", "scale"):
            assert np.array_equal(got[k].view(np.uint32), m[k].view(np.uint32)), (s, kind, k)


@pytest.mark.parametrize("N", W.WAYS)
def test_decode_host_equals_the_reference(coded, N):
    from idfcodec import deep
    for (n_, (h, w), kind), (u, m, S, words) in coded.items():
        if n_ != N:
            continue
        args = (m["shift"], m["sel"], S, words, m["low"], m["esc"])
        out, final, status = deep.host_decode_ways(h, w, N, *args)
        assert status == 0 and (final == R.L).all(), ((h, w), kind)
        assert np.array_equal(out, u), ((h, w), kind)
        if (h, w) != (64, 64) or N in (8, 64):                  # the reference decoder is Python
            want = W.decode(*args, h, w, N)
            assert np.array_equal(want[0], u) and want[1] == [R.L] * N and want[2] == 0


@pytest.mark.parametrize("N", W.WAYS)
def test_damaged_units_follow_the_step_rule(coded, N):
    from idfcodec import deep
    seen, names = 0, set()
    for shape, kind in (((40, 40), "diagonals"), ((24, 70), "mixed"), ((9, 40), "noisy"),
                        ((19, 9), "noisy"), ((33, 5), "noisy")):
        u, m, S, words = coded[N, shape, kind]
        for name, d in W.damaged(m, S, words):
            args = (d["shift"], d["sel"], d["states"], d["words"], d["low"], d["esc"])
            want = W.decode(*args, *shape, N)
            got = deep.host_decode_ways(*shape, N, *args)
            assert got[2] == want[2] and got[1].tolist() == want[1], (shape, name)
            assert np.array_equal(got[0], want[0]), (shape, name)
            assert want[2] != 0 or want[1] != [R.L] * N, (shape, name)
            if name == "escape removed":    # the step that lacks an escape keeps nothing
                assert want[2] == R.UNDERFLOW | R.WORDS_LEFT and (want[0] == 0).any()
            seen |= want[2]
            names.add(name)
    assert len(names) == 5
    assert seen == R.UNDERFLOW | R.OUT_OF_WINDOW | R.WORDS_LEFT


# ------------------------------------------------------------------ the container
def bitstream_of(images, th, tw, N):
    """The DeepTiledBitstream of a list of uint16 [C, H, W] images, its fields from the
    references (deep_ref at N = 1)."""
    from idfcodec import deep
    units = R.units_of(images, th, tw)
    coded = [R.unit_class(u) if N == 1 else W.unit_class(u, N) for u in units]
    cls = np.array([c[0] for c in coded])
    pk = [c for c in coded if c[0] == R.PACKED]
    cat = lambda parts, dt: np.concatenate([np.asarray(p, dtype=dt) for p in parts]
                                           or [np.zeros(0, dt)])  # noqa: E731
    raw = cat([u.reshape(-1) for u, k in zip(units, cls) if k == R.RAW], "<u2")
    states = np.array([c[2] for c in pk], dtype=np.uint64).reshape((-1, N) if N > 1 else -1)
    return deep.DeepTiledBitstream(
        [i.shape[1:] for i in images], images[0].shape[0], (th, tw), cls == R.CONSTANT,
        cls == R.PACKED,
        np.array([u.flat[0] for u, k in zip(units, cls) if k == R.CONSTANT], dtype=np.uint16),
        torch.from_numpy(raw.view(np.uint8).copy()),
        np.array([c[1]["shift"] for c in pk], dtype=np.uint8),
        np.array([c[1]["sel"] for c in pk], dtype=np.uint32), states,
        np.array([len(c[3]) for c in pk], dtype=np.int64),
        np.array([len(c[1]["esc"]) for c in pk], dtype=np.int64),
        torch.from_numpy(cat([c[3] for c in pk], np.uint32).view(np.int32).copy()),
        torch.from_numpy(cat([c[1]["low"] for c in pk], np.uint32).view(np.int32).copy()),
        cat([c[1]["esc"] for c in pk], np.uint16), ways=N)


def ways_images():
    """Two grey images for tile 16 x 16: 20 x 37 -- a smooth ramp with one escape, a constant
    tile, a tile of uniform noise and narrow tiles at the edges -- and 16 x 16 with noise of
    ~6 bits (low bits)."""
    rng = np.random.default_rng(816)
    yy, xx = np.mgrid[0:20, 0:37]
    a = 20000 + 30 * yy - 11 * xx + rng.integers(-3, 4, (20, 37))
    a[0:16, 16:32] = 4242
    a[3, 4] = 64000
    a[16:20, 0:16] = rng.integers(0, 65536, (4, 16))
    b = W.noisy_unit(16, 16)
    return [a.astype(np.uint16)[None], b[None]]


@pytest.mark.parametrize("N", (8, 64))
def test_container_round_trip(oracle, N):
    from idfcodec import DeepTiledBitstream, deep_section_bound
    images = [W.ramp_unit(40, 40, 3, True)[None], W.mixed_unit(24, 70)[None]]
    want = W.write_file(images, 64, 128, N)
    bs = bitstream_of(images, 64, 128, N)
    assert bs.ways == N and bs.states.shape == (2, N)
    assert bs.to_bytes() == want                        # the codec's writer, the reference's file
    assert struct.unpack_from("<H", want, 6)[0] == N
    back = DeepTiledBitstream.from_bytes(want)
    assert back.ways == N and back.states.shape == (2, N) and back.to_bytes() == want
    assert np.array_equal(back.escapes, bs.escapes)
    assert len(want) <= deep_section_bound(back.sizes, 1, (64, 128))
    assert 8 * len(want) > back.bits() == bs.bits()
    n_sect = 8 * (4 + (-2) % 4 + (-len(bs.escapes) * 2) % 4)    # the count and the two pads
    assert back.bits() + n_sect == 8 * (len(want) - 24 - 16 - 1 - 1 - 8 - 8)


def test_flags_and_states_that_do_not_fit_are_refused(oracle):
    from idfcodec import DeepTiledBitstream as B
    images = [W.ramp_unit(40, 40, 3, True)[None]]
    buf = W.write_file(images, 64, 64, 8)
    for flags in (7, 1, 4, 128, 0x8008):
        with pytest.raises(ValueError, match="flags"):
            B.from_bytes(buf[:6] + struct.pack("<H", flags) + buf[8:])
    for flags in (0, 16):                                   # another N: the tables do not fit
        with pytest.raises(ValueError):
            B.from_bytes(buf[:6] + struct.pack("<H", flags) + buf[8:])
    for n in range(len(buf)):
        if n % 7 == 0 or n > len(buf) - 16:
            with pytest.raises(ValueError):
                B.from_bytes(buf[:n])
    bs = bitstream_of(images, 64, 64, 8)
    bs.check()
    for states in (bs.states[:, :7], bs.states.reshape(-1), bs.states[:0],
                   np.concatenate([bs.states, bs.states])):
        bad = bitstream_of(images, 64, 64, 8)
        bad.states = states
        with pytest.raises(ValueError, match="states"):
            bad.to_bytes()
    bad = bitstream_of(images, 64, 64, 8)
    bad.ways = 4
    with pytest.raises(ValueError, match="ways"):
        bad.check()


def test_one_way_writes_the_bytes_it_always_wrote(oracle):
    """ways=1 is the default of every layer: deep_ref's files of the hand-made images, whose
    digests tests/golden/idfd_hand.sha256 pins."""
    from idfcodec import DeepTiledBitstream, deep
    with open(os.path.join(GOLDEN, "idfd_hand.sha256")) as f:
        pinned = {name: digest for digest, name in (line.split() for line in f)}
    a, b, c = R.hand_images()
    for name, images in (("grey", [a, c]), ("rgb", [b])):
        want = R.write_file(images, 8, 8)
        assert hashlib.sha256(want).hexdigest() == pinned[name]
        bs = bitstream_of(images, 8, 8, 1)
        assert bs.ways == 1 and bs.to_bytes() == want
        assert struct.unpack_from("<H", want, 6)[0] == 0
        back = DeepTiledBitstream.from_bytes(want)
        assert back.ways == 1 and back.states.ndim == 1 and back.to_bytes() == want
    assert deep.unit_overhead() == deep.UNIT_BYTES == 21 and deep.unit_overhead(8) == 77
    assert int(deep.packed_bytes(54, 0, 21, 1)) == 107
    assert int(deep.packed_bytes(54, 0, 21, 1, 8)) == 107 + 56
    assert deep.unit_class([1], [2], [64], [0], [12], [0], 8)[0] == deep.CLASS_PACKED   # 125
    assert deep.unit_class([1], [2], [64], [0], [13], [0], 8)[0] == deep.CLASS_RAW      # 129
    assert deep.unit_class([1], [2], [64], [0], [13], [0])[0] == deep.CLASS_PACKED


def test_the_reference_file_at_8_ways_is_pinned(oracle):
    from idfcodec import DeepTiledBitstream, deep, deep_section_bound
    images = ways_images()
    buf = W.write_file(images, 16, 16, 8)
    with open(os.path.join(GOLDEN, "idfd_ways_hand.sha256")) as f:
        want = {name: digest for digest, name in (line.split() for line in f)}
    assert hashlib.sha256(buf).hexdigest() == want["grey8"]
    bs = DeepTiledBitstream.from_bytes(buf)
    assert set(bs.classes.tolist()) == {deep.CLASS_CONSTANT, deep.CLASS_PACKED, deep.CLASS_RAW}
    assert bs.ways == 8 and len(bs.escapes) >= 1 and (bs.shift > 0).any() and (bs.shift == 0).any()
    assert bitstream_of(images, 16, 16, 8).to_bytes() == buf
    sizes = [i.shape[1:] for i in images]
    n_packed = {}
    for N in (1,) + W.WAYS:                                 # the bound holds at every N
        f = R.write_file(images, 16, 16) if N == 1 else W.write_file(images, 16, 16, N)
        assert len(f) <= deep_section_bound(sizes, 1, (16, 16)), N
        n_packed[N] = int(DeepTiledBitstream.from_bytes(f).packed.sum())
    assert n_packed[1] > n_packed[8] >= n_packed[64] == 0   # small units fall to raw as N grows


# ------------------------------------------------------------------ the interface
def test_ways_supported_follows_the_lds_cap():
    from idfcodec import _lib, deep
    for N in W.WAYS:
        assert deep.ways_supported(64, 64, N) and deep.ways_supported(128, 128, N)
        assert deep.ways_supported(8, 3800, N)              # 60 800 bytes of 61 440
        assert not deep.ways_supported(8, 3840, N)          # the tables no longer fit beside it
        assert not deep.ways_supported(256, 128, N) and not deep.ways_supported(1, 1 << 20, N)
    L = _lib.lib()
    for bad in (1, 4, 7, 0, -8, 128):
        assert L.idf_deep_ways_supported(64, 64, bad) == 1
    assert L.idf_deep_ways_supported(0, 64, 8) == 1


def test_constructor_refuses_what_the_decoder_cannot_take():
    from idfcodec import DeepTiledCodec
    for bad in (4, 0, 2, 128, True, 8.0, "8"):
        with pytest.raises(ValueError, match="ways"):
            DeepTiledCodec(1, ways=bad)
    with pytest.raises(ValueError, match="LDS"):
        DeepTiledCodec(1, tile=(256, 128), ways=8)
    assert DeepTiledCodec(1, tile=(256, 128)).ways == 1     # one way keeps a row, not the unit
    codec = DeepTiledCodec(2, tile=(128, 128), ways=64)
    assert (codec.C, codec.tile_hw, codec.ways) == (2, (128, 128), 64)
    # a file whose N the tile does not support is refused by any codec of its C and tile
    big = bitstream_of([np.full((1, 4, 4), 7, dtype=np.uint16)], 256, 128, 1)
    big.ways = 8
    big.states = np.zeros((0, 8), dtype=np.uint64)
    big.check()
    with pytest.raises(ValueError, match="LDS"):
        DeepTiledCodec(1, tile=(256, 128)).check_bitstream(big)


def test_the_calls_check_their_arguments():
    import ctypes
    from idfcodec import _lib
    L = _lib.lib()
    z = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(z, ctypes.c_void_p)
    assert L.idf_deep_prep_ways_host(z, 2, 2, 4, *([z] * 9)) == 1
    assert L.idf_deep_prep_ways_host(None, 2, 2, 8, *([z] * 9)) == 1
    assert L.idf_deep_prep_ways_host(z, 2, 0, 8, *([z] * 9)) == 1
    assert L.idf_deep_decode_ways_host(2, 2, 1, 0, 0, z, None, 0, None, None, 0, z, z, z) == 1
    assert L.idf_deep_decode_ways_host(2, 2, 8, 0, 0, None, None, 0, None, None, 0, z, z, z) == 1
    assert L.idf_deep_decode_ways_host(2, 2, 8, 0, 0, z, None, 1, None, None, 0, z, z, z) == 1
    row = (ctypes.c_int64 * 8)(2, 4, 4, 0, 0, 0, 8, 2)
    assert L.idf_deep_prep_ways_u16(None, 0, 8, 8, *([None] * 14), 8) == 0
    assert L.idf_deep_prep_ways_u16(None, 0, 8, 8, *([None] * 14), 4) == 1
    assert L.idf_deep_prep_ways_u16(None, -1, 8, 8, p, row, *([p] * 12), 8) == 1
    assert L.idf_deep_prep_ways_u16(None, 1, 8, 8, p, row, *([p] * 11), None, 8) == 1
    bad = (ctypes.c_int64 * 8)(*row)
    bad[0] = 3
    assert L.idf_deep_prep_ways_u16(None, 1, 8, 8, p, bad, *([p] * 12), 8) == 1
    assert L.idf_deep_decode_ways_u16(None, 0, 8, 8, 8, *([None] * 18)) == 0
    assert L.idf_deep_decode_ways_u16(None, 0, 1, 8, 8, *([None] * 18)) == 1
    assert L.idf_deep_decode_ways_u16(None, 1, 8, 8, 8, *([p] * 17), None) == 1
    assert L.idf_deep_decode_ways_u16(None, 1, 8, 256, 128, *([p] * 18)) == _lib.IDF_ERR_UNSUPPORTED
