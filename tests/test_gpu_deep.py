"""The 16-bit predictive coder on the device: DeepTiledCodec's files byte for byte against
tests/deep_ref.py (numpy and the C oracle) and the pinned digests, exact round trips, strided
sources and outputs, crops, a real-size tile, damaged units and the C calls' argument checks.

A file holds one channel count, so the images -- 13 x 11 (C = 1), 9 x 20 (C = 3) and 8 x 8
(C = 1) at tile 8 x 8 -- make two files: the grey pair and the 3-channel one."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import deep_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

L = 1 << 32
GUARD = 0xA5C3


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def to_np(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def hand():
    a, b, c = R.hand_images()
    return {"grey": ([a, c], R.write_file([a, c], 8, 8)), "rgb": ([b], R.write_file([b], 8, 8))}


def codec_for(images, tile=(8, 8)):
    from idfcodec import DeepTiledCodec
    return DeepTiledCodec(images[0].shape[0], tile=tile)


# ------------------------------------------------------------------ bytes and round trip
@pytest.mark.parametrize("name", ["grey", "rgb"])
def test_files_equal_the_reference_and_round_trip(hand, name):
    from idfcodec import DeepTiledBitstream, deep_section_bound
    images, want = hand[name]
    codec = codec_for(images)
    bs = codec.encode([to_dev(i) for i in images])
    buf = bs.to_bytes()
    assert buf == want
    with open(os.path.join(GOLDEN, "idfd_hand.sha256")) as f:
        pinned = {n: d for d, n in (line.split() for line in f)}
    assert hashlib.sha256(buf).hexdigest() == pinned[name]
    assert len(buf) <= deep_section_bound(bs.sizes, bs.C, (8, 8))
    outs, info = codec.decode(DeepTiledBitstream.from_bytes(buf, "cuda"))
    assert info["ok"] and info["damaged_planes"] == []
    for o, i in zip(outs, images):
        assert o.dtype == torch.uint16 and np.array_equal(to_np(o), i)
    cls = bs.classes
    assert (info["constant_planes"], info["packed_planes"], info["raw_planes"]) == tuple(
        int((cls == k).sum()) for k in (0, 1, 2))
    assert info["escapes"] == len(bs.escapes) == int(bs.nesc.sum())
    # a host source, and passes of a few units each, write the same file
    assert codec.encode([torch.from_numpy(i.view(np.int16)).view(torch.uint16)
                         for i in images]).to_bytes() == want
    from idfcodec import deep
    keep = deep.SYMBOLS_PER_PASS
    deep.SYMBOLS_PER_PASS = 100
    try:
        assert codec.encode([to_dev(i) for i in images]).to_bytes() == want
    finally:
        deep.SYMBOLS_PER_PASS = keep


def test_the_images_cover_what_they_are_meant_to(hand):
    """Every class, shifts 0, 3 (fields crossing a word boundary) and 8, an escape, units one
    sample wide and one sample high, partial tiles and a whole tile."""
    from idfcodec import DeepTiledBitstream
    classes, shifts, n_esc, rects = set(), set(), 0, set()
    for images, buf in hand.values():
        bs = DeepTiledBitstream.from_bytes(buf)
        classes |= set(bs.classes.tolist())
        ns = bs.unit_samples()[bs.packed]
        shifts |= set(bs.shift.tolist())
        assert any(s == 3 and n * 3 > 32 for s, n in zip(bs.shift, ns)) or 3 not in bs.shift
        n_esc += len(bs.escapes)
        rects |= set(bs.layout.rects)
    assert classes == {0, 1, 2} and {0, 3, 8} <= shifts and n_esc > 0
    assert (8, 8) in rects and any(h == 1 for h, w in rects) and any(w < 8 for h, w in rects)
    # a unit one sample wide: the 13 x 11 image at tile 8 x 8 has none, so one is coded here
    col = np.arange(13, dtype=np.uint16).reshape(1, 13, 1) * 3 + 7
    codec = codec_for([col])
    bs = codec.encode([to_dev(col)])
    assert bs.to_bytes() == R.write_file([col], 8, 8)
    assert np.array_equal(to_np(codec.decode(bs)[0][0]), col)


# ------------------------------------------------------------------ strides
def test_strided_sources_and_outputs(hand):
    (b,), want = hand["rgb"]
    C, H, W = b.shape
    codec = codec_for([b])
    hwc = to_dev(np.ascontiguousarray(b.transpose(1, 2, 0)))
    assert codec.encode([hwc], layout="hwc").to_bytes() == want
    pitched = torch.zeros((C, H, W + 5), dtype=torch.int16, device="cuda").view(torch.uint16)
    pitched[:, :, :W].view(torch.int16).copy_(to_dev(b).view(torch.int16))
    assert codec.encode([pitched[:, :, :W]], layout="chw").to_bytes() == want
    big = np.full((C, H + 4, W + 6), 31337, dtype=np.uint16)
    big[:, 2:2 + H, 3:3 + W] = b
    bs = codec.encode([to_dev(big)[:, 2:2 + H, 3:3 + W]], layout="chw")
    assert bs.to_bytes() == want
    with pytest.raises(ValueError, match="contiguous"):
        codec.encode([pitched[:, :, :W]])
    # out=: a window of a larger planar tensor, then interleaved with a pixel stride of 4
    host = np.full((C, H + 4, W + 6), GUARD, dtype=np.uint16)
    dst = to_dev(host)
    outs, info = codec.decode(bs, out=[dst[:, 2:2 + H, 3:3 + W]])
    assert info["ok"] and outs[0].data_ptr() == dst[:, 2:2 + H, 3:3 + W].data_ptr()
    got = to_np(dst)
    assert np.array_equal(got[:, 2:2 + H, 3:3 + W], b)
    got[:, 2:2 + H, 3:3 + W] = GUARD
    assert (got == GUARD).all()                         # nothing else was written
    dst = to_dev(np.full((H, W, 4), GUARD, dtype=np.uint16))
    outs, info = codec.decode(bs, layout="hwc", out=[dst[:, :, :C]])
    got = to_np(dst)
    assert info["ok"] and np.array_equal(got[:, :, :C].transpose(2, 0, 1), b)
    assert (got[:, :, C] == GUARD).all()
    outs, _ = codec.decode(bs, layout="hwc")
    assert tuple(outs[0].shape) == (H, W, C) and np.array_equal(to_np(outs[0]),
                                                               b.transpose(1, 2, 0))


# ------------------------------------------------------------------ crops and subsets
def test_crop_decodes_only_the_units_it_touches(hand):
    (a, c), want = hand["grey"]
    codec = codec_for([a])
    bs = codec.encode([to_dev(a), to_dev(c)])
    out, info = codec.decode_region(bs, 0, 2, 1, 5, 9)          # tiles (0, 0) and (0, 1) of four
    assert np.array_equal(to_np(out), a[:, 2:7, 1:10])
    assert info["ok"] and info["tiles"] == 2
    assert info["constant_planes"] + info["packed_planes"] + info["raw_planes"] == 2
    assert (info["constant_planes"], info["packed_planes"]) == (1, 1)
    out, info = codec.decode_region(bs, 0, 9, 9, 3, 2)          # the corner tile alone: raw
    assert np.array_equal(to_np(out), a[:, 9:12, 9:11])
    assert (info["tiles"], info["raw_planes"], info["escapes"]) == (1, 1, 0)
    outs, info = codec.decode(bs, images=[1])
    assert info["tiles"] == 1 and np.array_equal(to_np(outs[0]), c)


# ------------------------------------------------------------------ a real-size tile
def test_a_64x64_tile_of_a_noisy_ramp_packs_and_equals_the_reference():
    rng = np.random.default_rng(64)
    yy, xx = np.mgrid[0:64, 0:64]
    img = np.clip(np.rint(9000 + 40 * yy + 25 * xx + rng.normal(0, 30, (64, 64))), 0,
                  65535).astype(np.uint16)[None]
    codec = codec_for([img], tile=(64, 64))
    bs = codec.encode([to_dev(img)])
    buf = bs.to_bytes()
    assert bs.classes.tolist() == [1]
    assert buf == R.write_file([img], 64, 64)
    print(f"64x64 ramp, sigma 30: {len(buf)} bytes, {len(buf) / 8192:.3f} of raw, shift "
          f"{int(bs.shift[0])}, {int(bs.nesc[0])} escapes")
    assert len(buf) < 2 * 64 * 64
    outs, info = codec.decode(bs)
    assert info["ok"] and np.array_equal(to_np(outs[0]), img)


def test_escapes_keep_their_raster_order_across_waves_and_chunks():
    """A 64 x 64 unit is 16 chunks of 256 samples over 4 waves in the prep kernel; outliers in 3%
    of its samples put escapes in every chunk and most waves, and their order is the format."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:64, 0:64]
    img = 20000 + 30 * yy + 11 * xx + rng.normal(0, 3, (64, 64))
    hit = rng.random((64, 64)) < 0.03
    img[hit] = rng.integers(0, 65536, int(hit.sum()))
    img = np.clip(np.rint(img), 0, 65535).astype(np.uint16)[None]
    codec = codec_for([img], tile=(64, 64))
    bs = codec.encode([to_dev(img)])
    assert bs.classes.tolist() == [1] and int(bs.nesc[0]) >= 64
    esc_rows = np.flatnonzero(R.model(img[0])["esc_mask"].reshape(-1)) // 256
    assert len(set(esc_rows.tolist())) == 16                   # every chunk holds one
    assert np.array_equal(bs.escapes, R.model(img[0])["esc"])
    assert bs.to_bytes() == R.write_file([img], 64, 64)
    outs, info = codec.decode(bs)
    assert info["ok"] and info["escapes"] == int(bs.nesc[0])
    assert np.array_equal(to_np(outs[0]), img)


# ------------------------------------------------------------------ damage
def test_damaged_units_are_flagged_and_stay_inside_their_samples(hand):
    import copy
    (a, c), _ = hand["grey"]
    codec = codec_for([a])
    bs = codec.encode([to_dev(a), to_dev(c)])
    packed = np.flatnonzero(bs.packed)
    assert packed.tolist() == [0, 2, 4]
    off = np.concatenate([[0], np.cumsum(bs.nwords)])
    words = bs.words.cpu().numpy().copy()
    # unit 0 loses its last word; unit 4 has one bit of a middle word flipped; unit 2 is intact
    words[(off[2] + off[3]) // 2] ^= 1 << 9
    words = np.delete(words, off[1] - 1)
    bad = copy.copy(bs)
    bad.nwords = bs.nwords.copy()
    bad.nwords[0] -= 1
    bad.words = torch.from_numpy(words).cuda()
    shapes = [(1, 13, 11), (1, 8, 8)]
    dsts = [to_dev(np.full((s[0], s[1] + 2, s[2] + 2), GUARD, dtype=np.uint16)) for s in shapes]
    outs, info = codec.decode(bad, out=[d[:, 1:-1, 1:-1] for d in dsts])
    assert not info["ok"] and info["damaged_planes"] == [0, 4]
    got = [to_np(d) for d in dsts]
    for g in got:                                              # the guard frames are intact
        inner = g[:, 1:-1, 1:-1].copy()
        g[:, 1:-1, 1:-1] = GUARD
        assert (g == GUARD).all()
        g[:, 1:-1, 1:-1] = inner
    img0 = got[0][:, 1:-1, 1:-1]
    assert np.array_equal(img0[:, :8, 8:], a[:, :8, 8:])       # unit 1 (constant)
    assert np.array_equal(img0[:, 8:, :], a[:, 8:, :])         # units 2 (packed) and 3 (raw)
    status = info["status"].cpu().numpy()
    assert status[0] & R.UNDERFLOW
    # the same damage through the reference decoder gives the same samples, states and flags
    states = info["final_states"].cpu().numpy().view(np.uint64)
    nw = bad.nwords
    woff = np.concatenate([[0], np.cumsum(nw)])
    loff = np.concatenate([[0], np.cumsum([(n * s + 31) // 32 for n, s in
                                           zip(bs.unit_samples()[packed], bs.shift)])])
    eoff = np.concatenate([[0], np.cumsum(bs.nesc)])
    low = bs.low.cpu().numpy().view(np.uint32)
    units = [(0, a[0, :8, :8], img0[0, :8, :8]), (2, c[0], got[1][0, 1:-1, 1:-1])]
    for k, (u, src, dec) in zip((0, 2), units):
        want = R.decode(int(bs.shift[k]), int(bs.sel[k]), int(bs.states[k]),
                        words.view(np.uint32)[woff[k]:woff[k + 1]], low[loff[k]:loff[k + 1]],
                        bs.escapes[eoff[k]:eoff[k + 1]], 8, 8)
        unit = packed[k]
        assert (int(states[unit]), int(status[unit])) == (want[1], want[2])
        n_done = 64 if not want[2] & R.UNDERFLOW else None
        if n_done:
            assert np.array_equal(dec, want[0])


# ------------------------------------------------------------------ the C calls' arguments
def test_device_calls_refuse_bad_arguments_before_a_launch():
    from idfcodec import _lib
    lib = _lib.lib()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    row = (ctypes.c_int64 * 8)(t.data_ptr(), 4, 4, 0, 0, 0, 8, 2)
    s = _lib.stream_ptr(t.device)
    assert lib.idf_deep_prep_u16(s, 0, 8, 8, *([None] * 14)) == 0
    assert lib.idf_deep_prep_u16(s, -1, 8, 8, p, row, *([p] * 12)) == 1
    assert lib.idf_deep_prep_u16(s, 1, 8, 0, p, row, *([p] * 12)) == 1
    for hole in range(12):
        args = [p] * 12
        args[hole] = None
        assert lib.idf_deep_prep_u16(s, 1, 8, 8, p, row, *args) == 1
    assert lib.idf_deep_prep_u16(s, 1, 8, 8, None, row, *([p] * 12)) == 1
    for i, v in ((0, t.data_ptr() + 1), (6, 7), (7, 3), (7, -2)):
        bad = (ctypes.c_int64 * 8)(*row)
        bad[i] = v
        assert lib.idf_deep_prep_u16(s, 1, 8, 8, p, bad, *([p] * 12)) == 1
        assert lib.idf_tile_gather_raw_strided_u16(s, 1, 8, 8, p, bad, p, p) == 1
        assert lib.idf_tile_scatter_raw_strided_u16(s, 1, 8, 8, p, p, p, p, bad) == 1
    assert lib.idf_tile_gather_raw_strided_u16(s, -1, 8, 8, p, row, p, p) == 1
    assert lib.idf_tile_gather_raw_strided_u16(s, 1, 8, 8, p, row, p, None) == 1
    assert lib.idf_tile_scatter_raw_strided_u16(s, 1, 8, 8, None, p, p, p, row) == 1
    assert lib.idf_deep_decode_u16(s, 0, 8, 8, *([None] * 18)) == 0
    assert lib.idf_deep_decode_u16(s, -1, 8, 8, *([p] * 18)) == 1
    for hole in range(18):
        args = [p] * 18
        args[hole] = None
        assert lib.idf_deep_decode_u16(s, 1, 8, 8, *args) == 1
    assert lib.idf_deep_decode_u16(s, 1, 8, lib.idf_deep_tw_max() + 1, *([p] * 18)) \
        == _lib.IDF_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not t.any()                                          # nothing ran
