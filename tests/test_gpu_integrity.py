"""Sealed tiled files on the device: the three CRC-32 kernels against zlib.crc32 (every
comparison exact), SealedCodec round trips over the plain and the escaping tiled codec, one
damaged raw tile and one damaged coded tile named by their entry, and the model's fingerprint.
Tiny models only."""
import math
import zlib

import numpy as np
import pytest
import torch

import crc_ref

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (16, 16), (17, 16), (5, 40), (37, 21))
TILES = [(16, 16), (12, 8), (40, 33)]
# the kernel cases add a sixth image with a whole 40x33 tile: 5280 bytes at C = 4, two chunks of
# 4096, the second partly filled
KERNEL_SIZES = SIZES + ((45, 70),)
SENTINEL = 0x5A5A5A5A


def _tiny_model(*args):
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", *args[:5], _dense(24, 3), _dense(16, 2),
                                        args[5]))


@pytest.fixture(scope="module")
def model16():
    return _tiny_model(2, 2, 16, 16, 3, 2).cuda()


@pytest.fixture(scope="module")
def ragged():
    """1x1, 16x16, 17x16, 5x40, 37x21: 1 + 1 + 2 + 3 + 6 tiles of 16x16"""
    from idfcodec import synthetic
    return [synthetic.images(1, 3, H, W, seed=70 + i)[0].cuda() for i, (H, W) in enumerate(SIZES)]


@pytest.fixture(scope="module")
def ragged_crcs(ragged):
    return crc_ref.tile_crcs([t.cpu().numpy() for t in ragged], 16, 16)


def _dev(a, dt):
    return torch.tensor(a, dtype=dt, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def _guarded_out(n, pad=8):
    """int32 [n] inside `pad` sentinel words on either side: (whole, the view)."""
    whole = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[pad:pad + n]


def _sentinels_intact(whole, n, pad=8):
    w = whole.cpu().numpy()
    return bool((w[:pad] == SENTINEL).all() and (w[pad + n:] == SENTINEL).all())


# ------------------------------------------------------------------ 1. byte runs
SEG_LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
               65535, 65536, 65537, (1 << 20) + 3]


def test_segments_equal_zlib_at_every_length_and_offset():
    from idfcodec.integrity import device_crc32_segments
    rng = np.random.default_rng(5)
    # segment j starts at byte offset j % 8 past an 8-aligned position, one after the other
    starts, o = [], 0
    for j, n in enumerate(SEG_LENGTHS):
        o = (o + 7) // 8 * 8 + j % 8
        starts.append(o)
        o += n
    assert {s % 8 for s in starts} == set(range(8))
    host = rng.integers(0, 256, o + 8, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    order = list(reversed(range(len(SEG_LENGTHS))))
    rows = [(buf.data_ptr() + starts[j], SEG_LENGTHS[j]) for j in order]
    n = len(rows)
    whole, out = _guarded_out(n)
    device_crc32_segments(_dev(rows, torch.int64), n, out)
    raw = host.tobytes()
    assert _u32(out) == [zlib.crc32(raw[starts[j]:starts[j] + SEG_LENGTHS[j]]) for j in order]
    assert _sentinels_intact(whole, n)
    assert np.array_equal(buf.cpu().numpy(), host)
    # the outputs are overwritten, not accumulated: again into the same words, and a subset
    device_crc32_segments(_dev(rows, torch.int64), n, out)
    device_crc32_segments(_dev(rows[3:], torch.int64), 2, out[1:])
    want = [zlib.crc32(raw[starts[j]:starts[j] + SEG_LENGTHS[j]]) for j in order]
    want[1:3] = want[3:5]
    assert _u32(out) == want and _sentinels_intact(whole, n)


def test_crc_launchers_check_their_arguments():
    from idfcodec import _lib
    from idfcodec._lib import lib, ptr
    L, s = lib(), _lib.stream_ptr(torch.device("cuda"))
    img = torch.zeros((3, 16, 16), dtype=torch.uint8, device="cuda")
    table = _dev([[img.data_ptr(), 16, 16, 0, 0]], torch.int64)
    seg = _dev([[img.data_ptr(), 768]], torch.int64)
    rect = _dev([[16, 16]], torch.int32)
    buf = torch.zeros(256 * 4, device="cuda")
    whole, out = _guarded_out(1)
    t, g, r, b, o = (ptr(x) for x in (table, seg, rect, buf, out))
    ERR_ARG, ERR_UNSUPPORTED = 1, 4
    assert L.idf_crc32_segments_u8(s, 0, g, o) == L.idf_crc32_segments_u8(s, 0, None, None) == 0
    assert L.idf_crc32_segments_u8(s, -1, g, o) == ERR_ARG
    assert L.idf_crc32_segments_u8(s, 1, None, o) == L.idf_crc32_segments_u8(s, 1, g, None) \
        == ERR_ARG
    u8 = lambda n, C, th, tw, t=t, o=o: L.idf_tile_crc32_u8(s, n, C, th, tw, t, o)  # noqa: E731
    pm = lambda n, C, th, tw, b=b, ld=4, r=r, o=o: L.idf_tile_crc32_pm(  # noqa: E731
        s, n, C, th, tw, b, ld, r, o)
    for call in (u8, pm):
        assert call(0, 3, 16, 16) == 0
        for n, C, th, tw in ((1, 0, 16, 16), (1, 5, 16, 16), (1, 3, 0, 16), (1, 3, 16, 0),
                             (-1, 3, 16, 16)):
            assert call(n, C, th, tw) == ERR_ARG, (n, C, th, tw)
        assert call(1, 3, 8192, 8192) == ERR_UNSUPPORTED
        assert call(1, 3, 16, 16, o=None) == ERR_ARG
    assert u8(1, 3, 16, 16, t=None) == ERR_ARG
    assert pm(1, 3, 16, 16, b=None) == pm(1, 3, 16, 16, r=None) == pm(1, 3, 16, 16, ld=2) \
        == ERR_ARG
    torch.cuda.synchronize()
    assert _u32(whole) == [SENTINEL] * len(whole)      # nothing ran


# ------------------------------------------------------------------ 2. tiles
def _tile_case(C, th, tw):
    from idfcodec.tiled import TileLayout
    rng = np.random.default_rng(1000 * C + th)
    imgs = [rng.integers(0, 256, (C, H, W), dtype=np.uint8) for H, W in KERNEL_SIZES]
    src = [torch.from_numpy(i).cuda() for i in imgs]
    lay = TileLayout(KERNEL_SIZES, C, (th, tw))
    rows = lay.rows([t.data_ptr() for t in src])
    return imgs, src, lay, rows, crc_ref.tile_crcs(imgs, th, tw)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_tile_crc_of_sources_and_of_gathered_tiles_equal_zlib(C, th, tw):
    from idfcodec.integrity import device_tile_crc32, device_tile_crc32_pm
    from idfcodec.tiled import device_gather, device_scatter
    imgs, src, lay, rows, want = _tile_case(C, th, tw)
    n = len(rows)
    assert (C * th * tw > 4096) == (max(C * h * w for h, w in lay.rects) > 4096)
    # rows with no in-image part: a negative origin, an origin past the image
    H, W = SIZES[4]
    extra = [(src[4].data_ptr(), H, W, -th, 0), (src[4].data_ptr(), H, W, 0, -1),
             (src[4].data_ptr(), H, W, H, 0), (src[4].data_ptr(), H, W, 0, W)]
    table = _dev(rows + extra, torch.int64)
    whole, out = _guarded_out(n + 4)
    device_tile_crc32(table, n + 4, C, th, tw, out)
    assert _u32(out) == want + [0] * 4
    assert _sentinels_intact(whole, n + 4)
    assert all(np.array_equal(s.cpu().numpy(), i) for s, i in zip(src, imgs))
    # the same bytes from the pixel-major rows the decode lanes leave
    buf = torch.zeros(n * th * tw * 4, device="cuda")
    device_gather(table, n, C, th, tw, buf)
    rect = _dev(lay.rects, torch.int32)
    whole, out = _guarded_out(n)
    device_tile_crc32_pm(buf, n, C, th, tw, rect, out)
    assert _u32(out) == want and _sentinels_intact(whole, n)
    # the pad is never read into the sum: NaN at every pad position
    b4 = buf.view(n, th, tw, 4)
    for t, (h, w) in enumerate(lay.rects):
        b4[t, h:, :, :] = float("nan")
        b4[t, :, w:, :] = float("nan")
    if C < 4:
        b4[:, :, :, C:] = float("nan")
    device_tile_crc32_pm(buf, n, C, th, tw, rect, out)
    assert _u32(out) == want and _sentinels_intact(whole, n)
    # a value off the grid and one out of range: the bytes the scatter writes for them
    k = max(range(n), key=lambda e: lay.rects[e][0] * lay.rects[e][1])   # the largest part
    h, w = lay.rects[k]
    b4[k, 0, 0, 0] = 37.5 / 256
    b4[k, h - 1, w - 1, C - 1] = 300 / 256
    if h * w > 2:
        b4[k, 0, 1, 0] = -3 / 256
    outs = [torch.zeros_like(s) for s in src]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    device_scatter(_dev(lay.rows([o.data_ptr() for o in outs]), torch.int64), n, C, th, tw, buf,
                   bad)
    device_tile_crc32_pm(buf, n, C, th, tw, rect, out)
    written = crc_ref.tile_crcs([o.cpu().numpy() for o in outs], th, tw)
    assert int(bad.item()) >= 2 and written[k] != want[k]
    assert [e for e in range(n) if written[e] != want[e]] == [k]
    assert _u32(out) == written


# ------------------------------------------------------------------ 3. round trips
def _sealed_codec(model, safe, mb, ways):
    from idfcodec.integrity import SealedCodec
    from idfcodec.safe import SafeTiledCodec
    from idfcodec.tiled import TiledCodec
    return SealedCodec((SafeTiledCodec if safe else TiledCodec)(model, max_batch=mb, ways=ways))


@pytest.mark.parametrize("ways", [1, 8])
@pytest.mark.parametrize("mb", [256, 4])
@pytest.mark.parametrize("safe,ratio", [(False, None), (True, 1.0), (True, 2.0),
                                        (True, math.inf)])
def test_sealed_round_trip(model16, ragged, ragged_crcs, safe, ratio, mb, ways):
    from idfcodec.integrity import SealedBitstream
    zc = _sealed_codec(model16, safe, mb, ways)
    kw = {"max_ratio": ratio} if safe else {}
    zbs = zc.encode(ragged, **kw)
    plain = zc.codec.encode(ragged, **kw)
    N = 13
    assert zbs.crc.dtype == np.uint32 and zbs.crc.tolist() == ragged_crcs
    assert zbs.inner.to_bytes() == plain.to_bytes()
    buf = zbs.to_bytes()
    assert len(buf) == len(plain.to_bytes()) + 28 + 4 * N
    back = SealedBitstream.from_bytes(buf, device="cuda")
    assert back.to_bytes() == buf
    if safe:
        n_raw = int(back.inner.escaped.sum())
        assert {1.0: n_raw == N, 2.0: 0 < n_raw < N, math.inf: n_raw == 0}[ratio]
    out, info = zc.decode(back)
    assert info["crc_bad"] == [] and info["ok"] is True and info["tiles"] == N
    assert all(torch.equal(a, b) for a, b in zip(out, ragged))
    # the unsealed codec's info is there as it was
    _, pinfo = zc.codec.decode(plain)
    assert {k for k in pinfo} | {"crc_bad"} == set(info)
    assert torch.equal(info["final_states"], pinfo["final_states"])
    # a subset in another order, a region, and the sums left on the device
    out, info = zc.decode(back, images=[4, 0])
    assert info["crc_bad"] == [] and info["ok"] and info["tiles"] == 7
    assert torch.equal(out[0], ragged[4]) and torch.equal(out[1], ragged[0])
    crop, info = zc.decode_region(back, 4, 14, 13, 5, 6)
    assert info["crc_bad"] == [] and info["ok"] and info["tiles"] == 4
    assert torch.equal(crop, ragged[4][:, 14:19, 13:19])
    out, info = zc.decode(back, images=[3, 1], verify=False)
    assert "ok" not in info and "crc_bad" not in info
    assert info["crc_entries"] == [4, 5, 6, 1]
    assert _u32(info["crc"]) == [ragged_crcs[e] for e in (4, 5, 6, 1)]


def test_tiled_sealed_is_cached_beside_tiled_and_tiled_safe(model16):
    from idfcodec.safe import SafeTiledCodec
    zs, zt = model16.tiled_sealed(), model16.tiled_sealed(safe=False)
    assert isinstance(zs.codec, SafeTiledCodec) and zs.codec is model16.tiled_safe()
    assert zt.codec is model16.tiled() and not isinstance(zt.codec, SafeTiledCodec)
    assert model16.tiled_sealed(safe=False) is zt
    z8 = model16.tiled_sealed(max_batch=4, ways=8)
    assert z8.ways == 8 and z8.max_batch == 4 and z8.codec is model16.tiled_safe(4, 8)
    model16.tiled_safe(256, 1), model16.tiled(256, 1)      # as the other tests expect them


# ------------------------------------------------------------------ 4. damage
def test_one_damaged_raw_tile_is_named(model16, ragged):
    from idfcodec.integrity import SealedBitstream, bad_tiles
    from idfcodec.safe import raw_offsets
    zc = _sealed_codec(model16, True, 256, 1)
    zbs = SealedBitstream.from_bytes(zc.encode(ragged).to_bytes(), device="cuda")
    assert zbs.inner.escaped.all()
    k = 7                                   # tile (0, 0) of the 37x21 image
    offs, _ = raw_offsets(zbs.inner.escaped, zbs.inner.rects(), 3)
    zbs.inner.raw[offs[k] + 300] ^= 0x20    # channel 1, row 2, column 12 of the stored tile
    out, info = zc.decode(zbs)
    assert info["crc_bad"] == [k] and info["ok"] is False and info["raw_tiles"] == 13
    assert bad_tiles(zbs, info["crc_bad"]) == [(4, 0, 0)]
    assert all(torch.equal(a, b) for a, b in zip(out[:4], ragged[:4]))
    diff = (out[4] != ragged[4]).nonzero().tolist()
    assert diff == [[1, 2, 12]]             # every other tile's pixels are exact
    # a region that does not touch the entry, and one that does
    crop, info = zc.decode_region(zbs, 4, 20, 3, 14, 10)    # tiles (1, 0) and (2, 0)
    assert info["crc_bad"] == [] and info["ok"] and info["tiles"] == 2
    assert torch.equal(crop, ragged[4][:, 20:34, 3:13])
    crop, info = zc.decode_region(zbs, 4, 10, 10, 8, 8)     # tiles (0..1, 0..1): entries 7..10
    assert info["crc_bad"] == [k] and not info["ok"] and info["tiles"] == 4
    assert torch.equal(crop, ragged[4][:, 10:18, 10:18])    # the damaged byte lies outside it
    out, info = zc.decode(zbs, images=[0, 1, 2, 3])
    assert info["crc_bad"] == [] and info["ok"]


@pytest.mark.parametrize("mb", [256, 4])
def test_one_damaged_coded_tile_is_named(model16, ragged, mb):
    """The corruption test_decode_check_escapes_exactly_the_corrupted_tile decodes: entry 7,
    level 0, word offset + 2, ^ 0x00010000."""
    from idfcodec.integrity import SealedBitstream
    from idfcodec.tiled import tiles_host
    zc = _sealed_codec(model16, True, mb, 1)
    zbs = SealedBitstream.from_bytes(zc.encode(ragged, max_ratio=math.inf).to_bytes(),
                                     device="cuda")
    assert not zbs.inner.escaped.any()
    k = 7
    s = zbs.inner.stream
    assert int(s.nwords_host()[k]) > 4
    at = int(s.word_offsets()[k].item()) + 2
    s.words[at] = s.words[at] ^ 0x00010000
    out, info = zc.decode(zbs)
    assert info["crc_bad"] == [k] and info["ok"] is False
    assert all(torch.equal(a, b) for a, b in zip(out[:4], ragged[:4]))
    got, want = out[4].cpu().numpy(), ragged[4].cpu().numpy()
    same = [np.array_equal(a, b) for a, b in zip(tiles_host(got, 16, 16),
                                                 tiles_host(want, 16, 16))]
    assert same == [False] + [True] * 5     # the other 12 tiles are exact


# ------------------------------------------------------------------ 5. the fingerprint
def test_fingerprint_follows_the_weights(model16, ragged, monkeypatch):
    from idfcodec import integrity
    from idfcodec.integrity import model_fingerprint
    launches = []
    real = integrity.device_crc32_segments
    monkeypatch.setattr(integrity, "device_crc32_segments",
                        lambda *a: (launches.append(a[1]), real(*a))[1])
    other = _tiny_model(2, 2, 16, 16, 3, 2).cuda()
    fp = model_fingerprint(other)
    assert 0 <= fp < 1 << 32 and model_fingerprint(other) == fp
    assert launches == [len(other.state_dict())]            # one launch for the two calls
    assert model_fingerprint(model16) == fp                  # two builds of one seed
    assert model_fingerprint(other.cpu().cuda()) == fp
    zc = other.tiled_sealed()
    zbs = zc.encode(ragged, max_ratio=math.inf)
    assert zbs.fingerprint == fp
    # the lowest mantissa bit of one weight
    w = max(other.parameters(), key=lambda p: p.numel())
    with torch.no_grad():
        bits = w.view(-1).view(torch.int32)
        bits[0] ^= 1
    fp_flip = model_fingerprint(other)
    assert fp_flip != fp
    zc = other.tiled_sealed()
    other.codec()

    def no_decode(*a, **k):
        raise AssertionError("decoded a file of another model")
    monkeypatch.setattr(zc.codec, "_decode_entries", no_decode)
    monkeypatch.setattr(torch, "empty", no_decode)           # no output is allocated either
    with pytest.raises(ValueError, match="fingerprint"):
        zc.decode(zbs)
    with pytest.raises(ValueError, match="fingerprint"):
        zc.decode_region(zbs, 1, 0, 0, 4, 4)
    monkeypatch.undo()
    out, info = zc.decode(zbs, check_model=False)
    assert len(out) == 5 and isinstance(info["crc_bad"], list)
    assert not (info["crc_bad"] and info["ok"])
    wrong = [e for e, (a, b) in enumerate(zip(
        crc_ref.tile_crcs([t.cpu().numpy() for t in out], 16, 16), zbs.crc.tolist())) if a != b]
    assert info["crc_bad"] == wrong          # whatever tiles differ, and exactly those
    # back again: the first fingerprint; and the precision is part of it
    with torch.no_grad():
        bits[0] ^= 1
    assert model_fingerprint(other) == fp
    other.idf_precision = "bf16"
    assert model_fingerprint(other) not in (fp, fp_flip)
