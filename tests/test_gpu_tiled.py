"""Images of any size as tiles, on the device: the gather / scatter kernels against the
reference's ReplicationPad2d + Patching tiles, the tiled codec's exact round trip of a ragged
list, its identity with the plain codec on exact multiples, invariance under the chunk size,
the lanes and the batch, the one-mode rule, region and subset decode, and a non-square tile
model.  Tiny models only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0xAB


@pytest.fixture(scope="module")
def tiny(golden):
    d = golden("tiled_tiny.npz")
    return [(d[f"img{k}"], d[f"tiles{k}"], tuple(int(v) for v in d[f"tile_hw{k}"]))
            for k in range(int(d["n"]))]


@pytest.fixture(scope="module")
def model16():
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", 2, 2, 16, 16, 3, _dense(24, 3), _dense(16, 2),
                                        2)).cuda()


@pytest.fixture(scope="module")
def model12x8():
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", 2, 1, 12, 8, 3, _dense(24, 3), _dense(16, 2),
                                        1)).cuda()


@pytest.fixture(scope="module")
def ragged(tiny):
    """1x1, 16x16, 17x16, 5x40, 37x21 (the fixture's) and a 64x64: 1 + 1 + 2 + 3 + 6 + 16 tiles"""
    from idfcodec import synthetic
    imgs = [torch.from_numpy(img).cuda() for img, _, hw in tiny if hw == (16, 16)]
    return imgs + [synthetic.images(1, 3, 64, 64, seed=61)[0].cuda()]


def _dequant(u8):
    k = torch.as_tensor(u8).to(torch.int32)
    return (k + (k >= 128)).float() / 256


def _table(bufs, th, tw):
    """One row (addr, H, W, y0, x0) per tile of every [C, H, W] device buffer, in entry order."""
    from idfcodec.tiled import tile_table
    _, entries = tile_table([b.shape[1:] for b in bufs], th, tw)
    rows = [(bufs[i].data_ptr(), bufs[i].shape[1], bufs[i].shape[2], ty * th, tx * tw)
            for i, ty, tx in entries]
    return torch.tensor(rows, dtype=torch.int64, device="cuda"), len(rows)


def _guarded(shapes, gap=64):
    """uint8 buffers of `shapes` carved out of one buffer of guard bytes, `gap` of them around
    each: (the whole buffer, the views)."""
    total = gap + sum(int(np.prod(s)) + gap for s in shapes)
    big = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    views, o = [], gap
    for s in shapes:
        n = int(np.prod(s))
        views.append(big[o:o + n].view(*s))
        o += n + gap
    return big, views


def _guards_intact(big, views, want):
    """big equals guard bytes everywhere but in the views, which hold `want`."""
    ref = torch.full_like(big, GUARD)
    base = big.data_ptr()
    for v, w in zip(views, want):
        o = v.data_ptr() - base
        ref[o:o + v.numel()] = torch.as_tensor(w).cuda().reshape(-1)
    return torch.equal(big, ref)


def _same_streams(a, b):
    assert a.n_images == b.n_images and a.meta["conv"] == b.meta["conv"]
    assert torch.equal(a.states, b.states) and torch.equal(a.nwords, b.nwords)
    assert torch.equal(a.words, b.words)


# ------------------------------------------------------------------ 1. gather kernel
@pytest.mark.parametrize("which", ["c3_16x16", "c1_12x8"])
def test_gather_equals_reference_tiles(tiny, which):
    from idfcodec.tiled import device_gather
    sets = [s for s in tiny if (s[2] == (16, 16)) == (which == "c3_16x16")]
    th, tw = sets[0][2]
    C = sets[0][0].shape[0]
    assert C == (3 if which == "c3_16x16" else 1)
    src = [torch.from_numpy(img).cuda() for img, _, _ in sets]
    assert all(np.isin([0, 127, 128, 255], img).all() for img, _, _ in sets if img.size > C)
    table, n = _table(src, th, tw)
    assert n == sum(t.shape[0] for _, t, _ in sets)
    out = torch.full((n * th * tw * 4,), -7.0, device="cuda")
    device_gather(table, n, C, th, tw, out)
    out = out.view(n, th, tw, 4).cpu()
    want = torch.cat([_dequant(t) for _, t, _ in sets]).permute(0, 2, 3, 1)
    assert torch.equal(out[..., :C], want)
    assert bool((out[..., C:] == -7.0).all())   # columns >= C are not written


def test_gather_scatter_tiles_of_several_blocks():
    """A 40x33 tile is 1320 pixels: two blocks of the kernels per tile, the second partly
    filled.  Against the numpy restatement (itself pinned by the fixture on the host)."""
    from idfcodec import synthetic
    from idfcodec.tiled import device_gather, device_scatter, tiles_host
    th, tw = 40, 33
    imgs = [synthetic.images(1, 3, H, W, seed=62 + H)[0] for H, W in ((45, 70), (40, 33))]
    src = [t.cuda() for t in imgs]
    table, n = _table(src, th, tw)
    assert n == 6 + 1
    buf = torch.full((n * th * tw * 4,), -7.0, device="cuda")
    device_gather(table, n, 3, th, tw, buf)
    want = torch.cat([_dequant(tiles_host(t.numpy(), th, tw)) for t in imgs]).permute(0, 2, 3, 1)
    assert torch.equal(buf.view(n, th, tw, 4)[..., :3].cpu(), want)
    big, outs = _guarded([t.shape for t in imgs])
    otab, _ = _table(outs, th, tw)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    device_scatter(otab, n, 3, th, tw, buf, bad)
    assert int(bad.item()) == 0 and _guards_intact(big, outs, imgs)


# ------------------------------------------------------------------ 2. scatter kernel
def test_scatter_inverts_gather_inside_guards(tiny):
    from idfcodec.tiled import device_gather, device_scatter
    for th, tw in ((16, 16), (12, 8)):
        imgs = [img for img, _, hw in tiny if hw == (th, tw)]
        C = imgs[0].shape[0]
        src = [torch.from_numpy(i).cuda() for i in imgs]
        table, n = _table(src, th, tw)
        buf = torch.zeros(n * th * tw * 4, device="cuda")
        device_gather(table, n, C, th, tw, buf)
        big, outs = _guarded([i.shape for i in imgs])
        otab, _ = _table(outs, th, tw)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        device_scatter(otab, n, C, th, tw, buf, bad)
        assert int(bad.item()) == 0
        assert _guards_intact(big, outs, imgs), (th, tw)   # exact images, the pad never written


def test_scatter_negative_origin_writes_only_the_crop(tiny):
    from idfcodec.tiled import device_gather, device_scatter
    img = next(i for i, _, _ in tiny if i.shape == (3, 37, 21))
    src = torch.from_numpy(img).cuda()
    table, n = _table([src], 16, 16)
    buf = torch.zeros(n * 256 * 4, device="cuda")
    device_gather(table, n, 3, 16, 16, buf)
    # rows [18, 23) x columns [3, 10): inside tile (1, 0), entry 2, smaller than the tile
    y0, x0, h, w = 18, 3, 5, 7
    big, (crop,) = _guarded([(3, h, w)])
    row = torch.tensor([[crop.data_ptr(), h, w, 16 - y0, 0 - x0]], dtype=torch.int64,
                       device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    device_scatter(row, 1, 3, 16, 16, buf[2 * 256 * 4:], bad)
    assert int(bad.item()) == 0
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])
    # a crop across the four tiles (0..1, 0..1), each clipped on two sides
    y0, x0, h, w = 14, 13, 5, 6
    big, (crop,) = _guarded([(3, h, w)])
    rows = torch.tensor([[crop.data_ptr(), h, w, ty * 16 - y0, tx * 16 - x0]
                         for ty in (0, 1) for tx in (0, 1)], dtype=torch.int64, device="cuda")
    device_scatter(rows, 4, 3, 16, 16, buf, bad)   # entries 0..3 are those four tiles
    assert int(bad.item()) == 0
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])


def test_scatter_counts_off_grid_only_where_written(tiny):
    from idfcodec.tiled import device_gather, device_scatter
    img = next(i for i, _, _ in tiny if i.shape == (3, 17, 16))   # tile 1: row 0 image, rest pad
    src = torch.from_numpy(img).cuda()
    table, n = _table([src], 16, 16)
    assert n == 2
    buf = torch.zeros(n * 256 * 4, device="cuda")
    device_gather(table, n, 3, 16, 16, buf)
    out = torch.empty_like(src)
    otab, _ = _table([out], 16, 16)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    px = lambda t, r, c, ch: ((t * 16 + r) * 16 + c) * 4 + ch  # noqa: E731
    in_image = [px(0, 3, 5, 1), px(1, 0, 15, 2)]     # (3, 5) and (16, 15): written
    in_pad = [px(1, 1, 0, 0), px(1, 15, 15, 2)]      # rows 17 and 31: the pad
    for i in in_pad:
        buf[i] += 1.0 / 512
    device_scatter(otab, n, 3, 16, 16, buf, bad)
    assert int(bad.item()) == 0 and torch.equal(out, src)   # the pad is not looked at
    for i in in_image:
        buf[i] += 1.0 / 512
    device_scatter(otab, n, 3, 16, 16, buf, bad)
    assert int(bad.item()) == len(in_image)
    assert int((out != src).sum().item()) <= len(in_image)
    # 128/256 is no value of the dequantiser, 257/256 and NaN are outside: counted as well
    bad.zero_()
    buf[px(0, 0, 0, 0)], buf[px(0, 0, 1, 0)], buf[px(0, 0, 2, 0)] = 0.5, 257 / 256, float("nan")
    device_scatter(otab, n, 3, 16, 16, buf, bad)
    assert int(bad.item()) == len(in_image) + 3


def test_tile_launchers_check_their_arguments():
    from idfcodec import _lib
    from idfcodec._lib import lib, ptr
    L, s = lib(), _lib.stream_ptr(torch.device("cuda"))
    img = torch.zeros((3, 16, 16), dtype=torch.uint8, device="cuda")
    table, _ = _table([img], 16, 16)
    buf = torch.full((256 * 4,), -7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    t, b, d = ptr(table), ptr(buf), ptr(bad)
    assert L.idf_tile_gather_u8(s, 0, 3, 16, 16, t, b, 4) == _lib.IDF_OK
    assert L.idf_tile_scatter_u8(s, 0, 3, 16, 16, b, 4, t, d) == _lib.IDF_OK
    ERR_ARG = 1
    for n, C, th, tw, tab, out, ld in ((1, 0, 16, 16, t, b, 4), (1, 5, 16, 16, t, b, 8),
                                       (1, 3, 0, 16, t, b, 4), (1, 3, 16, 0, t, b, 4),
                                       (1, 3, 16, 16, t, b, 2), (1, 3, 16, 16, None, b, 4),
                                       (1, 3, 16, 16, t, None, 4), (-1, 3, 16, 16, t, b, 4)):
        assert L.idf_tile_gather_u8(s, n, C, th, tw, tab, out, ld) == ERR_ARG, (n, C, th, tw, ld)
        assert L.idf_tile_scatter_u8(s, n, C, th, tw, out, ld, tab, d) == ERR_ARG
    assert L.idf_tile_scatter_u8(s, 1, 3, 16, 16, b, 4, t, None) == ERR_ARG
    torch.cuda.synchronize()
    # nothing ran: the buffers are as they were
    assert bool((buf == -7.0).all()) and int(bad.item()) == 0 and int(img.sum().item()) == 0


# ------------------------------------------------------------------ 3. round trip
def test_ragged_round_trip(model16, ragged):
    from idfcodec.tiled import TiledBitstream
    tc = model16.tiled()
    assert tc is model16.tiled() and tc.max_batch == 256
    tbs = tc.encode(ragged)
    assert tbs.sizes == [(1, 1), (16, 16), (17, 16), (5, 40), (37, 21), (64, 64)]
    assert tbs.stream.n_images == 29 and tbs.stream.n_streams == 2 * 29
    out, info = tc.decode(tbs)
    assert info["ok"] and info["tiles"] == 29 and int(info["off_grid"].item()) == 0
    assert len(out) == len(ragged) and all(torch.equal(a, b) for a, b in zip(out, ragged))
    raw = tbs.to_bytes()
    for dev in ("cuda", None):      # the streams on the device, or left on the host
        back = TiledBitstream.from_bytes(raw, device=dev)
        out, info = tc.decode(back)
        assert info["ok"] and all(torch.equal(a, b) for a, b in zip(out, ragged)), dev
    nsub = 3 * sum(H * W for H, W in tbs.sizes)
    assert tbs.bpd() == tbs.bits() / nsub
    assert tbs.stream.bpd() == tbs.bits() / (29 * 3 * 256) < tbs.bpd()
    assert tbs.state_bits_per_subpixel() == 64 * 58 / nsub


def test_encode_input_errors(model16, ragged):
    tc = model16.tiled()
    ok = ragged[1]
    wide = torch.zeros((3, 16, 40), dtype=torch.uint8, device="cuda")
    for bad in ([], torch.zeros((0, 3, 16, 16), dtype=torch.uint8, device="cuda"),
                [ok, torch.zeros((1, 16, 16), dtype=torch.uint8, device="cuda")],
                [torch.zeros((3, 0, 16), dtype=torch.uint8, device="cuda")],
                [torch.zeros((3, 16, 0), dtype=torch.uint8, device="cuda")],
                [ok.float()], [ok.cpu()], [wide[:, :, :17]], [ok[None]],
                wide[None][:, :, :, ::2]):
        with pytest.raises(ValueError):
            tc.encode(bad)


# ------------------------------------------------------------------ 4. identity with ImageCodec
def test_exact_multiples_equal_the_plain_codec(model16):
    from idfcodec import synthetic
    tc = model16.tiled()
    batch = synthetic.images(5, 3, 16, 16, seed=63).cuda()
    assert tc.encode(batch).stream.to_bytes() == model16.encode(batch).to_bytes()
    img = synthetic.images(1, 3, 32, 48, seed=64)[0].cuda()
    # Patching(32, 48, 16, 16).forward of the one image
    tiles = img.view(3, 2, 16, 3, 16).permute(1, 3, 0, 2, 4).reshape(6, 3, 16, 16).contiguous()
    tbs = tc.encode([img])
    assert tbs.stream.to_bytes() == model16.encode(tiles).to_bytes()
    out, info = tc.decode(tbs)
    assert info["ok"] and torch.equal(out[0], img)


# ------------------------------------------------------------------ 5. chunk invariance
def test_chunk_size_does_not_change_the_bytes(model16, ragged):
    from idfcodec.tiled import TiledCodec
    imgs = ragged[:5]      # 13 tiles
    ref = TiledCodec(model16, max_batch=256).encode(imgs).to_bytes()
    for mb in (1, 3, 4):
        tc = TiledCodec(model16, max_batch=mb)
        tbs = tc.encode(imgs)
        assert tbs.to_bytes() == ref, mb
        out, info = tc.decode(tbs)
        assert info["ok"] and info["tiles"] == 13, mb
        assert all(torch.equal(a, b) for a, b in zip(out, imgs)), mb


def test_lanes_do_not_change_the_bytes(model16, ragged):
    from idfcodec import synthetic
    from idfcodec.tiled import TiledCodec
    imgs = [synthetic.images(1, 3, 64, 128, seed=65)[0].cuda(), ragged[4]]    # 32 + 6 tiles
    ic = model16.codec()
    assert ic.LANE_MIN == 8
    calls = []
    enc_lanes = ic._encode_lanes

    def spy(*a, **k):
        calls.append((a[1], a[2]))  # (B, nl)
        return enc_lanes(*a, **k)

    ic._encode_lanes = spy
    lanes, enc = ic.lanes, ic.enc_lanes
    try:
        ic.lanes = ic.enc_lanes = 1
        tc = TiledCodec(model16)
        ref = tc.encode(imgs)
        ref_out, ref_info = tc.decode(ref)
        assert not calls and ref_info["ok"]
        assert all(torch.equal(a, b) for a, b in zip(ref_out, imgs))
        ic.lanes = ic.enc_lanes = 2
        for mb, want in ((256, [(38, 2)]), (16, [(16, 2), (16, 2)])):   # the 6 left: one lane
            calls.clear()
            tc = TiledCodec(model16, max_batch=mb)
            got = tc.encode(imgs)
            torch.cuda.synchronize()
            assert calls == want, (mb, calls)
            assert got.to_bytes() == ref.to_bytes(), mb
            assert ic._n_lanes(min(mb, 38)) == 2
            out, info = tc.decode(got)
            torch.cuda.synchronize()
            assert info["ok"] and all(torch.equal(a, b) for a, b in zip(out, ref_out)), mb
    finally:
        ic.lanes, ic.enc_lanes = lanes, enc
        del ic._encode_lanes


# ------------------------------------------------------------------ 6. batch invariance
def test_image_codes_identically_alone(model16, ragged):
    tc = model16.tiled()
    full = tc.encode(ragged)
    counts = full.tile_counts()
    assert counts == [1, 1, 2, 3, 6, 16]
    for i in (0, 2, 4):
        alone = tc.encode([ragged[i]])
        first = sum(counts[:i])
        part = full.stream.select(range(first, first + counts[i]))
        _same_streams(part, alone.stream)
        assert int(alone.stream.nwords.sum()) > 0
        assert part.n_subpixels() == alone.stream.n_subpixels() == counts[i] * 3 * 256


# ------------------------------------------------------------------ 7. one conv mode
def test_range_guard_in_one_chunk_recodes_all_in_f32(model16, ragged, monkeypatch):
    from idfcodec.codec import SPLIT_F16
    from idfcodec.tiled import TiledBitstream, TiledCodec
    imgs = ragged[:5]      # 13 tiles: chunks of 4, 4, 4, 1
    tc = TiledCodec(model16, max_batch=4)
    eng = model16.engine()
    mode = eng.conv_mode
    assert eng.conv_family in SPLIT_F16      # the guard exists only for the split-f16 convs
    plain = tc.encode(imgs)
    assert plain.stream.meta["conv"] == mode
    eng.set_conv_mode("f32")
    try:
        ref = tc.encode(imgs)
    finally:
        eng.set_conv_mode(mode)
    assert ref.stream.meta["conv"] == "f32"
    asked = []

    def second_chunk_trips(self):
        asked.append(len(asked))
        return len(asked) == 2

    monkeypatch.setattr(type(eng), "range_flag_tripped", second_chunk_trips)
    got = tc.encode(imgs)
    monkeypatch.undo()
    assert len(asked) == 4                   # once per chunk; the f32 re-encodes never ask
    assert eng.conv_mode == mode
    assert got.stream.meta["conv"] == "f32"
    assert got.to_bytes() == ref.to_bytes() != plain.to_bytes()
    out, info = tc.decode(TiledBitstream.from_bytes(got.to_bytes(), device="cuda"))
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(out, imgs))
    assert eng.conv_mode == mode


# ------------------------------------------------------------------ 8. region and subset decode
def test_region_and_subset_decode(model16, ragged):
    from idfcodec.tiled import TiledCodec
    tc = TiledCodec(model16, max_batch=4)
    tbs = tc.encode(ragged)
    full, info = tc.decode(tbs)
    assert info["ok"]
    for image, rect in ((4, (18, 3, 5, 7)),        # inside one tile
                        (4, (14, 13, 5, 6)),       # across four tiles
                        (4, (30, 10, 7, 11)),      # the padded bottom/right edge tiles
                        (4, (36, 20, 1, 1)),       # the last pixel
                        (5, (16, 16, 32, 32)),     # exactly four whole tiles
                        (5, (0, 0, 64, 64)),       # a whole image, 16 tiles in chunks of 4
                        (0, (0, 0, 1, 1))):
        y0, x0, h, w = rect
        crop, rinfo = tc.decode_region(tbs, image, y0, x0, h, w)
        n = ((y0 + h - 1) // 16 - y0 // 16 + 1) * ((x0 + w - 1) // 16 - x0 // 16 + 1)
        assert rinfo["ok"] and rinfo["tiles"] == n, (image, rect)
        assert crop.shape == (3, h, w)
        assert torch.equal(crop, full[image][:, y0:y0 + h, x0:x0 + w]), (image, rect)
    for bad in ((4, (0, 0, 0, 5)), (4, (30, 10, 8, 11)), (4, (-1, 0, 2, 2)), (6, (0, 0, 1, 1))):
        with pytest.raises(ValueError):
            tc.decode_region(tbs, bad[0], *bad[1])
    out, sinfo = tc.decode(tbs, images=[2, 0])
    assert sinfo["ok"] and sinfo["tiles"] == 2 + 1 and len(out) == 2
    assert torch.equal(out[0], ragged[2]) and torch.equal(out[1], ragged[0])
    with pytest.raises(ValueError):
        tc.decode(tbs, images=[6])
    out, sinfo = tc.decode(tbs, images=[])
    assert out == [] and sinfo["ok"] and sinfo["tiles"] == 0


# ------------------------------------------------------------------ 9. non-square tiles
def test_non_square_tile_model_round_trip(model12x8):
    from idfcodec import synthetic
    from idfcodec.tiled import TiledBitstream
    imgs = [synthetic.images(1, 3, H, W, seed=66 + H)[0].cuda() for H, W in ((25, 9), (12, 8))]
    tc = model12x8.tiled(max_batch=4)
    assert tc.tile_hw == (12, 8) and tc.max_batch == 4 and model12x8.tiled() is tc
    tbs = tc.encode(imgs)
    assert tbs.tile_counts() == [6, 1]
    out, info = tc.decode(TiledBitstream.from_bytes(tbs.to_bytes(), device="cuda"))
    assert info["ok"] and info["tiles"] == 7
    assert all(torch.equal(a, b) for a, b in zip(out, imgs))
    crop, rinfo = tc.decode_region(tbs, 0, 11, 7, 2, 2)
    assert rinfo["ok"] and rinfo["tiles"] == 4
    assert torch.equal(crop, imgs[0][:, 11:13, 7:9])
