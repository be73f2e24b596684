"""The raw-tile escape on the device: the three byte / index kernels against numpy inside guard
bytes, and SafeTiledCodec -- a model whose top level lies outside the rANS window (TiledCodec
loses the images, SafeTiledCodec returns them), a mixed set of kept and escaped tiles, the seeded
weights at max_ratio 1, inf and in between, identical bytes across chunk sizes, batches and ways,
and check="decode" against a corrupted stream.  Tiny models only."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0xAB
SIZES = ((1, 1), (16, 16), (17, 16), (5, 40), (37, 21))


def _tiny_model(*args):
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    return synthetic.build_model(_flows("IDFlows", *args[:5], _dense(24, 3), _dense(16, 2),
                                        args[5]))


@pytest.fixture(scope="module")
def model16():
    return _tiny_model(2, 2, 16, 16, 3, 2).cuda()


@pytest.fixture(scope="module")
def model12x8():
    return _tiny_model(2, 1, 12, 8, 3, 1).cuda()


@pytest.fixture(scope="module")
def model_far():
    """The 16x16 model with the top level's prior mean moved 8.0 away: that prior is
    unconditional and |latent - mean| <= 1.2 on the seeded model, so every top-level symbol lies
    4 or more outside the rANS window of 2048 bins of 1/256 around the mean."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    prior = m.blocks[-1]["prior"]
    with torch.no_grad():
        prior.NN.layers[-1].bias[:prior.out_channel] += 8.0
    return m.cuda()


@pytest.fixture(scope="module")
def model_sharp():
    """The 16x16 model with every prior's logscale lowered by 3.0: dark tiles then cost less
    than their bytes and noise tiles more than twice them."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            b["prior"].NN.layers[-1].bias[b["prior"].out_channel:] -= 3.0
    return m.cuda()


def _noise(H, W, seed, C=3):
    from idfcodec import synthetic
    return synthetic.images(1, C, H, W, seed=seed)[0]


@pytest.fixture(scope="module")
def ragged():
    """1x1, 16x16, 17x16, 5x40, 37x21: 1 + 1 + 2 + 3 + 6 tiles of 16x16"""
    return [_noise(H, W, 70 + i).cuda() for i, (H, W) in enumerate(SIZES)]


@pytest.fixture(scope="module")
def mixed():
    """dark (bytes 0..3) 32x32, noise 16x16, dark 17x16, noise 37x21, dark 5x40:
    4 + 1 + 2 + 6 + 3 tiles"""
    dark = lambda H, W, s: _noise(H, W, s) % 4  # noqa: E731
    return [t.cuda() for t in (dark(32, 32, 80), _noise(16, 16, 81), dark(17, 16, 82),
                               _noise(37, 21, 83), dark(5, 40, 84))]


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


def _rows(bufs, th, tw):
    from idfcodec.tiled import tile_table
    _, entries = tile_table([b.shape[1:] for b in bufs], th, tw)
    return [(bufs[i].data_ptr(), bufs[i].shape[1], bufs[i].shape[2], ty * th, tx * tw)
            for i, ty, tx in entries], entries


def _dev(a, dt):
    return torch.tensor(a, dtype=dt, device="cuda")


def _kernel_case(C, th, tw):
    """The five images, their table, in-image parts, byte offsets handed out in reverse entry
    order (so the offsets fall as the entries rise, with 5 unused bytes between two parts) and the
    raw bytes numpy expects."""
    from idfcodec.safe import entry_rects
    rng = np.random.default_rng(1000 * C + th)
    imgs = [rng.integers(0, 256, (C, H, W), dtype=np.uint8) for H, W in SIZES]
    src = [torch.from_numpy(i).cuda() for i in imgs]
    rows, entries = _rows(src, th, tw)
    rects = entry_rects(SIZES, th, tw)
    offs, o = [0] * len(rects), 0
    for e in reversed(range(len(rects))):
        offs[e] = o
        o += C * rects[e][0] * rects[e][1] + 5
    want = np.full(o, GUARD, dtype=np.uint8)
    for e, (i, ty, tx) in enumerate(entries):
        h, w = rects[e]
        part = imgs[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w]
        assert part.shape == (C, h, w)
        want[offs[e]:offs[e] + part.size] = part.reshape(-1)
    return imgs, src, rows, rects, offs, want


TILES = [(16, 16), (12, 8), (40, 33)]     # 40x33 = 1320 pixels: two blocks, the second partly filled


# ------------------------------------------------------------------ 1. raw gather / scatter
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_raw_gather_and_scatter_equal_numpy_inside_guards(C, th, tw):
    from idfcodec.safe import device_gather_raw, device_scatter_raw
    imgs, src, rows, rects, offs, want = _kernel_case(C, th, tw)
    n = len(rows)
    assert offs[0] > offs[-1] == 0        # not monotone
    table = _dev(rows, torch.int64)
    d_off = _dev(offs, torch.int64)
    big, (raw,) = _guarded([(len(want),)])
    device_gather_raw(table, n, C, th, tw, d_off, raw)
    assert _guards_intact(big, [raw], [want])   # the parts exactly, nothing between or around them
    obig, outs = _guarded([i.shape for i in imgs])
    orows, _ = _rows(outs, th, tw)
    device_scatter_raw(_dev(orows, torch.int64), n, C, th, tw, raw, d_off,
                       _dev(rects, torch.int32))
    assert _guards_intact(obig, outs, imgs)
    # a subset, in another order, lands the same bytes
    pick = [n - 1, 0, n // 2]
    obig, outs = _guarded([i.shape for i in imgs])
    orows, _ = _rows(outs, th, tw)
    device_scatter_raw(_dev([orows[e] for e in pick], torch.int64), 3, C, th, tw, raw,
                       _dev([offs[e] for e in pick], torch.int64),
                       _dev([rects[e] for e in pick], torch.int32))
    ref = [np.full_like(i, GUARD) for i in imgs]
    for e in pick:
        k = next(j for j, o in enumerate(outs) if o.data_ptr() == orows[e][0])
        _, _, _, y0, x0 = orows[e]
        h, w = rects[e]
        ref[k][:, y0:y0 + h, x0:x0 + w] = imgs[k][:, y0:y0 + h, x0:x0 + w]
    assert _guards_intact(obig, outs, ref)


def test_raw_scatter_negative_origin_writes_only_the_crop():
    from idfcodec.safe import device_gather_raw, device_scatter_raw, entry_rects, raw_offsets
    img = _noise(37, 21, 90).numpy()
    src = torch.from_numpy(img).cuda()
    rows, _ = _rows([src], 16, 16)
    rects = entry_rects([(37, 21)], 16, 16)
    offs, total = raw_offsets([True] * 6, rects, 3)
    raw = torch.empty(total, dtype=torch.uint8, device="cuda")
    device_gather_raw(_dev(rows, torch.int64), 6, 3, 16, 16, _dev(offs, torch.int64), raw)
    # rows [18, 23) x columns [3, 10): inside tile (1, 0), entry 2, smaller than the tile
    y0, x0, h, w = 18, 3, 5, 7
    big, (crop,) = _guarded([(3, h, w)])
    device_scatter_raw(_dev([[crop.data_ptr(), h, w, 16 - y0, 0 - x0]], torch.int64), 1, 3, 16,
                       16, raw, _dev([offs[2]], torch.int64), _dev([rects[2]], torch.int32))
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])
    # a crop across the four tiles (0..1, 0..1), each clipped on two sides; tiles (0, 1) and
    # (1, 1) are stored 5 wide
    y0, x0, h, w = 14, 13, 5, 6
    big, (crop,) = _guarded([(3, h, w)])
    crows = [[crop.data_ptr(), h, w, ty * 16 - y0, tx * 16 - x0] for ty in (0, 1) for tx in (0, 1)]
    device_scatter_raw(_dev(crows, torch.int64), 4, 3, 16, 16, raw, _dev(offs[:4], torch.int64),
                       _dev(rects[:4], torch.int32))
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])
    # the bottom-right tile (5 x 5 stored) into a crop that reaches the image's last pixel
    y0, x0, h, w = 33, 17, 4, 4
    big, (crop,) = _guarded([(3, h, w)])
    device_scatter_raw(_dev([[crop.data_ptr(), h, w, 32 - y0, 16 - x0]], torch.int64), 1, 3, 16,
                       16, raw, _dev([offs[5]], torch.int64), _dev([rects[5]], torch.int32))
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])


# ------------------------------------------------------------------ 2. verify kernel
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_verify_counts_in_image_mismatches_per_tile(C, th, tw):
    from idfcodec.safe import device_verify
    from idfcodec.tiled import device_gather
    imgs, src, rows, rects, _, _ = _kernel_case(C, th, tw)
    n = len(rows)
    table = _dev(rows, torch.int64)
    buf = torch.zeros(n * th * tw * 4, device="cuda")
    device_gather(table, n, C, th, tw, buf)
    mism = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = lambda: (device_verify(table, n, C, th, tw, buf, mism), mism.tolist())[1]  # noqa: E731
    assert count() == [0] * n
    px = lambda t, r, c, ch: ((t * th + r) * tw + c) * 4 + ch  # noqa: E731
    # the last entry with a pad, its last in-image pixel and its last (pad) pixel; the first
    # entry's pixel (0, 0); and, where a tile has two blocks, a pixel of the second block
    k = max(e for e, (h, w) in enumerate(rects) if (h, w) != (th, tw))
    h, w = rects[k]
    spots = [(k, h - 1, w - 1, C - 1), (0, 0, 0, 0)]
    full = next((e for e, r in enumerate(rects) if r == (th, tw)), None)
    if th * tw > 1024 and full is not None:
        spots.append((full, th - 1, tw - 1, 0))       # pixel 1319 of the tile
        assert (th - 1) * tw + tw - 1 >= 1024
    for t, r, c, ch in spots:
        i = px(t, r, c, ch)
        old = float(buf[i])
        buf[i] = old + (2 / 256 if old < 0.5 else -2 / 256)    # another byte's value
        mism.zero_()
        assert count() == [int(e == t) for e in range(n)], (t, r, c, ch)
        assert count() == [2 * int(e == t) for e in range(n)]   # added to the counters
        buf[i] = old + 1 / 512                                  # off the grid
        mism.zero_()
        assert count() == [int(e == t) for e in range(n)]
        buf[i] = old
    # 128/256 is no value of the dequantiser, 257/256 and NaN are outside: each differs
    i = px(0, 0, 0, 0)
    old = float(buf[i])
    for v in (0.5, 257 / 256, -1 / 256, float("nan")):
        buf[i] = v
        mism.zero_()
        assert count() == [1] + [0] * (n - 1), v
    buf[i] = old
    # pad pixels and the columns >= C are not compared
    buf[px(k, th - 1, tw - 1, 0)] += 2 / 256
    if h < th:
        buf[px(k, h, 0, C - 1)] = float("nan")
    if w < tw:
        buf[px(k, 0, w, 0)] += 1 / 512
    if C < 4:
        buf[px(0, 0, 0, C)] = 7.0
    mism.zero_()
    assert count() == [0] * n


def test_escape_launchers_check_their_arguments():
    from idfcodec import _lib
    from idfcodec._lib import lib, ptr
    L, s = lib(), _lib.stream_ptr(torch.device("cuda"))
    img = torch.zeros((3, 16, 16), dtype=torch.uint8, device="cuda")
    table = _dev([[img.data_ptr(), 16, 16, 0, 0]], torch.int64)
    off = _dev([0], torch.int64)
    rect = _dev([[16, 16]], torch.int32)
    raw = torch.full((768,), GUARD, dtype=torch.uint8, device="cuda")
    buf = torch.full((256 * 4,), -7.0, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    t, o, r, w, b, m = (ptr(x) for x in (table, off, rect, raw, buf, mism))
    gather = lambda n, C, th, tw, t=t, o=o, w=w: L.idf_tile_gather_raw_u8(  # noqa: E731
        s, n, C, th, tw, t, o, w)
    scatter = lambda n, C, th, tw, w=w, o=o, r=r, t=t: L.idf_tile_scatter_raw_u8(  # noqa: E731
        s, n, C, th, tw, w, o, r, t)
    verify = lambda n, C, th, tw, b=b, ld=4, t=t, m=m: L.idf_tile_verify_u8(  # noqa: E731
        s, n, C, th, tw, b, ld, t, m)
    for call in (gather, scatter, verify):
        assert call(0, 3, 16, 16) == _lib.IDF_OK
    ERR_ARG, ERR_UNSUPPORTED = 1, 4
    for call in (gather, scatter, verify):
        for n, C, th, tw in ((1, 0, 16, 16), (1, 5, 16, 16), (1, 3, 0, 16), (1, 3, 16, 0),
                             (-1, 3, 16, 16)):
            assert call(n, C, th, tw) == ERR_ARG, (n, C, th, tw)
        assert call(1, 3, 8192, 8192) == ERR_UNSUPPORTED     # 65536 bands of 1024 pixels
        assert call(1, 3, 16, 16, t=None) == ERR_ARG
    assert gather(1, 3, 16, 16, o=None) == gather(1, 3, 16, 16, w=None) == ERR_ARG
    assert scatter(1, 3, 16, 16, o=None) == scatter(1, 3, 16, 16, w=None) == ERR_ARG
    assert scatter(1, 3, 16, 16, r=None) == ERR_ARG
    assert verify(1, 3, 16, 16, b=None) == verify(1, 3, 16, 16, m=None) == ERR_ARG
    assert verify(1, 3, 16, 16, ld=2) == ERR_ARG
    torch.cuda.synchronize()
    # nothing ran: the buffers are as they were
    assert bool((raw == GUARD).all()) and int(mism.item()) == 0 and int(img.sum().item()) == 0


# ------------------------------------------------------------------ 3. the defect and the fix
def test_out_of_window_tiles_are_lost_by_tiled_and_returned_by_tiled_safe(model_far, ragged):
    from idfcodec import _lib
    from idfcodec.safe import REASON_STATUS, SafeTiledBitstream
    N = 13
    tbs = model_far.tiled().encode(ragged)
    status = tbs.stream.status.view(2, N)
    # the precondition: the plain tiled bitstream is flagged and does not decode to the source
    assert bool((status[1] & _lib.STREAM_OUT_OF_WINDOW).all())
    out, info = model_far.tiled().decode(tbs)
    assert not info["ok"]
    assert not all(torch.equal(a, b) for a, b in zip(out, ragged))
    sc = model_far.tiled_safe()
    assert sc is model_far.tiled_safe() and sc is not model_far.tiled()
    for ratio, only_status in ((1.0, False), (math.inf, True)):
        sbs = sc.encode(ragged, max_ratio=ratio)
        assert sbs.escaped.all() and sbs.stream is None and sbs.n_kept == 0
        assert bool((sbs.reasons & REASON_STATUS).all())
        if only_status:
            assert sbs.reasons.tolist() == [REASON_STATUS] * N
        assert sbs.bits() == 8 * sum(t.numel() for t in ragged) and sbs.escaped_share() == 1.0
        back = SafeTiledBitstream.from_bytes(sbs.to_bytes(), device="cuda")
        for s in (sbs, back):
            out, info = sc.decode(s)
            assert info["ok"] and info["tiles"] == N and info["raw_tiles"] == N
            assert all(torch.equal(a, b) for a, b in zip(out, ragged))


# ------------------------------------------------------------------ 4. a mixed set
def _entry_ratios(tbs):
    """bits_e / (8 raw_e) of every entry of a TiledBitstream"""
    from idfcodec.safe import entry_bits, entry_rects
    rects = entry_rects(tbs.sizes, *tbs.tile_hw)
    bits = entry_bits(tbs.stream.nwords_host().numpy(), len(rects), tbs.stream.ways)
    return [float(b) / (8 * tbs.C * h * w) for b, (h, w) in zip(bits, rects)]


def test_mixed_set_of_kept_and_escaped_tiles(model_sharp, mixed):
    from idfcodec.safe import REASON_SIZE, SafeTiledBitstream, file_size_bound, inner_index
    sc = model_sharp.tiled_safe()
    sbs = sc.encode(mixed)
    N = 4 + 1 + 2 + 6 + 3
    print("bits_e / raw bits per entry:",
          [round(r, 3) for r in _entry_ratios(model_sharp.tiled().encode(mixed))])
    print("escaped:", sbs.escaped.astype(int).tolist())
    assert len(sbs.escaped) == N
    K = sbs.n_kept
    assert 0 < K < N                       # at least one kept and one escaped tile
    assert sbs.stream.n_images == K and set(sbs.reasons.tolist()) == {0, REASON_SIZE}
    out, info = sc.decode(sbs)
    assert info["ok"] and info["tiles"] == N and info["raw_tiles"] == N - K
    assert all(torch.equal(a, b) for a, b in zip(out, mixed))
    # the bound: the source plus the fixed headers
    src = sum(t.numel() for t in mixed)
    buf = sbs.to_bytes()
    assert len(buf) <= file_size_bound(sbs.sizes, 3, 16, 16, 2) \
        == src + 24 + 8 * 5 + 2 + 16 + 36 + 12 * 2
    assert sbs.bits() <= 8 * src
    assert sbs.bits() == sbs.stream.bits() + 8 * sbs.raw.numel()
    # a subset of the images, in the order asked
    out, sinfo = sc.decode(sbs, images=[2, 0])
    assert sinfo["ok"] and sinfo["tiles"] == 2 + 4
    assert sinfo["raw_tiles"] == int(sbs.escaped[5:7].sum() + sbs.escaped[0:4].sum())
    assert torch.equal(out[0], mixed[2]) and torch.equal(out[1], mixed[0])
    # regions over kept tiles only, raw tiles only and both
    esc = sbs.escaped
    assert not esc[0:4].any() and esc[4] and not esc[5] and esc[6]
    for image, rect, tiles, raw_tiles in ((0, (10, 10, 12, 12), 4, 0),     # dark 32x32: kept
                                          (1, (3, 2, 9, 11), 1, 1),        # noise 16x16: raw
                                          (2, (14, 1, 3, 9), 2, 1),        # dark 17x16: both
                                          (2, (16, 0, 1, 16), 1, 1),       # its 1x16 edge tile
                                          (3, (30, 10, 7, 11), 4, int(esc[7 + 2:7 + 6].sum()))):
        y0, x0, h, w = rect
        crop, rinfo = sc.decode_region(sbs, image, y0, x0, h, w)
        assert rinfo["ok"] and rinfo["tiles"] == tiles and rinfo["raw_tiles"] == raw_tiles, rect
        assert torch.equal(crop, mixed[image][:, y0:y0 + h, x0:x0 + w]), (image, rect)
        if raw_tiles == tiles:             # raw tiles only: no flow ran
            assert rinfo["final_states"].numel() == 0 and rinfo["status"].numel() == 0
    for bad in ((0, (0, 0, 0, 5)), (0, (30, 30, 3, 3)), (5, (0, 0, 1, 1))):
        with pytest.raises(ValueError):
            sc.decode_region(sbs, bad[0], *bad[1])
    with pytest.raises(ValueError):
        sc.decode(sbs, images=[5])
    out, sinfo = sc.decode(sbs, images=[])
    assert out == [] and sinfo["ok"] and sinfo["tiles"] == 0 and sinfo["raw_tiles"] == 0
    # both scatters inside guard bytes: the rows decode() builds, over buffers with guards
    big, outs = _guarded([t.shape for t in mixed])
    rows, _ = _rows(outs, 16, 16)
    ginfo = sc._decode_entries(sbs, list(range(N)), rows, True)
    assert ginfo["ok"] and ginfo["raw_tiles"] == N - K
    assert _guards_intact(big, outs, mixed)
    # through the container, the streams on the device or left on the host
    assert inner_index(sbs.escaped)[5] == 4
    for dev in ("cuda", None):
        back = SafeTiledBitstream.from_bytes(buf, device=dev)
        assert back.to_bytes() == buf and back.reasons is None
        out, info = sc.decode(back)
        assert info["ok"] and info["raw_tiles"] == N - K, dev
        assert all(torch.equal(a, b) for a, b in zip(out, mixed)), dev
    # another model's geometry is refused
    other = SafeTiledBitstream(sbs.stream, sbs.sizes, 3, (12, 8), sbs.escaped, sbs.raw)
    with pytest.raises(ValueError):
        sc.decode(other)


# ------------------------------------------------------------------ 5. the seeded weights
# Chosen from the per-entry ratios the test prints (seeded 16x16 model, noise images): full
# tiles cost about 1.3 times their bytes, an edge tile a whole tile's streams for a part of its
# bytes -- 4 and more for the 5x40 image's 5x16 and 5x8 parts.
BETWEEN = 2.0


def test_seeded_weights_at_ratio_1_inf_and_between(model16, ragged):
    from idfcodec.safe import REASON_SIZE, file_size_bound
    sc, tc = model16.tiled_safe(), model16.tiled()
    plain = tc.encode(ragged)
    ratios = _entry_ratios(plain)
    print("bits_e / raw bits per entry:", [round(r, 3) for r in ratios])
    N, src = 13, sum(t.numel() for t in ragged)
    # max_ratio 1: these weights do not compress noise, every tile is stored raw
    sbs = sc.encode(ragged)
    assert sbs.escaped.all() and sbs.reasons.tolist() == [REASON_SIZE] * N
    assert len(sbs.to_bytes()) == file_size_bound(sbs.sizes, 3, 16, 16, 2, kept=False)
    assert sbs.bits() == 8 * src
    out, info = sc.decode(sbs)
    assert info["ok"] and info["raw_tiles"] == N
    assert all(torch.equal(a, b) for a, b in zip(out, ragged))
    # inf: every tile kept, the inner stream is TiledCodec's byte for byte
    sbs = sc.encode(ragged, max_ratio=math.inf)
    assert not sbs.escaped.any() and sbs.raw.numel() == 0 and not sbs.reasons.any()
    assert sbs.stream.to_bytes() == plain.stream.to_bytes()
    assert sbs.bits() == plain.bits()
    out, info = sc.decode(sbs)
    assert info["ok"] and info["tiles"] == N and info["raw_tiles"] == 0
    assert all(torch.equal(a, b) for a, b in zip(out, ragged))
    # in between: full tiles are kept, the 5x40 image's edge tiles (entries 4..6) escape
    sbs = sc.encode(ragged, max_ratio=BETWEEN)
    full = [e for e, r in enumerate(sbs.rects()) if r == (16, 16)]
    assert full == [1, 2, 7, 9] and all(ratios[e] <= BETWEEN for e in full)
    assert all(ratios[e] > BETWEEN for e in (4, 5, 6))
    assert not sbs.escaped[full].any() and sbs.escaped[4:7].all()
    assert sbs.escaped.tolist() == [r > BETWEEN for r in ratios]
    out, info = sc.decode(sbs)
    assert info["ok"] and info["raw_tiles"] == int(sbs.escaped.sum())
    assert all(torch.equal(a, b) for a, b in zip(out, ragged))


# ------------------------------------------------------------------ 6. identical bytes
def _same_streams(a, b):
    assert a.n_images == b.n_images and a.meta["conv"] == b.meta["conv"] and a.ways == b.ways
    assert torch.equal(a.states, b.states) and torch.equal(a.nwords, b.nwords)
    assert torch.equal(a.words, b.words)


def test_chunk_size_does_not_change_the_bytes(model_sharp, mixed):
    from idfcodec.safe import SafeTiledCodec
    ref = SafeTiledCodec(model_sharp, max_batch=256).encode(mixed)
    assert 0 < ref.n_kept < len(ref.escaped)
    for mb in (1, 3):
        sc = SafeTiledCodec(model_sharp, max_batch=mb)
        for check in ("status", "decode"):
            sbs = sc.encode(mixed, check=check)
            assert sbs.to_bytes() == ref.to_bytes(), (mb, check)
            assert sbs.reasons.tolist() == ref.reasons.tolist()
        out, info = sc.decode(sbs)
        assert info["ok"] and all(torch.equal(a, b) for a, b in zip(out, mixed)), mb


def test_image_codes_identically_alone(model_sharp, mixed):
    from idfcodec.safe import inner_index, raw_offsets
    sc = model_sharp.tiled_safe()
    full = sc.encode(mixed)
    counts = full.tile_counts()
    assert counts == [4, 1, 2, 6, 3]
    inner = inner_index(full.escaped)
    offs, _ = raw_offsets(full.escaped, full.rects(), 3)
    for i in (0, 2, 3):
        alone = sc.encode([mixed[i]])
        first = sum(counts[:i])
        ent = range(first, first + counts[i])
        assert alone.escaped.tolist() == full.escaped[first:first + counts[i]].tolist()
        assert alone.reasons.tolist() == full.reasons[first:first + counts[i]].tolist()
        kept = [inner[e] for e in ent if not full.escaped[e]]
        if kept:
            _same_streams(full.stream.select(kept), alone.stream)
        else:
            assert alone.stream is None
        lo = min((offs[e] for e in ent if full.escaped[e]), default=0)
        assert torch.equal(alone.raw, full.raw[lo:lo + alone.raw.numel()])
        part_bits = (full.stream.select(kept).bits() if kept else 0) + 8 * alone.raw.numel()
        assert alone.bits() == part_bits


def test_ways_follow_the_inner_stream(model_sharp, mixed):
    from idfcodec.safe import SafeTiledBitstream
    for ways in (1, 8):
        sc = model_sharp.tiled_safe(ways=ways)
        assert sc.ways == ways
        for ratio in (1.0, math.inf):
            sbs = sc.encode(mixed, max_ratio=ratio)
            if sbs.stream is not None:
                assert sbs.stream.ways == ways
                assert sbs.stream.states.numel() == 2 * sbs.n_kept * ways
            back = SafeTiledBitstream.from_bytes(sbs.to_bytes(), device="cuda")
            assert back.stream is None or back.stream.ways == ways
            # any SafeTiledCodec of the model decodes it: the ways are the stream's
            out, info = model_sharp.tiled_safe(ways=1).decode(back)
            assert info["ok"] and all(torch.equal(a, b) for a, b in zip(out, mixed)), ways
            if ratio == math.inf:
                assert not sbs.escaped.any()
            else:
                assert sbs.bits() <= 8 * sum(t.numel() for t in mixed)


# ------------------------------------------------------------------ 7. check="decode"
def test_decode_check_escapes_exactly_the_corrupted_tile(model16, ragged):
    from idfcodec.safe import REASON_VERIFY, SafeTiledCodec
    N, k = 13, 7          # entry 7: tile (0, 0) of the 37x21 image, a full tile

    class OneBadWord(SafeTiledCodec):
        hit = 0

        def _coded(self, images):
            tbs = super()._coded(images)
            s = tbs.stream
            assert int(s.nwords_host()[k]) > 4       # level 0 of entry k
            at = int(s.word_offsets()[k].item()) + 2
            s.words[at] = s.words[at] ^ 0x00010000
            self.hit += 1
            return tbs

    for mb in (256, 4):
        bad = OneBadWord(model16, max_batch=mb)
        good = SafeTiledCodec(model16, max_batch=mb)
        # the status check cannot see it: the file does not decode to the source
        sbs = bad.encode(ragged, max_ratio=math.inf)
        assert not sbs.escaped.any()
        out, info = bad.decode(sbs)
        assert not (info["ok"] and all(torch.equal(a, b) for a, b in zip(out, ragged)))
        # the decode check does
        sbs = bad.encode(ragged, max_ratio=math.inf, check="decode")
        assert bad.hit == 2
        assert sbs.reasons.tolist() == [REASON_VERIFY if e == k else 0 for e in range(N)]
        assert sbs.n_kept == N - 1 and sbs.raw.numel() == 3 * 256
        out, info = bad.decode(sbs)
        assert info["ok"] and info["raw_tiles"] == 1
        assert all(torch.equal(a, b) for a, b in zip(out, ragged))
        # without corruption the two checks give the same file
        a = good.encode(ragged, max_ratio=math.inf)
        b = good.encode(ragged, max_ratio=math.inf, check="decode")
        assert a.to_bytes() == b.to_bytes() and not b.reasons.any()
    with pytest.raises(ValueError):
        good.encode(ragged, check="both")


# ------------------------------------------------------------------ 8. non-square tiles
def test_non_square_tile_model_round_trip(model12x8):
    from idfcodec.safe import SafeTiledBitstream
    imgs = [_noise(25, 9, 91).cuda(), _noise(12, 8, 92).cuda() % 4]
    sc = model12x8.tiled_safe(max_batch=4)
    assert sc.tile_hw == (12, 8) and sc.max_batch == 4 and model12x8.tiled_safe() is sc
    for ratio in (1.0, 3.0, math.inf):
        sbs = sc.encode(imgs, max_ratio=ratio)
        assert sbs.tile_counts() == [6, 1]
        out, info = sc.decode(SafeTiledBitstream.from_bytes(sbs.to_bytes(), device="cuda"))
        assert info["ok"] and info["tiles"] == 7
        assert info["raw_tiles"] == int(sbs.escaped.sum())
        assert all(torch.equal(a, b) for a, b in zip(out, imgs))
        crop, rinfo = sc.decode_region(sbs, 0, 11, 7, 2, 2)
        assert rinfo["ok"] and rinfo["tiles"] == 4
        assert torch.equal(crop, imgs[0][:, 11:13, 7:9])
