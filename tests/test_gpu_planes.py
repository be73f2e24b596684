"""Plane sets on the device: the two byte-run kernels against numpy at every alignment and inside
sentinel bytes, and model.tiled_planes end to end -- RGBA read where it lies, grey and grey +
alpha without a flow, two extra planes over each kind of base, N-way streams, the caller's
strided outputs, crops, subsets, a damaged unit, and bytes that depend on neither chunking nor
company nor the source's layout.  The 16x16-tile, C = 3 tiny model only."""
import functools
import struct

import numpy as np
import pytest
import torch

import predict_ref as ref
from test_gpu_safe import GUARD, _guarded, _guards_intact, _noise, _tiny_model

pytestmark = pytest.mark.gpu

L = 1 << 32
LENS = [0, 1, 2, 3, 15, 16, 17, 31, 33, 255, 256, 4099]
SIZES = [(16, 16), (17, 33), (1, 1), (40, 5)]       # 1 + 6 + 1 + 3 tiles of 16x16
ALPHAS = ["noise", "step", "const", "ramp"]         # image i's alpha


@pytest.fixture(scope="module")
def model16():
    return _tiny_model(2, 2, 16, 16, 3, 2).cuda()


@pytest.fixture(scope="module")
def model_sharp():
    """test_gpu_safe's: the same model with every prior's logscale lowered by 3.0, so dark tiles
    are kept and noise tiles escape."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            b["prior"].NN.layers[-1].bias[b["prior"].out_channel:] -= 3.0
    return m.cuda()


# ------------------------------------------------------------------ 1. the byte-run kernels
@functools.lru_cache(maxsize=None)
def _segments():
    """Every length of LENS starting at every alignment 0..15 of one buffer: (starts, lengths,
    which of them are the wanted ones).  In front of each wanted run lies a pad run of 16..31
    bytes that brings its start to the alignment; the runs are adjacent, pads included."""
    starts, lens, wanted, o = [], [], [], 0
    for a in range(16):
        for n in LENS:
            pad = 16 + (a - (o + 16)) % 16
            starts += [o, o + pad]
            lens += [pad, n]
            wanted += [False, True]
            o += pad + n
            assert (o - n) % 16 == a
    return np.array(starts), np.array(lens), np.array(wanted)


@pytest.mark.parametrize("mark", ["none", "first", "last"])
def test_segment_range_equals_numpy_at_every_alignment(mark):
    """Neighbouring runs hold 0 and 255, so a byte read past a run's ends changes its range;
    mark: the other extreme once, at the run's first or last byte, so a dropped head or tail
    changes it too."""
    from idfcodec.planes import device_segment_range
    starts, lens, _ = _segments()
    n = len(starts)
    off = np.append(starts, starts[-1] + lens[-1])
    host = np.empty(off[-1], dtype=np.uint8)
    for k in range(n):
        seg = host[off[k]:off[k + 1]]
        seg[:] = 255 * (k % 2)
        if mark != "none" and len(seg):
            seg[0 if mark == "first" else -1] = 255 * (1 - k % 2)
    want = np.array([(host[a:b].min(), host[a:b].max()) if b > a else (255, 0)
                     for a, b in zip(off[:-1], off[1:])], dtype=np.uint8)
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    got = device_segment_range(torch.from_numpy(off).cuda(), n, src).cpu().numpy()
    assert np.array_equal(got, want)
    if mark != "none":      # every run of two bytes or more spans both extremes
        assert (want[lens >= 2] == (0, 255)).all()
    # a buffer that ends with its last run, at every alignment of that end: nothing behind it
    for tail in (1, 15, 16, 17, 4099):
        t = src[:int(off[3]) + tail]
        o2 = torch.tensor([0, int(off[3]), int(off[3]) + tail], dtype=torch.int64, device="cuda")
        got = device_segment_range(o2, 2, t.clone()).cpu().numpy()
        h = host[:int(off[3]) + tail]
        assert got.tolist() == [[h[:off[3]].min(), h[:off[3]].max()],
                                [h[off[3]:].min(), h[off[3]:].max()]]
    assert device_segment_range(torch.zeros(1, dtype=torch.int64, device="cuda"), 0,
                                src).shape == (0, 2)


def test_segment_fill_writes_its_runs_and_nothing_else():
    from idfcodec.planes import device_segment_fill
    starts, lens, wanted = _segments()
    starts, lens = starts[wanted], lens[wanted]       # the pads in front of them stay sentinel
    n = len(starts)
    values = (np.arange(n) % 170 + 1).astype(np.uint8)      # never the sentinel 0xAB = 171
    total = int(starts[-1] + lens[-1]) + 64
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    # handed over in reverse: the order of the runs is the caller's
    order = np.arange(n)[::-1].copy()
    device_segment_fill(torch.from_numpy(starts[order]).cuda(),
                        torch.from_numpy(lens[order]).cuda(),
                        torch.from_numpy(values[order]).cuda(), n, dst)
    want = np.full(total, GUARD, dtype=np.uint8)
    for s, m, v in zip(starts, lens, values):
        want[s:s + m] = v
    assert np.array_equal(dst.cpu().numpy(), want)
    # a negative length writes nothing
    dst.fill_(GUARD)
    device_segment_fill(torch.tensor([32], device="cuda"), torch.tensor([-5], device="cuda"),
                        torch.tensor([7], dtype=torch.uint8, device="cuda"), 1, dst)
    assert bool((dst == GUARD).all())


# ------------------------------------------------------------------ 2. sources and the reference
def _alpha(kind, H, W, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "const":
        a = np.full((H, W), 255)
    elif kind == "step":
        a = np.where(xx >= (3 * W) // 5, 255, 0)
    elif kind == "ramp":
        a = (3 * yy + 2 * xx + 11) % 256
    else:
        a = np.random.default_rng(900 + seed).integers(0, 256, (H, W))
    return torch.from_numpy(a.astype(np.uint8))


def _with_planes(rgb, extra):
    """[3, H, W] and a list of [H, W] planes -> planar [3 + len, H, W] on the device"""
    return torch.cat([rgb] + [e[None] for e in extra]).contiguous().cuda()


@pytest.fixture(scope="module")
def rgba():
    """SIZES as dense [H, W, 4] tensors: noise RGB; alpha noise, a 0 / 255 step, constant 255
    and a ramp."""
    return [_with_planes(_noise(H, W, 300 + i), [_alpha(k, H, W, i)]).permute(1, 2, 0).contiguous()
            for i, ((H, W), k) in enumerate(zip(SIZES, ALPHAS))]


def _units(imgs_chw, Cb, lay):
    """The extra planes' units of planar images as numpy [1, hin, win], unit order."""
    th, tw = lay.tile_hw
    Cs = imgs_chw[0].shape[0]
    return [imgs_chw[i][p:p + 1, ty * th:ty * th + h, tx * tw:tx * tw + w].cpu().numpy()
            for (i, ty, tx), (h, w) in zip(lay.entries, lay.rects) for p in range(Cb, Cs)]


def _reference(units, ways=1):
    """What the numpy restatement and the C oracle make of the units: (classes, sel, states,
    nwords, [words]) with the last four over the units that are not constant."""
    import rans_oracle
    from idfcodec import planes
    assert ways == 1
    const = np.array([u.min() == u.max() for u in units])
    coded = [u for u, c in zip(units, const) if not c]
    sel = np.array([ref.choose_sel(u) for u in coded], dtype=np.uint32)
    off = np.zeros(len(coded) + 1, dtype=np.int64)
    np.cumsum([u.size for u in coded], out=off[1:])
    nw = np.zeros(0, dtype=np.int64)
    states, words = np.zeros(0, dtype=np.uint64), []
    if coded:
        arrs = [ref.arrays(u, int(s)) for u, s in zip(coded, sel)]
        x, mean, scale = (np.concatenate([a[i] for a in arrs]) for i in range(3))
        states, w, nw, status = rans_oracle.encode_streams(off, x, mean, scale)
        assert not status.any()
        words = [w[a:a + m] for a, m in zip(off[:-1], nw)]
    nb = np.array([u.size for u in units])
    cls = np.full(len(units), planes.CLASS_CONSTANT, dtype=np.uint8)
    cls[~const] = planes.unit_class(np.zeros(len(coded)), np.ones(len(coded)),
                                    np.zeros(len(coded)), nw, nb[~const], 1)
    return cls, sel, states, nw, words


def _assert_packed_equals_reference(bs, units):
    from idfcodec import planes
    cls, sel, states, nw, words = _reference(units)
    assert np.array_equal(bs.classes, cls)
    pk = cls[cls != planes.CLASS_CONSTANT] == planes.CLASS_PACKED
    assert np.array_equal(bs.sel, sel[pk]) and np.array_equal(bs.nwords, nw[pk])
    assert np.array_equal(np.asarray(bs.states, dtype=np.uint64), states[pk])
    want = [w for w, p in zip(words, pk) if p]
    want = np.concatenate(want) if want else np.zeros(0, np.uint32)
    assert np.array_equal(bs.words.cpu().numpy().view(np.uint32), want)
    return cls, nw[pk]


def _same(outs, imgs):
    return len(outs) == len(imgs) and all(torch.equal(a, b) for a, b in zip(outs, imgs))


# ------------------------------------------------------------------ 3. RGBA
def test_rgba_round_trips_and_costs_what_the_layout_says(model16, rgba):
    from idfcodec import planes
    from idfcodec.tiled import planes as chw
    pc = model16.tiled_planes(4)
    base = model16.tiled_safe(predict=True)
    assert pc.base is base and (pc.Cb, pc.Ce) == (3, 1)
    bs = pc.encode(rgba, layout="hwc")
    buf = bs.to_bytes()
    got = planes.PlaneSetBitstream.from_bytes(buf, device="cuda")
    outs, info = pc.decode(got, layout="hwc")
    assert info["ok"] and _same(outs, rgba) and all(o.is_contiguous() for o in outs)
    assert info["tiles"] == 11
    # the base section is the base codec's file of the RGB views, read in place
    want = base.encode([chw(t, "hwc")[:3] for t in rgba], layout="chw").to_bytes()
    n_hdr = 28 + 8 * 4
    assert struct.unpack_from("<Q", buf, n_hdr)[0] == len(want)
    assert buf[n_hdr + 8:n_hdr + 8 + len(want)] == want
    # the classes, the packed units' streams and with them the file's length from the reference
    units = _units([chw(t, "hwc") for t in rgba], 3, bs.layout)
    assert len(units) == 11
    cls, nw = _assert_packed_equals_reference(bs, units)
    nb = np.array([u.size for u in units])
    K, n_raw = int((cls == planes.CLASS_CONSTANT).sum()), int(nb[cls == planes.CLASS_RAW].sum())
    # 11 units: a constant bitmap of 2 bytes; a constant costs its bit there and one byte
    assert len(buf) == (n_hdr + 8 + len(want) + 2 + -(-(11 - K) // 8) + K + 8 + n_raw
                        + 8 + 4 + 16 * len(nw) + 4 * int(nw.sum()))
    assert len(buf) == n_hdr + 8 + len(want) + planes.plane_section_bytes(11, K, n_raw, nw)
    assert len(bs.values) == K and bs.values.tolist() == [int(u.flat[0]) for u, c in
                                                         zip(units, cls) if c == 0]
    # image 0's alpha is noise: raw; image 2 is one opaque pixel; the step image has tiles of
    # 0 alone and of 255 alone, and two that hold the step
    assert cls[0] == planes.CLASS_RAW and cls[7] == planes.CLASS_CONSTANT
    assert K >= 4 and set(bs.values.tolist()) == {0, 255}
    assert (info["constant_planes"], info["raw_planes"]) == (K, int((cls == 2).sum()))
    assert info["packed_planes"] == len(nw) and K + len(nw) + info["raw_planes"] == 11
    assert len(bs.plane_section()) <= planes.plane_section_bound(SIZES, 1, 16, 16)
    assert bs.n_subpixels() == 4 * sum(H * W for H, W in SIZES)
    assert bs.bits() == bs.base.bits() + bs.plane_bits()


def test_the_parent_interface_refuses_rgba_and_tiled_planes_codes_it(model16, rgba):
    """What the tiled codecs did with four channels before plane sets, and still do."""
    with pytest.raises(ValueError, match="4 channels, the model 3"):
        model16.tiled_safe(predict=True).encode(rgba, layout="hwc")
    pc = model16.tiled_planes(4)
    outs, info = pc.decode(pc.encode(rgba, layout="hwc"), layout="hwc")
    assert info["ok"] and _same(outs, rgba)


# ------------------------------------------------------------------ 4. grey, grey + alpha
@pytest.mark.parametrize("Cs", [1, 2])
def test_grey_sources_run_no_flow_and_equal_the_reference(model16, Cs):
    from idfcodec import planes
    kinds = ["ramp", "noise", "step", "const"]
    imgs = [torch.stack([_alpha(kinds[(i + p) % 4], H, W, 10 * i + p) for p in range(Cs)]).cuda()
            for i, (H, W) in enumerate([(37, 21), (16, 16), (17, 33), (5, 40)])]
    pc = model16.tiled_planes(Cs)
    assert (pc.Cb, pc.Ce) == (0, Cs)
    bs = pc.encode(imgs)
    assert bs.base is None and bs.n_units == Cs * (6 + 1 + 6 + 3)
    buf = bs.to_bytes()
    n_hdr = 28 + 8 * 4
    assert struct.unpack_from("<Q", buf, n_hdr)[0] == 0          # no base section
    assert len(buf) == n_hdr + 8 + len(bs.plane_section())
    outs, info = pc.decode(planes.PlaneSetBitstream.from_bytes(buf, device="cuda"))
    assert info["ok"] and _same(outs, imgs)
    assert info["flow_tiles"] == 0 and info["final_states"].numel() == 0 and info["tiles"] == 16
    cls, nw = _assert_packed_equals_reference(bs, _units(imgs, 0, bs.layout))
    assert {0, 1, 2} <= set(cls.tolist()) and len(nw) >= 4
    assert len(bs.plane_section()) <= planes.plane_section_bound(bs.sizes, Cs, 16, 16)
    with pytest.raises(ValueError, match="no base"):
        pc.encode(imgs, max_ratio=2.0)
    with pytest.raises(ValueError, match=f"3 channels, the model {Cs}"):
        pc.encode([_noise(16, 16, 1).cuda()])


# ------------------------------------------------------------------ 5. two extra planes, every base
@pytest.mark.parametrize("kind", ["tiled", "safe", "colour"])
def test_five_channels_over_each_kind_of_base(model16, kind):
    from idfcodec import planes
    base = {"tiled": model16.tiled, "safe": model16.tiled_safe,
            "colour": lambda: model16.tiled_safe(predict="colour")}[kind]()
    imgs = [_with_planes(_noise(H, W, 400 + i), [_alpha("ramp", H, W), _alpha("step", H, W)])
            for i, (H, W) in enumerate(SIZES)]
    pc = model16.tiled_planes(5, base=base)
    assert pc.base is base and (pc.Cb, pc.Ce) == (3, 2)
    bs = pc.encode(imgs)
    buf = bs.to_bytes()
    assert bs.base.to_bytes() == base.encode([t[:3] for t in imgs], layout="chw").to_bytes()
    outs, info = pc.decode(planes.PlaneSetBitstream.from_bytes(buf, device="cuda"))
    assert info["ok"] and _same(outs, imgs)
    assert info["constant_planes"] + info["packed_planes"] + info["raw_planes"] == 22
    # a file of another kind of base is refused by name, not misread
    other = model16.tiled_planes(5, base=model16.tiled_safe() if kind != "safe" else
                                 model16.tiled())
    with pytest.raises(ValueError, match="base"):
        other.decode(bs)


# ------------------------------------------------------------------ 6. N-way streams
def test_eight_ways_decode_to_the_one_way_bytes(model16, rgba):
    from idfcodec import planes
    one = model16.tiled_planes(4)
    pc = model16.tiled_planes(4, predict_ways=8)
    src = [t.clone() for t in rgba]
    src[0][..., 3] = _alpha("ramp", 16, 16).cuda()   # a full tile that packs at 8 states too
    bs = pc.encode(src, layout="hwc")
    buf = bs.to_bytes()
    assert struct.unpack_from("<H", buf, 6)[0] == 8 and bs.predict_ways == 8
    assert struct.unpack_from("<H", one.encode(src, layout="hwc").to_bytes(), 6)[0] == 0
    assert bs.n_packed >= 1 and bs.states.shape == (bs.n_packed, 8)
    got = planes.PlaneSetBitstream.from_bytes(buf, device="cuda")
    outs, info = one.decode(got, layout="hwc")      # decode follows the file's own N
    assert info["ok"] and _same(outs, src) and info["packed_planes"] == bs.n_packed
    outs1, _ = one.decode(one.encode(src, layout="hwc"), layout="hwc")
    assert _same(outs, outs1)


# ------------------------------------------------------------------ 7. the caller's outputs
def test_decode_into_an_rgba_window_of_a_wider_pixel(model16, rgba):
    pc = model16.tiled_planes(4)
    bs = pc.encode(rgba, layout="hwc")
    big, wide = _guarded([(H, W, 8) for H, W in SIZES])
    outs, info = pc.decode(bs, layout="hwc", out=[v[:, :, 2:6] for v in wide])
    assert info["ok"] and _same(outs, rgba)
    want = []
    for v, t in zip(wide, rgba):
        w = torch.full_like(v, GUARD)
        w[:, :, 2:6] = t
        want.append(w)
    assert _guards_intact(big, wide, want)


def test_decode_into_a_row_pitched_output(model16, rgba):
    from idfcodec.tiled import planes as chw
    pc = model16.tiled_planes(4)
    bs = pc.encode(rgba, layout="hwc")
    big, pitched = _guarded([(4, H, W + 7) for H, W in SIZES])
    outs, info = pc.decode(bs, out=[v[:, :, :W] for v, (H, W) in zip(pitched, SIZES)])
    assert info["ok"] and _same(outs, [chw(t, "hwc") for t in rgba])
    want = []
    for v, t, (H, W) in zip(pitched, rgba, SIZES):
        w = torch.full_like(v, GUARD)
        w[:, :, :W] = chw(t, "hwc")
        want.append(w)
    assert _guards_intact(big, pitched, want)


# ------------------------------------------------------------------ 8. regions and subsets
@pytest.fixture(scope="module")
def patchwork():
    """A 32x48 RGBA image of six tiles: RGB dark (bytes 0..3), noise, dark / noise, dark, noise;
    alpha constant, a ramp, noise / noise, constant, a ramp."""
    dark = lambda s: _noise(16, 16, s) % 4  # noqa: E731
    rgb = torch.cat([torch.cat([dark(80), _noise(16, 16, 81), dark(82)], dim=2),
                     torch.cat([_noise(16, 16, 83), dark(84), _noise(16, 16, 85)], dim=2)], dim=1)
    a = torch.cat([torch.cat([_alpha("const", 16, 16), _alpha("ramp", 16, 16),
                              _alpha("noise", 16, 16, 1)], dim=1),
                   torch.cat([_alpha("noise", 16, 16, 2), _alpha("const", 16, 16) // 5,
                              _alpha("ramp", 16, 16)], dim=1)], dim=0)
    return _with_planes(rgb, [a])


def test_region_over_every_class_of_unit_and_tile(model_sharp, patchwork):
    from idfcodec import planes
    pc = model_sharp.tiled_planes(4)
    bs = pc.encode([patchwork, patchwork[:, :17, :20].contiguous()])
    assert bs.classes[:6].tolist() == [0, 1, 2, 2, 0, 1]
    assert not bs.base.escaped[:6].all() and bs.base.escaped[:6].any()   # kept and escaped
    y0, x0, h, w = 10, 9, 15, 30            # all six tiles, each clipped
    crop, info = pc.decode_region(bs, 0, y0, x0, h, w)
    assert info["ok"] and info["tiles"] == 6
    assert (info["constant_planes"], info["packed_planes"], info["raw_planes"]) == (2, 2, 2)
    assert info["flow_tiles"] == int((~bs.base.escaped[:6]).sum())
    assert torch.equal(crop, patchwork[:, y0:y0 + h, x0:x0 + w])
    # inside one tile: one unit, and into an interleaved output of the caller's
    big, (out,) = _guarded([(9, 11, 4)])
    crop, info = pc.decode_region(bs, 0, 3, 18, 9, 11, layout="hwc", out=out)
    assert info["ok"] and info["tiles"] == 1 and info["packed_planes"] == 1
    assert info["constant_planes"] == info["raw_planes"] == 0
    want = patchwork[:, 3:12, 18:29].permute(1, 2, 0)
    assert crop is out and torch.equal(crop, want) and _guards_intact(big, [out], [want])
    with pytest.raises(ValueError, match="not inside"):
        pc.decode_region(bs, 1, 0, 0, 18, 20)
    assert isinstance(bs, planes.PlaneSetBitstream)


def test_a_subset_comes_in_the_order_asked(model16, rgba):
    pc = model16.tiled_planes(4)
    bs = pc.encode(rgba, layout="hwc")
    outs, info = pc.decode(bs, images=[2, 0], layout="hwc")
    assert info["ok"] and _same(outs, [rgba[2], rgba[0]])
    assert info["tiles"] == 2 and info["constant_planes"] == 1 and info["raw_planes"] == 1


# ------------------------------------------------------------------ 9. damage and determinism
def test_a_flipped_word_is_reported_for_its_unit_alone(model16):
    imgs = [_with_planes(_noise(32, 32, 500), [_alpha("ramp", 32, 32)]),
            _with_planes(_noise(16, 16, 501), [_alpha("ramp", 16, 16)])]
    pc = model16.tiled_planes(4)
    bs = pc.encode(imgs)
    assert bs.packed.all() and int(bs.nwords.min()) >= 4
    hit = 2                                       # the unit: image 0's tile (1, 0)
    bs.words = bs.words.clone()
    bs.words[int(bs.nwords[:hit].sum()) + 2] ^= 0x00010000
    outs, info = pc.decode(bs)
    assert not info["ok"] and info["damaged_planes"] == [hit]
    assert info["plane_units"].tolist() == [0, 1, 2, 3, 4]
    assert torch.equal(outs[1], imgs[1]) and torch.equal(outs[0][:3], imgs[0][:3])
    keep = torch.ones(32, 32, dtype=torch.bool, device="cuda")
    keep[16:, :16] = False
    assert torch.equal(outs[0][3][keep], imgs[0][3][keep])
    # without verify nothing is looked at
    assert "ok" not in pc.decode(bs, verify=False)[1]


def test_bytes_depend_on_neither_max_batch_nor_company_nor_layout(model16, rgba):
    a = model16.tiled_planes(4, max_batch=2).encode(rgba, layout="hwc").to_bytes()
    b = model16.tiled_planes(4, max_batch=256).encode(rgba, layout="hwc").to_bytes()
    assert a == b
    planar = [t.permute(2, 0, 1).contiguous() for t in rgba]
    pc = model16.tiled_planes(4)
    assert pc.encode(planar).to_bytes() == b
    assert pc.encode(planar, layout="chw").to_bytes() == b
    whole = pc.encode(rgba, layout="hwc")
    alone = pc.encode([rgba[1]], layout="hwc")      # the step image: tiles 1..6 of the set
    assert alone.classes.tolist() == whole.classes[1:7].tolist()
    k0, p0 = int(whole.constant[:1].sum()), int(whole.packed[:1].sum())
    K, P = alone.n_constant, alone.n_packed
    assert alone.values.tolist() == whole.values[k0:k0 + K].tolist() and P >= 1
    assert np.array_equal(alone.sel, whole.sel[p0:p0 + P])
    assert np.array_equal(alone.states, whole.states[p0:p0 + P])
    assert np.array_equal(alone.nwords, whole.nwords[p0:p0 + P])
    w0 = int(whole.nwords[:p0].sum())
    assert torch.equal(alone.words.cpu(), whole.words[w0:w0 + int(alone.nwords.sum())].cpu())
    r0 = 256                                        # image 0's raw alpha tile comes first
    assert torch.equal(alone.raw.cpu(), whole.raw[r0:r0 + alone.raw.numel()].cpu())
    assert alone.base.to_bytes() == pc.base.encode(
        [rgba[1].permute(2, 0, 1)[:3]], layout="chw").to_bytes()
