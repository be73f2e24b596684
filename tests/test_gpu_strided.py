"""Interleaved (HWC) and strided images in the tiled codecs, on the device: every strided kernel
against its planar sibling over the dense planar copy of the same pixels, scatters into views
carved out of one buffer of guard bytes, and every tiled codec end to end -- files byte for byte
those of the planar copies, decodes into HWC tensors, pitched canvases and windows.  Tiny models
only."""
import zlib

import numpy as np
import pytest
import torch

from test_gpu_predict import mixed, model_sharp  # noqa: F401  (fixtures)
from test_gpu_tiled import model12x8, model16  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0xAB
SHAPES = ("hwc", "hwc_pitch", "rgbx", "window", "flat")     # (a) .. (e)
WRITABLE = SHAPES[:4]
RAGGED = ((1, 1), (16, 16), (17, 16), (5, 40), (37, 21))
GEOMETRIES = {"ragged_16x16": (3, 16, 16, RAGGED),
              "two_blocks_40x33": (3, 40, 33, ((45, 70), (40, 33))),
              "c1_12x8": (1, 12, 8, ((1, 1), (12, 8), (13, 8), (5, 20), (29, 11)))}


def _images(C, sizes, seed=0):
    """uint8 [C, H, W] per size, with the quantiser's edge values in every image that has room"""
    rng = np.random.default_rng(seed)
    out = []
    for H, W in sizes:
        a = rng.integers(0, 256, (C, H, W), dtype=np.uint8)
        if a.size >= 4:
            a.reshape(-1)[:4] = (0, 127, 128, 255)
        out.append(torch.from_numpy(a))
    return out


def _carve(big, o, shape, strides):
    return big.as_strided(shape, strides, o)


def _views(kind, planar, fill=True):
    """The pixels of the planar images [C, H, W] in memory shape `kind`, all carved out of one
    buffer of guard bytes -> (the buffer, the tensors a codec takes, their layout, their
    [C, H, W] views).  fill=False: the addressed bytes stay guard bytes (a destination)."""
    specs, total = [], 64
    for t in planar:
        C, H, W = t.shape
        if kind == "hwc":            # (a) dense [H, W, C]
            shape, strides, off, span = (H, W, C), (W * C, C, 1), 0, H * W * C
        elif kind == "hwc_pitch":    # (b) rows of W*C + 5 bytes
            shape, strides, off, span = (H, W, C), (W * C + 5, C, 1), 0, H * (W * C + 5)
        elif kind == "rgbx":         # (c) four bytes a pixel, C of them addressed
            assert C == 3
            shape, strides, off, span = (H, W, C), (W * 4, 4, 1), 0, H * W * 4
        elif kind == "window":       # (d) inside a planar [C, H + 3, W + 5] image, at (2, 3)
            shape, strides = (C, H, W), ((H + 3) * (W + 5), W + 5, 1)
            off, span = 2 * (W + 5) + 3, C * (H + 3) * (W + 5)
        elif kind == "flat":         # (e) one plane read C times
            shape, strides, off, span = (C, H, W), (0, W, 1), 0, H * W
        else:
            raise AssertionError(kind)
        specs.append((shape, strides, total + off))
        total += span + 64
    big = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    tensors = [_carve(big, o, s, st) for s, st, o in specs]
    layout = "chw" if kind in ("window", "flat") else "hwc"
    views = [t if layout == "chw" else t.permute(2, 0, 1) for t in tensors]
    if fill:
        for v, t in zip(views, planar):
            (v[0] if kind == "flat" else v).copy_(t[0] if kind == "flat" else t)
    return big, tensors, layout, views


def _pixels(kind, planar):
    """What the views of `kind` hold: a flat source shows plane 0 in every channel"""
    return [t[:1].expand_as(t).contiguous() if kind == "flat" else t for t in planar]


def _synthetic(sizes, seed):
    from idfcodec import synthetic
    return [synthetic.images(1, 3, H, W, seed=seed + i)[0] for i, (H, W) in enumerate(sizes)]


def _guards_intact(big, views, want):
    """big is guard bytes everywhere but at the bytes the views address, which hold `want`"""
    ref = torch.full_like(big, GUARD)
    for v, w in zip(views, want):
        ref.as_strided(v.shape, v.stride(), v.storage_offset()).copy_(w.cuda())
    return torch.equal(big, ref)


def _table(views, th, tw, strided=True):
    from idfcodec.tiled import TileLayout, TiledCodec
    C = views[0].shape[0]
    lay = TileLayout([v.shape[1:] for v in views], C, (th, tw))
    strides = [tuple(v.stride()) for v in views] if strided else None
    rows = lay.rows([v.data_ptr() for v in views], strides)
    return lay, TiledCodec._device_table(rows, torch.device("cuda", 0))


class _Case:
    """One geometry: the planar images on the device, their five-field table and what the planar
    kernels give for it.  Computed once per geometry and shared, never modified."""

    def __init__(self, name):
        from idfcodec.safe import raw_offsets
        self.C, self.th, self.tw, self.sizes = GEOMETRIES[name]
        C, th, tw = self.C, self.th, self.tw
        self.host = _images(C, self.sizes, seed=len(name))
        self.dev = [t.cuda() for t in self.host]
        self.lay, self.table = _table(self.dev, th, tw, strided=False)
        assert self.table.shape[1] == 5
        self.flat = [t.cuda() for t in _pixels("flat", self.host)]
        _, self.flat_table = _table(self.flat, th, tw, strided=False)
        self.n = n = self.lay.n_tiles
        self.offs, self.n_raw = raw_offsets([True] * n, self.lay.rects, C)
        self.d_off = torch.tensor(self.offs, dtype=torch.int64, device="cuda")
        self.d_rect = torch.tensor(self.lay.rects, dtype=torch.int32, device="cuda")

    def gathered(self, table, fill=-7.0):
        from idfcodec.tiled import device_gather
        buf = torch.full((self.n * self.th * self.tw * 4,), fill, device="cuda")
        device_gather(table, self.n, self.C, self.th, self.tw, buf)
        return buf

    def planar_table(self, kind):
        """The five-field table over the dense planar copy of what views of `kind` hold"""
        return self.flat_table if kind == "flat" else self.table

    def raw(self, table):
        from idfcodec.safe import device_gather_raw
        out = torch.full((self.n_raw,), GUARD, dtype=torch.uint8, device="cuda")
        device_gather_raw(table, self.n, self.C, self.th, self.tw, self.d_off, out)
        return out


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Case(name)
    return _CASES[name]


def _kinds(name, kinds):
    """RGBX is a three-channel shape: the C = 1 geometry has no X to skip"""
    return [k for k in kinds if k != "rgbx" or GEOMETRIES[name][0] == 3]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_gather_equals_the_planar_gather(name):
    for kind in _kinds(name, SHAPES):
        c = _case(name)
        want = c.gathered(c.planar_table(kind)).view(c.n, c.th, c.tw, 4)
        big, _, _, views = _views(kind, c.host)
        _, stab = _table(views, c.th, c.tw)
        assert stab.shape == (c.n, 8), kind
        got = c.gathered(stab).view(c.n, c.th, c.tw, 4)
        assert torch.equal(got, want), kind                # bit-equal, the pad included
        assert bool((got[..., c.C:] == -7.0).all()), kind  # columns >= C are not written
        if kind != "flat":                                 # a source is only read
            assert _guards_intact(big, views, c.host), kind


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_scatter_and_raw_scatter_write_only_the_addressed_bytes(name):
    from idfcodec.safe import device_scatter_raw
    from idfcodec.tiled import device_scatter
    for kind in _kinds(name, WRITABLE):
        c = _case(name)
        buf, raw = c.gathered(c.table, 0.0), c.raw(c.table)
        big, _, _, views = _views(kind, c.host, fill=False)
        _, otab = _table(views, c.th, c.tw)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        device_scatter(otab, c.n, c.C, c.th, c.tw, buf, bad)
        assert int(bad.item()) == 0 and _guards_intact(big, views, c.host), kind
        big, _, _, views = _views(kind, c.host, fill=False)
        _, otab = _table(views, c.th, c.tw)
        device_scatter_raw(otab, c.n, c.C, c.th, c.tw, raw, c.d_off, c.d_rect)
        assert _guards_intact(big, views, c.host), kind


@pytest.mark.parametrize("kind", WRITABLE)
def test_scatters_of_a_crop_with_negative_origins(kind):
    """The decode_region case: rows [14, 19) x columns [13, 19) of the 37x21 image lie across
    tiles (0..1, 0..1), each clipped on two sides; the table rows have negative origins."""
    from idfcodec.safe import device_scatter_raw
    from idfcodec.tiled import device_scatter
    c = _case("ragged_16x16")
    i = RAGGED.index((37, 21))
    first = c.lay.first[i]
    y0, x0, h, w = 14, 13, 5, 6
    ent, rows = c.lay.region_rows(i, y0, x0, h, w)
    assert ent == [first, first + 1, first + 2, first + 3]
    crop = c.host[i][:, y0:y0 + h, x0:x0 + w].contiguous()
    buf, raw = c.gathered(c.table, 0.0), c.raw(c.table)
    px4 = c.th * c.tw * 4
    part = torch.cat([buf[e * px4:(e + 1) * px4] for e in ent])
    d_off = c.d_off[ent].contiguous()
    d_rect = c.d_rect[ent].contiguous()
    from idfcodec.tiled import TiledCodec
    for run in ("scatter", "raw"):
        big, _, _, views = _views(kind, [crop], fill=False)
        v = views[0]
        tab = TiledCodec._device_table(c.lay.place(rows, [v.data_ptr()], [v.stride()]),
                                       torch.device("cuda", 0))
        assert tab.shape == (4, 8) and int(tab[:, 3:5].min()) < 0
        if run == "scatter":
            bad = torch.zeros(1, dtype=torch.int32, device="cuda")
            device_scatter(tab, 4, c.C, c.th, c.tw, part, bad)
            assert int(bad.item()) == 0
        else:
            device_scatter_raw(tab, 4, c.C, c.th, c.tw, raw, d_off, d_rect)
        assert _guards_intact(big, views, [crop]), run


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_raw_gather_and_tile_crc_equal_the_planar_calls(name):
    from idfcodec.integrity import device_tile_crc32
    for kind in _kinds(name, SHAPES):
        c = _case(name)
        px = _pixels(kind, c.host)
        _, _, _, views = _views(kind, c.host)
        _, stab = _table(views, c.th, c.tw)
        got = c.raw(stab)
        assert torch.equal(got, c.raw(c.planar_table(kind))), kind
        crc = torch.empty(c.n, dtype=torch.int32, device="cuda")
        device_tile_crc32(stab, c.n, c.C, c.th, c.tw, crc)
        th, tw = c.th, c.tw
        want = [zlib.crc32(px[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w].contiguous()
                           .numpy().tobytes())
                for (i, ty, tx), (h, w) in zip(c.lay.entries, c.lay.rects)]
        assert crc.cpu().numpy().view(np.uint32).tolist() == want, kind


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_verify_counts_one_changed_byte_at_its_tile(name):
    from idfcodec.safe import device_verify
    for kind in _kinds(name, SHAPES):
        c = _case(name)
        buf = c.gathered(c.planar_table(kind), 0.0)
        _, _, _, views = _views(kind, c.host)
        _, stab = _table(views, c.th, c.tw)
        mism = torch.zeros(c.n, dtype=torch.int32, device="cuda")
        device_verify(stab, c.n, c.C, c.th, c.tw, buf, mism)
        assert int(mism.abs().sum()) == 0, kind
        # the last image's last pixel, channel C - 1: in the last tile
        v = views[-1]
        v[c.C - 1, -1, -1] ^= 0x40
        device_verify(stab, c.n, c.C, c.th, c.tw, buf, mism)
        want = [0] * (c.n - 1) + [c.C if kind == "flat" else 1]    # one plane, read C times
        assert mism.tolist() == want, kind


# ------------------------------------------------------------------ 2. the codecs, end to end
CODECS = ("tiled", "tiled_ways8", "safe", "predict", "colour", "predict_ways8", "sealed",
          "sealed_tiled")
E2E_SHAPES = ("hwc", "hwc_pitch", "window")                  # (a), (b), (d)


def _codec(model, which):
    return {"tiled": lambda: model.tiled(), "tiled_ways8": lambda: model.tiled(ways=8),
            "safe": lambda: model.tiled_safe(), "predict": lambda: model.tiled_safe(predict=True),
            "colour": lambda: model.tiled_safe(predict="colour"),
            "predict_ways8": lambda: model.tiled_safe(predict=True, predict_ways=8),
            "sealed": lambda: model.tiled_sealed(),
            "sealed_tiled": lambda: model.tiled_sealed(safe=False)}[which]()


@pytest.mark.parametrize("which", CODECS)
def test_files_are_those_of_the_planar_copies(model_sharp, mixed, which):  # noqa: F811
    codec = _codec(model_sharp, which)
    host = [t.cpu() for t in mixed]
    ref = codec.encode(mixed)
    want = ref.to_bytes()
    if which in ("predict", "colour", "predict_ways8"):
        # the flow, the packed and the raw paths all run
        assert ref.n_kept > 0 and ref.n_packed > 0 and ref.stored_raw.any()
    if which == "safe":
        assert ref.n_kept > 0 and ref.escaped.any()
    for kind in E2E_SHAPES:
        big, tensors, layout, views = _views(kind, host)
        bs = codec.encode(tensors, layout=layout)
        assert bs.to_bytes() == want, kind
        assert _guards_intact(big, views, host), kind     # a source is only read
        # decode(layout="hwc"): dense [H, W, C] tensors of the sources' pixels
        outs, info = codec.decode(bs, layout="hwc")
        assert info["ok"], kind
        for o, t in zip(outs, host):
            assert o.is_contiguous() and tuple(o.shape) == (*t.shape[1:], 3)
            assert torch.equal(o.cpu(), t.permute(1, 2, 0)), kind
        # decode(out=...): into guarded canvases of the same memory shape
        big, tensors, layout, views = _views(kind, host, fill=False)
        outs, info = codec.decode(bs, layout=layout, out=tensors)
        assert info["ok"] and all(a is b for a, b in zip(outs, tensors)), kind
        assert _guards_intact(big, views, host), kind
    if which == "safe":     # the strided verify inside a codec
        big, tensors, layout, views = _views("hwc_pitch", host)
        checked = codec.encode(tensors, check="decode", layout=layout)
        assert checked.to_bytes() == codec.encode(mixed, check="decode").to_bytes()
        assert checked.n_kept > 0


@pytest.mark.parametrize("which", CODECS)
def test_region_into_a_window_of_a_canvas(model_sharp, mixed, which):  # noqa: F811
    codec = _codec(model_sharp, which)
    bs = codec.encode(mixed)
    y0, x0, h, w = 10, 9, 15, 30                # all six tiles of image 0, each clipped
    want = mixed[0][:, y0:y0 + h, x0:x0 + w].cpu()
    crop, info = codec.decode_region(bs, 0, y0, x0, h, w, layout="hwc")
    assert info["ok"] and info["tiles"] == 6
    assert crop.is_contiguous() and torch.equal(crop.cpu(), want.permute(1, 2, 0))
    for kind in ("hwc_pitch", "window"):
        big, (t,), layout, views = _views(kind, [want], fill=False)
        out, info = codec.decode_region(bs, 0, y0, x0, h, w, layout=layout, out=t)
        assert out is t and info["ok"] and info["tiles"] == 6, kind
        assert _guards_intact(big, views, [want]), kind
    canvas = torch.full((40, 64, 3), GUARD, dtype=torch.uint8, device="cuda")
    out, info = codec.decode_region(bs, 0, y0, x0, h, w, layout="hwc",
                                    out=canvas[7:7 + h, 20:20 + w])
    ref = torch.full_like(canvas, GUARD)
    ref[7:7 + h, 20:20 + w] = want.permute(1, 2, 0).cuda()
    assert info["ok"] and torch.equal(canvas, ref)


def test_outputs_are_checked_before_any_launch(model16):  # noqa: F811
    tc = model16.tiled()
    img = _images(3, [(17, 16)])[0].cuda()
    bs = tc.encode([img])
    flat = torch.zeros((17, 16), dtype=torch.uint8, device="cuda").expand(3, 17, 16)
    for out, msg in (([flat], "twice"), ([torch.empty_like(img), torch.empty_like(img)], "holds"),
                     ([torch.empty((3, 17, 17), dtype=torch.uint8, device="cuda")], "shape"),
                     ([torch.empty_like(img).float()], "uint8"), ([torch.empty_like(img).cpu()],
                                                                  "lies on")):
        with pytest.raises(ValueError, match=msg):
            tc.decode(bs, out=out)
    with pytest.raises(ValueError, match="shape"):
        tc.decode(bs, out=[torch.empty_like(img)], layout="hwc")
    with pytest.raises(ValueError, match="layout"):
        tc.encode([img], layout="nhwc")


def test_a_slice_of_a_larger_hwc_batch(model16):  # noqa: F811
    tc = model16.tiled()
    rng = np.random.default_rng(9)
    batch = torch.from_numpy(rng.integers(0, 256, (5, 21, 19, 3), dtype=np.uint8)).cuda()
    part = batch[1::2, 2:, :17]                     # [2, 19, 17, 3], no dimension dense
    assert not part.is_contiguous()
    planar = part.permute(0, 3, 1, 2).contiguous()
    want = tc.encode(planar).to_bytes()
    assert tc.encode(part, layout="hwc").to_bytes() == want
    assert tc.encode(part.permute(0, 3, 1, 2), layout="chw").to_bytes() == want  # a permuted view
    with pytest.raises(ValueError, match="not contiguous"):     # no layout named: as before
        tc.encode(part.permute(0, 3, 1, 2))
    outs, info = tc.decode(tc.encode(part, layout="hwc"), layout="hwc")
    assert info["ok"] and all(torch.equal(o, p) for o, p in zip(outs, part))


def test_a_gray_plane_expanded_over_the_channels(model16):  # noqa: F811
    tc = model16.tiled()
    gray = _images(1, [(17, 23)], seed=4)[0].cuda()[0]
    flat = gray.expand(3, 17, 23)
    assert flat.stride(0) == 0
    assert tc.encode([flat], layout="chw").to_bytes() == tc.encode([flat.contiguous()]).to_bytes()
    with pytest.raises(ValueError, match="not contiguous"):     # no layout named: as before
        tc.encode([flat])


def test_a_non_square_tile_model_codes_hwc(model12x8):  # noqa: F811
    tc = model12x8.tiled()
    host = _synthetic(GEOMETRIES["c1_12x8"][3], 30)
    want = tc.encode([t.cuda() for t in host]).to_bytes()
    for kind in ("hwc", "hwc_pitch", "window"):
        big, tensors, layout, views = _views(kind, host)
        bs = tc.encode(tensors, layout=layout)
        assert bs.to_bytes() == want, kind
        big, tensors, layout, views = _views(kind, host, fill=False)
        _, info = tc.decode(bs, layout=layout, out=tensors)
        assert info["ok"] and _guards_intact(big, views, host), kind


def test_sealed_hwc_decode_names_the_damaged_tile(model16):  # noqa: F811
    """test_gpu_integrity's corruption: entry 7, level 0, word offset + 2, ^ 0x00010000."""
    import math
    from idfcodec.integrity import SealedBitstream
    from idfcodec.tiled import tiles_host
    zc = model16.tiled_sealed()
    host = _synthetic(RAGGED, 70)                # test_gpu_integrity's ragged set
    _, tensors, layout, _ = _views("hwc_pitch", host)
    zbs = SealedBitstream.from_bytes(zc.encode(tensors, max_ratio=math.inf,
                                               layout=layout).to_bytes(), device="cuda")
    assert not zbs.inner.escaped.any()
    k = 7
    s = zbs.inner.stream
    assert int(s.nwords_host()[k]) > 4
    at = int(s.word_offsets()[k].item()) + 2
    s.words[at] = s.words[at] ^ 0x00010000
    planar, pinfo = zc.decode(zbs)
    outs, info = zc.decode(zbs, layout="hwc")
    assert info["crc_bad"] == pinfo["crc_bad"] == [k] and info["ok"] is False
    assert all(torch.equal(o, p.permute(1, 2, 0)) for o, p in zip(outs, planar))
    assert all(torch.equal(o.cpu(), t.permute(1, 2, 0)) for o, t in zip(outs[:4], host[:4]))
    got = outs[4].permute(2, 0, 1).cpu().numpy()
    same = [np.array_equal(a, b) for a, b in zip(tiles_host(got, 16, 16),
                                                 tiles_host(host[4].numpy(), 16, 16))]
    assert same == [False] + [True] * 5         # the sound tiles are correct in the HWC output
