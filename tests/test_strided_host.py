"""Interleaved and strided images in the tiled codecs, on the host: table rows with strides, the
checks of sources and outputs in both layouts, the declared and bound entry points, and the file
tool's as-stored reader and layout-aware writer.  No device."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

CPU = torch.device("cpu")
STRIDED = ("idf_tile_gather_strided_u8", "idf_tile_scatter_strided_u8",
           "idf_tile_gather_raw_strided_u8", "idf_tile_scatter_raw_strided_u8",
           "idf_tile_verify_strided_u8", "idf_tile_crc32_strided_u8")


def _u8(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.int64).remainder(251).to(
        torch.uint8).reshape(*shape)


# ------------------------------------------------------------------ table rows
def test_place_appends_the_strides_of_the_right_image():
    from idfcodec.tiled import TileLayout
    lay = TileLayout([(17, 16), (5, 40)], 3, (16, 16))
    want, entries, rows = lay.image_rows([1, 0])
    assert entries == [2, 3, 4, 0, 1]
    addrs, strides = [1000, 2000], [(1, 120, 3), (400, 21, 1)]
    five = lay.place(rows, addrs)
    assert five == [(1000, 5, 40, 0, 0), (1000, 5, 40, 0, 16), (1000, 5, 40, 0, 32),
                    (2000, 17, 16, 0, 0), (2000, 17, 16, 16, 0)]
    eight = lay.place(rows, addrs, strides)
    assert eight == [r + strides[0] for r in five[:3]] + [r + strides[1] for r in five[3:]]
    assert lay.place(rows, addrs, strides=None) == five
    assert lay.rows([7, 9]) == lay.place(lay.image_rows()[2], [7, 9])
    assert all(len(r) == 5 for r in lay.rows([7, 9]))
    assert lay.rows([7, 9], [(0, 16, 1), (1, 160, 4)])[2:] == [
        (9, 5, 40, 0, 0, 1, 160, 4), (9, 5, 40, 0, 16, 1, 160, 4), (9, 5, 40, 0, 32, 1, 160, 4)]
    # a region: negative origins keep their place in front of the strides
    ent, rows = lay.region_rows(0, 14, 3, 3, 5)
    assert lay.place(rows, [50], [(1, 15, 3)]) == [(50, 3, 5, -14, -3, 1, 15, 3),
                                                   (50, 3, 5, 2, -3, 1, 15, 3)]


def test_view_strides_is_none_only_for_dense_planar_views():
    from idfcodec.tiled import is_dense_planar, planes, view_strides
    dense = _u8(3, 5, 7)
    assert is_dense_planar(dense) and view_strides([dense, _u8(3, 2, 2)]) is None
    hwc = planes(_u8(5, 7, 3), "hwc")
    assert tuple(hwc.shape) == (3, 5, 7) and not is_dense_planar(hwc)
    assert view_strides([dense, hwc]) == [(35, 7, 1), (1, 21, 3)]
    window = _u8(3, 9, 12)[:, 2:7, 3:10]
    assert view_strides([window]) == [(108, 12, 1)]
    rgbx = planes(_u8(5, 7, 4)[:, :, :3], "hwc")
    assert view_strides([rgbx]) == [(1, 28, 4)]
    assert view_strides([_u8(1, 5, 7).expand(3, 5, 7)]) == [(0, 7, 1)]
    # the stride of a dimension of size 1 addresses nothing
    assert is_dense_planar(_u8(1, 5, 7).as_strided((1, 5, 7), (999, 7, 1)))
    assert is_dense_planar(planes(_u8(1, 1, 3), "hwc"))      # a 1x1 image is both


# ------------------------------------------------------------------ sources
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_sources_of_any_strides_are_accepted(layout):
    from idfcodec.tiled import source_views
    shape = lambda H, W: (3, H, W) if layout == "chw" else (H, W, 3)  # noqa: E731
    big = _u8(*shape(9, 12))
    window = big[:, 2:7, 3:10] if layout == "chw" else big[2:7, 3:10, :]
    gray = _u8(5, 7)
    flat = gray.expand(3, 5, 7) if layout == "chw" else gray[:, :, None].expand(5, 7, 3)
    perm = _u8(*shape(4, 6)[::-1]).permute(2, 1, 0)     # the right shape, reversed strides
    views = source_views([big, window, flat, perm], 3, CPU, layout)
    assert [tuple(v.shape) for v in views] == [(3, 9, 12), (3, 5, 7), (3, 5, 7), (3, 4, 6)]
    assert views[2].stride(0) == 0                      # a zero channel stride is a source
    for v, t in zip(views, (big, window, flat, perm)):
        assert v.data_ptr() == t.data_ptr()
        assert torch.equal(v, t if layout == "chw" else t.permute(2, 0, 1))
    # the 4-D batch forms, a non-contiguous slice of a larger batch included
    batch = _u8(4, *shape(5, 7))
    views = source_views(batch[1::2], 3, CPU, layout)
    assert len(views) == 2 and all(tuple(v.shape) == (3, 5, 7) for v in views)
    assert views[1].data_ptr() == batch[3].data_ptr()
    inner = batch[:, :, 1:4] if layout == "chw" else batch[:, 1:4]
    assert [tuple(v.shape) for v in source_views(inner, 3, CPU, layout)] == [(3, 3, 7)] * 4


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_sources_are_refused_as_before(layout):
    from idfcodec.tiled import source_views
    shape = lambda C, H, W: (C, H, W) if layout == "chw" else (H, W, C)  # noqa: E731
    ok = _u8(*shape(3, 5, 7))
    for bad, msg in (([ok.float()], "not uint8"), ([_u8(*shape(4, 5, 7))], "channels"),
                     ([_u8(*shape(3, 0, 7))], "zero-sized"), ([_u8(*shape(3, 5, 0))], "zero-sized"),
                     ([ok[0]], "tensor"), ([], "no images"), (_u8(2, 3, 4, 5, 6), "list of"),
                     ([ok.numpy()], "tensor")):
        with pytest.raises(ValueError, match=msg):
            source_views(bad, 3, CPU, layout)
    with pytest.raises(ValueError, match="lies on"):
        source_views([ok], 3, torch.device("cuda", 0), layout)
    with pytest.raises(ValueError, match="layout"):
        source_views([ok], 3, CPU, "cwh")
    # the other layout's shape has the wrong channel count
    with pytest.raises(ValueError, match="channels"):
        source_views([ok], 3, CPU, "hwc" if layout == "chw" else "chw")


def test_without_a_layout_only_contiguous_planar_sources_pass():
    """encode's contract before layouts, kept for every call that names none."""
    from idfcodec.tiled import as_chw, source_views
    ok, big = _u8(3, 5, 7), _u8(3, 9, 12)
    views = source_views([ok, big], 3, CPU)
    assert views[0] is ok and views[1] is big
    assert len(source_views(_u8(2, 3, 5, 7), 3, CPU, None)) == 2
    for bad in ([big[:, 2:7, 3:10]], [ok, _u8(5, 7, 3).permute(2, 0, 1)],
                [_u8(5, 7).expand(3, 5, 7)], _u8(4, 3, 5, 7)[1::2], _u8(2, 3, 5, 14)[..., ::2]):
        with pytest.raises(ValueError, match="not contiguous"):
            source_views(bad, 3, CPU)
        with pytest.raises(ValueError, match="not contiguous"):
            as_chw(bad, None)
        assert len(source_views(bad, 3, CPU, "chw")) == len(bad)    # named: a view is a source
    with pytest.raises(ValueError, match="channels"):               # [H, W, C] needs its name
        source_views([_u8(5, 7, 3)], 3, CPU)


# ------------------------------------------------------------------ outputs
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_outputs_new_and_given(layout):
    from idfcodec.tiled import output_views
    shape = lambda C, H, W: (C, H, W) if layout == "chw" else (H, W, C)  # noqa: E731
    outs, views = output_views([(3, 5, 7), (3, 1, 1)], CPU, layout)
    assert [tuple(o.shape) for o in outs] == [shape(3, 5, 7), shape(3, 1, 1)]
    assert all(o.is_contiguous() and o.dtype == torch.uint8 for o in outs)
    assert [tuple(v.shape) for v in views] == [(3, 5, 7), (3, 1, 1)]
    assert [v.data_ptr() for v in views] == [o.data_ptr() for o in outs]
    # the caller's: a pitched canvas, a window, RGBX
    canvas = _u8(*shape(3, 9, 12))
    window = canvas[:, 2:7, 3:10] if layout == "chw" else canvas[2:7, 3:10]
    rgbx = _u8(5, 7, 4)[:, :, :3] if layout == "hwc" else _u8(4, 5, 7)[:3]
    for t in (window, rgbx):
        outs, views = output_views([(3, 5, 7)], CPU, layout, [t])
        assert outs[0] is t and views[0].data_ptr() == t.data_ptr()
        assert tuple(views[0].shape) == (3, 5, 7)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_outputs_that_overlap_or_do_not_fit_are_refused(layout):
    from idfcodec.tiled import check_no_overlap, output_views
    shape = lambda C, H, W: (C, H, W) if layout == "chw" else (H, W, C)  # noqa: E731
    ok = _u8(*shape(3, 5, 7))
    gray = _u8(5, 7)
    flat = gray.expand(3, 5, 7) if layout == "chw" else gray[:, :, None].expand(5, 7, 3)
    with pytest.raises(ValueError, match="twice"):       # a zero channel stride
        output_views([(3, 5, 7)], CPU, layout, [flat])
    rows = _u8(128).as_strided(shape(3, 5, 7), shape(1, 4, 1) if layout == "hwc" else (35, 4, 1))
    with pytest.raises(ValueError, match="twice"):       # rows of 7 bytes, 4 apart
        output_views([(3, 5, 7)], CPU, layout, [rows])
    for bad, msg in (([ok.float()], "uint8"), ([_u8(*shape(3, 5, 8))], "shape"),
                     ([ok.permute(2, 1, 0)], "shape"), ([ok, ok], "holds 2"), ([], "holds 0"),
                     ([ok.numpy()], "uint8")):
        with pytest.raises(ValueError, match=msg):
            output_views([(3, 5, 7)], CPU, layout, bad)
    with pytest.raises(ValueError, match="lies on"):
        output_views([(3, 5, 7)], torch.device("cuda", 0), layout, [ok])
    # the rule itself: sorted by stride, each at least the previous stride times its size
    check_no_overlap(_u8(3, 5, 7), "x")
    check_no_overlap(_u8(3, 5, 7).permute(1, 2, 0), "x")
    check_no_overlap(_u8(3, 5, 12)[:, :, :7], "x")
    check_no_overlap(_u8(200).as_strided((3, 5, 7), (1, 21, 3)), "x")
    check_no_overlap(_u8(200).as_strided((3, 5, 7), (1, 26, 3)), "x")
    check_no_overlap(_u8(3, 1, 1).as_strided((3, 1, 1), (1, 0, 0)), "x")   # sizes of 1 aside
    for strides in ((1, 20, 3), (1, 21, 2), (0, 7, 1), (35, 7, 0), (35, 6, 1)):
        with pytest.raises(ValueError, match="twice"):
            check_no_overlap(_u8(200).as_strided((3, 5, 7), strides), "x")


# ------------------------------------------------------------------ the ABI
def test_header_declares_and_lib_binds_the_strided_entry_points():
    from idfcodec import _lib
    with open(_lib.HEADER) as f:
        header = f.read()
    for name in STRIDED:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        planar = re.search(r"\bint %s\(([^;]*)\);" % name.replace("_strided", ""), header)
        norm = lambda m: re.sub(r"\s+", " ", m.group(1))  # noqa: E731
        assert norm(decl) == norm(planar), name          # the sibling's arguments
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_strided", "")]
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert all(hasattr(L, name) for name in STRIDED)
    assert "sc, sy, sx" in header


def test_device_calls_pick_the_entry_point_by_the_table_width():
    from idfcodec import tiled

    class Lib:
        idf_tile_gather_u8, idf_tile_gather_strided_u8 = "planar", "strided"

    real = tiled.lib
    tiled.lib = lambda: Lib
    try:
        assert tiled._entry("idf_tile_gather_u8", 5) == "planar"
        assert tiled._entry("idf_tile_gather_u8", 8) == "strided"
    finally:
        tiled.lib = real


# ------------------------------------------------------------------ the file tool
def _tool():
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_file_tool_reads_as_stored_and_writes_either_layout(tmp_path):
    tool = _tool()
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)
    hwc = np.ascontiguousarray(rgb.transpose(1, 2, 0))
    gray = rng.integers(0, 256, (1, 4, 3), dtype=np.uint8)
    p = tool.write_image(str(tmp_path), 0, rgb)
    a, layout = tool.read_image_stored(p, 3)
    assert layout == "hwc" and a.shape == (5, 7, 3) and np.array_equal(a, hwc)
    with open(p, "rb") as f:
        data = f.read()
    assert data.endswith(a.tobytes())                     # the file's own bytes, not transposed
    g = tool.write_image(str(tmp_path), 1, gray)
    a, layout = tool.read_image_stored(g, 1)
    assert layout == "hwc" and np.array_equal(a, gray.transpose(1, 2, 0))
    np.save(tmp_path / "hwc.npy", hwc)
    np.save(tmp_path / "chw.npy", rgb)
    np.save(tmp_path / "hw.npy", gray[0])
    for name, want, lay in (("hwc.npy", hwc, "hwc"), ("chw.npy", rgb, "chw"),
                            ("hw.npy", gray, "chw")):
        a, layout = tool.read_image_stored(str(tmp_path / name), want.shape[2 if lay == "hwc"
                                                                            else 0])
        assert layout == lay and np.array_equal(a, want), name
    for path, C in ((g, 3), (str(tmp_path / "hw.npy"), 3), (str(tmp_path / "chw.npy"), 4)):
        with pytest.raises(ValueError):
            tool.read_image_stored(path, C)
    # write_image(layout="hwc") writes the file the planar call writes
    os.makedirs(tmp_path / "b")
    for i, chw in enumerate((rgb, gray, rng.integers(0, 256, (4, 3, 2), dtype=np.uint8))):
        one = tool.write_image(str(tmp_path), 10 + i, chw)
        two = tool.write_image(str(tmp_path / "b"), 10 + i, chw.transpose(1, 2, 0), layout="hwc")
        assert os.path.basename(one) == os.path.basename(two)
        with open(one, "rb") as f, open(two, "rb") as h:
            assert f.read() == h.read()
    with pytest.raises(ValueError):
        tool.write_image(str(tmp_path), 0, rgb, layout="cwh")
