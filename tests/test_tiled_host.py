"""Images of any size as tiles, on the host (no device): the tiling rule against the
reference's ReplicationPad2d + Patching output, the tile table and the region arithmetic,
Bitstream.select on a hand-built bitstream, the IDFT container and its error cases, and the
stream overhead per sub-pixel."""
import struct

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def tiny(golden):
    return golden("tiled_tiny.npz")


def _sets(d):
    return [(d[f"img{k}"], d[f"tiles{k}"], tuple(int(v) for v in d[f"tile_hw{k}"]))
            for k in range(int(d["n"]))]


# ------------------------------------------------------------------ the rule
def test_tiles_host_equals_reference(tiny):
    from idfcodec.tiled import tiles_host
    sets = _sets(tiny)
    assert [s[0].shape for s in sets] == [(3, 1, 1), (3, 16, 16), (3, 17, 16), (3, 5, 40),
                                          (3, 37, 21), (1, 25, 9)]
    for img, tiles, (th, tw) in sets:
        got = tiles_host(img, th, tw)
        assert got.dtype == np.uint8 and got.shape == tiles.shape, img.shape
        assert np.array_equal(got, tiles), img.shape
    # the bytes on both sides of the dequantiser's step are in the fixture
    assert all(np.isin([0, 127, 128, 255], s[0]).all() for s in sets[1:])


def test_tile_table_counts_and_order():
    from idfcodec.tiled import tile_table
    sizes = [(1, 1), (16, 16), (17, 16), (16, 17), (5, 40), (37, 21)]
    counts, entries = tile_table(sizes, 16, 16)
    assert counts == [1, 1, 2, 2, 3, 6] and len(entries) == sum(counts)
    assert entries[:4] == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0)]
    assert entries[4:6] == [(3, 0, 0), (3, 0, 1)]
    assert entries[6:9] == [(4, 0, 0), (4, 0, 1), (4, 0, 2)]
    assert entries[9:] == [(5, 0, 0), (5, 0, 1), (5, 1, 0), (5, 1, 1), (5, 2, 0), (5, 2, 1)]
    assert tile_table([(25, 9), (12, 8)], 12, 8) == ([6, 1], [(0, ty, tx) for ty in range(3)
                                                            for tx in range(2)] + [(1, 0, 0)])
    assert tile_table([], 4, 4) == ([], [])
    for bad in ([(0, 5)], [(5, 0)]):
        with pytest.raises(ValueError):
            tile_table(bad, 16, 16)
    with pytest.raises(ValueError):
        tile_table([(5, 5)], 0, 16)


def test_tile_layout():
    """Everything the codecs take from a TileLayout, on a ragged set: no device."""
    from idfcodec.tiled import TileLayout
    sizes = [(32, 32), (16, 16), (17, 16), (40, 37), (5, 40)]
    lay = TileLayout(sizes, 3, (16, 16))
    assert lay.counts == [4, 1, 2, 9, 3] and lay.first == [0, 4, 5, 7, 16, 19]
    assert lay.n_tiles == 19 == len(lay.entries) == len(lay.rects)
    assert lay.n_subpixels == 3 * (32 * 32 + 16 * 16 + 17 * 16 + 40 * 37 + 5 * 40)
    assert lay.entries[4:7] == [(1, 0, 0), (2, 0, 0), (2, 1, 0)]
    assert lay.rects[lay.first[3] - 1] == (1, 16)          # the last entry of image 2
    assert lay.rects[7:16] == [(16, 16), (16, 16), (16, 5)] * 2 + [(8, 16), (8, 16), (8, 5)]
    # every entry's row, image i at address 1000 * (i + 1)
    rows = lay.rows([1000 * (i + 1) for i in range(5)])
    assert rows == [(1000 * (i + 1), *sizes[i], 16 * ty, 16 * tx) for i, ty, tx in lay.entries]
    # whole images, in the order asked: entries, and rows that name the output by its place
    want, entries, rows = lay.image_rows([2, 0])
    assert want == [2, 0] and entries == [5, 6, 0, 1, 2, 3]
    assert rows == [(0, 17, 16, 0, 0), (0, 17, 16, 16, 0), (1, 32, 32, 0, 0), (1, 32, 32, 0, 16),
                    (1, 32, 32, 16, 0), (1, 32, 32, 16, 16)]
    assert lay.place(rows, [70, 80])[1:3] == [(70, 17, 16, 16, 0), (80, 32, 32, 0, 0)]
    assert lay.image_rows()[:2] == (list(range(5)), list(range(19)))
    assert lay.image_rows([]) == ([], [], [])
    for bad in ([5], [0, -1]):
        with pytest.raises(ValueError, match="outside"):
            lay.image_rows(bad)
    # a region: image 3 is 3 x 3 tiles from entry 7; rows [30, 37) x columns [10, 21) touch
    # tile rows 1, 2 and tile columns 0, 1
    entries, rows = lay.region_rows(3, 30, 10, 7, 11)
    assert entries == [7 + 3, 7 + 4, 7 + 6, 7 + 7]
    assert rows == [(0, 7, 11, 16 - 30, 0 - 10), (0, 7, 11, 16 - 30, 16 - 10),
                    (0, 7, 11, 32 - 30, 0 - 10), (0, 7, 11, 32 - 30, 16 - 10)]
    with pytest.raises(ValueError, match="outside"):
        lay.region_rows(5, 0, 0, 1, 1)
    with pytest.raises(ValueError):
        lay.region_rows(3, 30, 10, 11, 11)
    # the header both containers open with
    head = lay.pack(b"IDFT")
    assert head == (struct.pack("<4sHHIIII", b"IDFT", 1, 0, 5, 3, 16, 16)
                    + b"".join(struct.pack("<II", *s) for s in sizes))
    assert TileLayout.unpack(head, b"IDFT", "tiled bitstream") == (lay, 24 + 8 * 5)
    assert TileLayout.unpack(head + b"rest", b"IDFT", "tiled bitstream", tail=4)[1] == 64
    with pytest.raises(ValueError, match="truncated tiled bitstream"):
        TileLayout.unpack(head, b"IDFT", "tiled bitstream", tail=1)
    with pytest.raises(ValueError, match="not an IDF safe tiled bitstream"):
        TileLayout.unpack(head, b"IDFS", "safe tiled bitstream")
    # a value: equal by sizes, C and tile size, whatever the sizes came as
    assert TileLayout([torch.Size(s) for s in sizes], 3, [16, 16]) == lay
    assert TileLayout(sizes, 3, (16, 8)) != lay


@pytest.mark.parametrize("rect,want", [
    ((3, 4, 5, 6), [(0, 0)]),                                   # inside one tile
    ((0, 0, 16, 16), [(0, 0)]),                                 # ends exactly on the tile's edge
    ((0, 0, 17, 16), [(0, 0), (1, 0)]),                         # one row past it
    ((16, 16, 16, 5), [(1, 1)]),                                # starts exactly on an edge
    ((15, 15, 2, 2), [(0, 0), (0, 1), (1, 0), (1, 1)]),         # across four tiles
    ((15, 15, 1, 1), [(0, 0)]), ((16, 16, 1, 1), [(1, 1)]),     # single pixels at a corner
    ((36, 20, 1, 1), [(2, 1)]),                                 # the image's last pixel
    ((0, 0, 37, 21), [(ty, tx) for ty in range(3) for tx in range(2)]),
])
def test_region_tiles(rect, want):
    from idfcodec.tiled import region_tiles
    y0, x0, h, w = rect
    got = region_tiles((37, 21), y0, x0, h, w, 16, 16)
    assert got == want
    n = ((y0 + h - 1) // 16 - y0 // 16 + 1) * ((x0 + w - 1) // 16 - x0 // 16 + 1)
    assert len(got) == n


@pytest.mark.parametrize("rect", [(0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4),
                                  (34, 0, 4, 4), (0, 18, 4, 4), (37, 0, 1, 1), (0, 0, 38, 21)])
def test_region_tiles_errors(rect):
    from idfcodec.tiled import region_tiles
    with pytest.raises(ValueError):
        region_tiles((37, 21), *rect, 16, 16)


# ------------------------------------------------------------------ Bitstream.select
def _hand_bitstream(N=4, n_lvl=2, seed=0):
    """Stream (l, e) holds nw = (3 * l + e) % 4 words of value 100 * (l * N + e) + j."""
    from idfcodec.codec import Bitstream
    nw = [(3 * l + e) % 4 for l in range(n_lvl) for e in range(N)]
    words = [100 * k + j for k, n in enumerate(nw) for j in range(n)]
    states = [(1 << 32) + k for k in range(n_lvl * N)]
    t = lambda a, dt: torch.tensor(a, dtype=dt)  # noqa: E731
    return Bitstream(N, [(6, 8, 8), (12, 4, 4)][:n_lvl], t(states, torch.int64),
                     t(nw, torch.int64), t(words, torch.int32),
                     meta={"n_subpixels": N * 3 * 16 * 16, "conv": "f32"},
                     host_nwords=t(nw, torch.int64))


def _streams(bs):
    """{(level, entry): (state, [words])}"""
    N = bs.n_images
    off = bs.word_offsets().tolist()
    nw = bs.nwords.tolist()
    return {(k // N, k % N): (int(bs.states[k]), bs.words[off[k]:off[k] + nw[k]].tolist())
            for k in range(bs.n_streams)} if N else {}


@pytest.mark.parametrize("entries", [[1, 3], [3, 0, 2, 1], [2], [2, 2], []])
def test_select_subset_and_permutation(entries):
    bs = _hand_bitstream()
    src = _streams(bs)
    sub = bs.select(entries)
    assert sub.n_images == len(entries) and sub.n_streams == 2 * len(entries)
    assert sub.group == 1 and sub.level_shapes == bs.level_shapes
    assert sub.meta["conv"] == "f32"
    assert sub.n_subpixels() == len(entries) * 3 * 16 * 16
    assert sub.host_nwords is not None and torch.equal(sub.host_nwords, sub.nwords)
    assert int(sub.nwords.sum()) == sub.words.numel()
    got = _streams(sub)
    for l in range(2):
        for j, e in enumerate(entries):
            assert got[(l, j)] == src[(l, e)], (l, j, e)
    # the source is unchanged
    assert _streams(bs) == src and bs.n_images == 4


def test_select_identity_equals_input():
    bs = _hand_bitstream()
    same = bs.select(range(4))
    assert torch.equal(same.states, bs.states) and torch.equal(same.nwords, bs.nwords)
    assert torch.equal(same.words, bs.words)
    assert same.to_bytes() == bs.to_bytes()
    # from a file, and again through select
    from idfcodec.codec import Bitstream
    back = Bitstream.from_bytes(bs.to_bytes())
    assert back.select([0, 1, 2, 3]).to_bytes() == bs.to_bytes()
    # two selections compose
    assert bs.select([3, 1, 0]).select([2, 0]).to_bytes() == bs.select([0, 3]).to_bytes()


def test_select_errors():
    from idfcodec.codec import Bitstream
    bs = _hand_bitstream()
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(ValueError, match="outside"):
            bs.select(bad)
    grouped = Bitstream(4, bs.level_shapes, bs.states[:4], bs.nwords[:4],
                        bs.words[:int(bs.nwords[:4].sum())], meta=dict(bs.meta), group=2)
    with pytest.raises(ValueError, match="shares a stream"):
        grouped.select([0])
    scratch = Bitstream(4, bs.level_shapes, bs.states, bs.nwords, bs.words,
                        meta=dict(bs.meta, scratch_offsets=torch.zeros(8, dtype=torch.int64)))
    with pytest.raises(ValueError, match="compacted"):
        scratch.select([0])


# ------------------------------------------------------------------ the IDFT container
SIZES = [(1, 1), (17, 16), (5, 40)]     # 1 + 2 + 3 tiles at 16x16


def _tiled(N=6):
    from idfcodec.tiled import TiledBitstream
    return TiledBitstream(_hand_bitstream(N), list(SIZES), 3, (16, 16))


def test_idft_round_trip_and_layout():
    from idfcodec.tiled import TiledBitstream
    tbs = _tiled()
    raw = tbs.to_bytes()
    inner = tbs.stream.to_bytes()
    want = (struct.pack("<4sHHIIII", b"IDFT", 1, 0, 3, 3, 16, 16)
            + b"".join(struct.pack("<II", *s) for s in SIZES) + struct.pack("<Q", len(inner)))
    assert raw == want + inner
    assert struct.unpack_from("<I", inner, 8)[0] == 6   # the inner n_images field holds N
    back = TiledBitstream.from_bytes(raw)
    assert back.sizes == SIZES and back.C == 3 and back.tile_hw == (16, 16)
    assert back.n_images == 3 and back.stream.n_images == 6
    assert back.to_bytes() == raw
    assert _streams(back.stream) == _streams(tbs.stream)
    assert back.bits() == tbs.bits() == tbs.stream.bits()


def test_idft_bytes_are_frozen():
    """The digest of the hand-built container, taken before TileLayout wrote its header."""
    import hashlib
    assert hashlib.sha256(_tiled().to_bytes()).hexdigest() == \
        "4b6cc28204342c3f541b6925d051452fe6a5bec5f8377d24646dc97f3461b3ff"


def _patched(raw, fmt, offset, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_idft_errors():
    from idfcodec.tiled import TiledBitstream
    raw = _tiled().to_bytes()
    o_len = 24 + 8 * len(SIZES)          # the u64 byte length
    o_inner = o_len + 8
    cases = {
        "magic": _patched(raw, "<4s", 0, b"IDFB"),
        "version": _patched(raw, "<H", 4, 2),
        "flags": _patched(raw, "<H", 6, 1),
        "zero n_images": _patched(raw, "<I", 8, 0),
        "zero C": _patched(raw, "<I", 12, 0),
        "zero tile_h": _patched(raw, "<I", 16, 0),
        "zero tile_w": _patched(raw, "<I", 20, 0),
        "zero H": _patched(raw, "<I", 24 + 8, 0),
        "zero W": _patched(raw, "<I", 24 + 4, 0),
        "truncated header": raw[:20],
        "truncated sizes": raw[:24 + 8],
        "truncated length": raw[:o_len + 4],
        "truncated payload": raw[:-4],
        "trailing bytes": raw + b"\0\0\0\0",
        "length too small": _patched(raw, "<Q", o_len, len(raw) - o_inner - 4),
        "length too large": _patched(raw, "<Q", o_len, len(raw) - o_inner + 4),
        "inner truncated": raw[:o_len] + struct.pack("<Q", 10) + raw[o_inner:o_inner + 10],
        "inner magic": _patched(raw, "<4s", o_inner, b"IDFX"),
    }
    for name, buf in cases.items():
        with pytest.raises(ValueError):
            TiledBitstream.from_bytes(buf)
            pytest.fail(name)
    # an inner entry count that differs from the sum of the images' tiles
    for N in (5, 7):
        with pytest.raises(ValueError, match="tiles"):
            TiledBitstream.from_bytes(_tiled(N).to_bytes())
    # another image size with the same tile count is no error of the container
    assert TiledBitstream.from_bytes(_patched(raw, "<I", 24 + 8, 20)).sizes[1] == (20, 16)


# ------------------------------------------------------------------ accounting
def test_bpd_and_state_bits_per_subpixel():
    from idfcodec.codec import Bitstream
    from idfcodec.tiled import TiledBitstream
    tbs = _tiled()
    nsub = 3 * (1 * 1 + 17 * 16 + 5 * 40)
    assert tbs.n_subpixels() == nsub
    assert tbs.bpd() == tbs.bits() / nsub
    assert tbs.stream.bpd() == tbs.bits() / (6 * 3 * 16 * 16)   # the padded denominator
    assert tbs.state_bits_per_subpixel() == 64 * 12 / nsub
    assert tbs.padded_share() == 1 - (1 + 17 * 16 + 5 * 40) / (6 * 256)
    # full tiles: 64 * levels / (C * th * tw); imagenet64's three levels at 3x64x64 pay 0.0156
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    full = TiledBitstream(Bitstream(4, [(6, 32, 32), (12, 16, 16), (48, 8, 8)],
                                    z(12, torch.int64), z(12, torch.int64), z(0, torch.int32)),
                          [(128, 128)], 3, (64, 64))
    assert full.state_bits_per_subpixel() == 64 * 3 / (3 * 64 * 64) == 0.015625
    assert full.padded_share() == 0.0


def test_file_tool_reads_and_writes_images(tmp_path):
    import importlib.util
    import os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)
    gray = rng.integers(0, 256, (1, 4, 3), dtype=np.uint8)
    p = tool.write_image(str(tmp_path), 0, rgb)
    assert p.endswith("image_0000.ppm") and np.array_equal(tool.read_image(p, 3), rgb)
    g = tool.write_image(str(tmp_path), 1, gray)
    assert g.endswith("image_0001.pgm") and np.array_equal(tool.read_image(g, 1), gray)
    with open(tmp_path / "c.ppm", "wb") as f:     # comments and other whitespace in the header
        f.write(b"P6 # made by hand\n# size\n7\t5\n255\n" + rgb.transpose(1, 2, 0).tobytes())
    assert np.array_equal(tool.read_image(str(tmp_path / "c.ppm"), 3), rgb)
    np.save(tmp_path / "hwc.npy", rgb.transpose(1, 2, 0))
    np.save(tmp_path / "chw.npy", rgb)
    np.save(tmp_path / "hw.npy", gray[0])
    assert np.array_equal(tool.read_image(str(tmp_path / "hwc.npy"), 3), rgb)
    assert np.array_equal(tool.read_image(str(tmp_path / "chw.npy"), 3), rgb)
    assert np.array_equal(tool.read_image(str(tmp_path / "hw.npy"), 1), gray)
    for path, C in ((g, 3), (str(tmp_path / "hw.npy"), 3)):
        with pytest.raises(ValueError):
            tool.read_image(path, C)
    with open(tmp_path / "t.ppm", "wb") as f:
        f.write(b"P6\n7 5\n255\n" + bytes(10))
    with pytest.raises(ValueError):
        tool.read_image(str(tmp_path / "t.ppm"), 3)


def test_exports_and_model_checks():
    import idfcodec
    from idfcodec import synthetic, tiled
    from idfcodec.configs import _dense, _flows
    assert idfcodec.TiledCodec is tiled.TiledCodec
    assert idfcodec.TiledBitstream is tiled.TiledBitstream
    args = (2, 1, 8, 8, 3, _dense(8, 1), _dense(8, 1), 2)
    plain = synthetic.build_model(_flows("IDFlows", *args))
    assert tiled.TiledCodec(plain, max_batch=3).tile_hw == (8, 8)
    with pytest.raises(ValueError):
        tiled.TiledCodec(plain, max_batch=0)
    with pytest.raises(TypeError):
        tiled.TiledCodec(synthetic.build_model(_flows("ConditionalFlows", *args)))
    with pytest.raises(TypeError):
        tiled.TiledCodec(torch.nn.Identity())
    with pytest.raises(NotImplementedError):
        tiled.TiledCodec(synthetic.build_model(_flows("IDFlows", *args, batch_squeeze=2)))
