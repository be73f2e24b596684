"""Images of any size, coded as tiles of an IDFlows' input.

A model with input C x th x tw codes image i of C x H_i x W_i (any H_i, W_i >= 1) as
nh_i * nw_i tiles, nh_i = ceil(H_i / th), nw_i = ceil(W_i / tw).  Tile (ty, tx) has its origin
at (ty * th, tx * tw); its pixel (r, c) is source pixel (min(ty*th + r, H_i - 1),
min(tx*tw + c, W_i - 1)): bit for bit the reference's ReplicationPad2d((0, pw, 0, ph))
(trainer.py:62) followed by Patching(Hp, Wp, th, tw).forward (extenddim.py:51-57); tiles_host is
the numpy restatement the kernels are tested against.  Entries are ordered by image, then tile
row, then tile column; all images' tiles in that order are one batch of N entries.

encode: idf_tile_gather_u8 reads the source bytes where the caller's tensors lie (a device
        table of addresses; no concatenation, no torch op on pixel data) and writes each chunk
        of at most max_batch tiles straight into the FlowEngine's input; the chunks run through
        ImageCodec._encode_guarded and their streams are merged level-major, entry-minor into
        one Bitstream of N entries (one rANS stream per (tile, level)).  The convs are
        batch-invariant, so the bytes do not depend on max_batch or on the lanes.
decode: chunks of at most max_batch entries (Bitstream.select) through the decode lanes, then
        idf_tile_scatter_u8 into outputs of the source sizes; the pad is never written.
        A tile's streams depend on no other tile's: decode(images=...) and decode_region decode
        only the tiles they need.

Memory layouts.  encode(images, layout=...) takes any uint8 device tensor of shape [C, H, W]
("chw") or [H, W, C] ("hwc"), contiguous or not: interleaved pixels, a row pitch, RGBX, a window
of a larger image, a slice of a larger batch, a plane expanded over the channels.  `layout` names
the order of the dimensions, the tensor's own strides say where the bytes are; they go into the
tile table (rows of eight fields, idf_tile_gather_strided_u8 and its siblings), so nothing is
copied.  decode(..., layout=..., out=...) returns dense tensors in the layout asked, or writes
into tensors of the caller's (any strides whose bytes do not coincide; bytes the image does not
address are left alone).  The layout is not stored: a file is byte for byte the file of the
planar copy of its source.  Without a layout argument (layout=None) encode keeps its earlier
contract: [C, H, W] tensors, each contiguous, and anything else is refused; naming the layout,
"chw" included, is what admits strides.

All chunks of one bitstream are coded in one conv mode: if the split-f16 range guard sent any
chunk to exact-f32 convs, the others are re-encoded in "f32" and the bitstream records "f32".

Container IDFT (little-endian): magic "IDFT", u16 version 1, u16 flags 0, u32 n_images, u32 C,
u32 tile_h, u32 tile_w, n_images x (u32 H, u32 W), u64 byte length, the inner IDFB container
(codec.Bitstream.to_bytes; its n_images field holds N).  The containers built on this one (IDFS,
IDFP, IDFQ, IDFM, IDFD) open with the same header (TileLayout.pack, unpack) and are read behind
it through Reader and written with pack_bitmap, pack_lengthed and pack_words.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from functools import cached_property
from itertools import accumulate

import numpy as np
import torch

from . import _lib, dist
from ._lib import check, lib, ptr
from .codec import Bitstream, check_ways, streams_ok

MAGIC = b"IDFT"
VERSION = 1                 # of the header both tiled containers (IDFT, IDFS) open with
_HDR = "<4sHHIIII"


# ------------------------------------------------------------------ host arithmetic
def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclass(frozen=True)
class TileLayout:
    """The tiles of a list of images: all that follows from the images' sizes, the channel
    count and the tile size.  Pure host arithmetic, computed on first use.

    A table row (what TiledCodec._device_table takes) is (addr, H, W, y0, x0): a tile whose
    origin is pixel (y0, x0) of the uint8 buffer [C, H, W] at addr.  image_rows and region_rows
    plan a decode before its outputs exist: their rows hold the output's index in place of addr,
    and `place` puts the addresses in -- and, for images that are not dense planar, their byte
    strides (sc, sy, sx) behind them: byte (c, y, x) then lies at addr + c*sc + y*sy + x*sx."""
    sizes: tuple                # ((H, W), ...) per image
    C: int
    tile_hw: tuple              # (th, tw)

    def __post_init__(self):
        th, tw = (int(v) for v in self.tile_hw)
        if th < 1 or tw < 1:
            raise ValueError(f"tile size {(th, tw)} must be positive")
        sizes = tuple((int(H), int(W)) for H, W in self.sizes)
        for i, (H, W) in enumerate(sizes):
            if H < 1 or W < 1:
                raise ValueError(f"image {i} has a zero-sized dimension {(H, W)}")
        for name, v in (("sizes", sizes), ("C", int(self.C)), ("tile_hw", (th, tw))):
            object.__setattr__(self, name, v)

    @cached_property
    def grids(self) -> list:
        """[(tile rows, tile columns)] per image"""
        th, tw = self.tile_hw
        return [(_ceil_div(H, th), _ceil_div(W, tw)) for H, W in self.sizes]

    @cached_property
    def counts(self) -> list:
        """tiles per image"""
        return [nh * nw for nh, nw in self.grids]

    @cached_property
    def first(self) -> list:
        """first[i]: the first entry of image i; first[n_images] = n_tiles"""
        return [0, *accumulate(self.counts)]

    @property
    def n_tiles(self) -> int:
        return self.first[-1]

    @property
    def n_subpixels(self) -> int:
        """of the unpadded images"""
        return sum(self.C * H * W for H, W in self.sizes)

    @cached_property
    def entries(self) -> list:
        """[(image, ty, tx)] in entry order"""
        return [(i, ty, tx) for i, (nh, nw) in enumerate(self.grids)
                for ty in range(nh) for tx in range(nw)]

    @cached_property
    def rects(self) -> list:
        """[(hin, win)] per entry: the in-image part of every tile"""
        th, tw = self.tile_hw
        return [(min(th, self.sizes[i][0] - ty * th), min(tw, self.sizes[i][1] - tx * tw))
                for i, ty, tx in self.entries]

    def _image(self, i) -> int:
        i = int(i)
        if not 0 <= i < len(self.sizes):
            raise ValueError(f"image {i} is outside the bitstream's {len(self.sizes)} images")
        return i

    def image_rows(self, images=None):
        """-> (images, entries, rows): the tiles of the images asked (their indices; default:
        all), in the order asked; rows[k] = (j, H, W, y0, x0) puts tile k into the j-th of
        them."""
        want = range(len(self.sizes)) if images is None else images
        want = [self._image(i) for i in want]
        th, tw = self.tile_hw
        entries, rows = [], []
        for j, i in enumerate(want):
            (H, W), (nh, nw) = self.sizes[i], self.grids[i]
            entries += range(self.first[i], self.first[i + 1])
            rows += [(j, H, W, ty * th, tx * tw) for ty in range(nh) for tx in range(nw)]
        return want, entries, rows

    def region_rows(self, image: int, y0: int, x0: int, h: int, w: int):
        """-> (entries, rows): exactly the tiles that intersect rows [y0, y0 + h) x columns
        [x0, x0 + w) of one image; rows[k] = (0, h, w, ...) puts tile k into an output of the
        region's size, its origin shifted by (-y0, -x0)."""
        image = self._image(image)
        th, tw = self.tile_hw
        tiles = region_tiles(self.sizes[image], y0, x0, h, w, th, tw)
        y0, x0, h, w = int(y0), int(x0), int(h), int(w)
        first, nw = self.first[image], self.grids[image][1]
        return ([first + ty * nw + tx for ty, tx in tiles],
                [(0, h, w, ty * th - y0, tx * tw - x0) for ty, tx in tiles])

    @staticmethod
    def place(rows, addrs, strides=None) -> list:
        """The planned rows with addrs[j] in place of j; strides: [(sc, sy, sx)] per j, appended
        to its rows (eight fields a row)."""
        if strides is None:
            return [(addrs[j], H, W, y, x) for j, H, W, y, x in rows]
        return [(addrs[j], H, W, y, x, *(int(s) for s in strides[j])) for j, H, W, y, x in rows]

    def rows(self, addrs, strides=None) -> list:
        """The table rows of every entry, image i lying at addrs[i] (with strides[i])."""
        return self.place(self.image_rows()[2], addrs, strides)

    def pack(self, magic: bytes, flags: int = 0) -> bytes:
        """The header and the size table that open the tiled containers.  flags: 0 but in the
        predictive containers, where it holds predict_ways > 1 (idfcodec.predict)."""
        hdr = struct.pack(_HDR, magic, VERSION, flags, len(self.sizes), self.C, *self.tile_hw)
        return hdr + b"".join(struct.pack("<II", H, W) for H, W in self.sizes)

    @classmethod
    def unpack(cls, buf: bytes, magic: bytes, name: str, tail: int = 0, flags_ok=(0,)):
        """-> (layout, the offset behind the size table) of a container `name` whose size table
        is followed by at least `tail` bytes.  flags_ok: the values of the header's u16 flags
        (bytes 6..7) the container accepts; every other is refused."""
        n_hdr = struct.calcsize(_HDR)
        if len(buf) < n_hdr:
            raise ValueError(f"truncated {name} (header)")
        got, ver, flags, n, C, th, tw = struct.unpack_from(_HDR, buf, 0)
        if got != magic:
            raise ValueError(f"not an IDF {name}")
        if ver != VERSION:
            raise ValueError(f"unknown {name} version {ver}")
        if flags not in flags_ok:
            raise ValueError(f"unknown {name} flags {flags:#x}")
        if min(n, C, th, tw) < 1:
            raise ValueError(f"{name} header holds a zero size")
        o = n_hdr + 8 * n
        if len(buf) < o + tail:
            raise ValueError(f"truncated {name} (image sizes)")
        sizes = [struct.unpack_from("<II", buf, n_hdr + 8 * i) for i in range(n)]
        if any(min(s) < 1 for s in sizes):
            raise ValueError(f"{name} holds an image with a zero size")
        return cls(sizes, C, (th, tw)), o


class Reader:
    """The bytes of a container `name` and the offset its parser has reached: what the tiled
    containers (IDFS, IDFP, IDFQ, IDFM, IDFD) are read through, behind their header.  A part
    that is cut off raises "truncated {name} ({what})"; `then`: the bytes that must follow the
    part for it to count as whole -- a length field behind it, which is then read unasked."""

    def __init__(self, buf: bytes, name: str, o: int = 0):
        self.buf, self.name, self.o = buf, name, o

    def take(self, n: int, what: str = None, then: int = 0) -> int:
        """-> the offset of the next n bytes, and moves behind them.  what None: an earlier
        take has vouched for them (as its `then`, or as a section they lie in)."""
        o = self.o
        if what is not None and len(self.buf) < o + n + then:
            raise ValueError(f"truncated {self.name} ({what})")
        self.o = o + n
        return o

    def u32(self) -> int:
        return struct.unpack_from("<I", self.buf, self.take(4))[0]

    def u64(self) -> int:
        return struct.unpack_from("<Q", self.buf, self.take(8))[0]

    def array(self, dtype, n: int, what: str = None, then: int = 0) -> np.ndarray:
        """The next n values of dtype: a read-only view of the bytes."""
        return np.frombuffer(self.buf, dtype, n,
                             self.take(n * np.dtype(dtype).itemsize, what, then))

    def bitmap(self, n: int, what: str, of: str, then: int = 0) -> np.ndarray:
        """bool [n]: n bits, LSB first, in ceil(n / 8) bytes whose other bits are clear."""
        bits = np.unpackbits(self.array(np.uint8, _ceil_div(n, 8), f"{what} bitmap", then),
                             bitorder="little")
        if bits[n:].any():
            raise ValueError(f"{self.name} of {n} {of} sets {what} bits past them")
        return bits[:n].astype(bool)

    def sub_bitmap(self, parent, what: str, of: str, then: int = 0) -> np.ndarray:
        """bool [len(parent)]: a bitmap over the positions the mask `parent` sets, the others
        clear."""
        parent = np.asarray(parent, dtype=bool)
        out = np.zeros(len(parent), dtype=bool)
        out[parent] = self.bitmap(int(parent.sum()), what, of, then)
        return out

    def lengthed(self, want: int, what: str, of: str, then: int = 0) -> np.ndarray:
        """uint8 [want]: a u64 length, which must be `want`, and that many raw bytes."""
        n = self.u64()
        if n != want:
            raise ValueError(f"{self.name} names {n} raw bytes, its {of} hold {want}")
        return self.array(np.uint8, n, what, then)

    def section(self, n: int, what: str, then: int = 0) -> "Reader":
        """-> a reader at the start of the next n bytes, and moves behind them."""
        return Reader(self.buf, self.name, self.take(n, what, then))

    def end(self, n: int, what: str = "packed section") -> "Reader":
        """section(n) where the container ends with it."""
        sect = self.section(n, what)
        if len(self.buf) > self.o:
            raise ValueError(f"{self.name} holds {len(self.buf) - self.o} trailing bytes")
        return sect


def pack_bitmap(mask, over=None) -> bytes:
    """What Reader.bitmap reads; over: a parent mask, what Reader.sub_bitmap reads."""
    mask = np.asarray(mask, dtype=bool)
    if over is not None:
        mask = mask[np.asarray(over, dtype=bool)]
    return np.packbits(mask, bitorder="little").tobytes()


def pack_lengthed(data) -> bytes:
    """What Reader.lengthed reads: a u64 length and the bytes (or a uint8 tensor's)."""
    if isinstance(data, torch.Tensor):
        data = data.detach().cpu().numpy().tobytes()
    return struct.pack("<Q", len(data)) + data


def pack_words(words: torch.Tensor) -> bytes:
    """int32 words as little-endian u32"""
    return words.detach().cpu().numpy().view(np.uint32).astype("<u4").tobytes()


def read_words(r: Reader, n: int) -> torch.Tensor:
    """n u32 words a section vouches for -> int32 [n]"""
    return torch.from_numpy(r.array("<u4", n).astype(np.uint32).view(np.int32).copy())


def check_words(name: str, nwords, words: torch.Tensor):
    """Raises unless the u32 word counts of a container `name` sum to the words it holds."""
    nw = np.asarray(nwords, dtype=np.int64)
    if (nw < 0).any() or (nw >= 1 << 32).any() or int(nw.sum()) != int(words.numel()):
        raise ValueError(f"{name} holds {words.numel()} words, its word counts name "
                         f"{int(nw.sum())}")


def tile_table(sizes, th: int, tw: int):
    """sizes: [(H, W)] per image -> (tiles per image, [(image, ty, tx)] in entry order: by
    image, then tile row, then tile column)."""
    lay = TileLayout(sizes, 1, (th, tw))
    return lay.counts, lay.entries


def region_tiles(size, y0: int, x0: int, h: int, w: int, th: int, tw: int):
    """The (ty, tx) of the tiles that intersect rows [y0, y0 + h) x columns [x0, x0 + w) of an
    image of size (H, W), in entry order: (floor((y0+h-1)/th) - floor(y0/th) + 1) *
    (floor((x0+w-1)/tw) - floor(x0/tw) + 1) of them.  An empty rectangle, or one not inside the
    image, raises ValueError."""
    H, W = (int(v) for v in size)
    y0, x0, h, w = int(y0), int(x0), int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"empty region {(h, w)}")
    if y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"region rows [{y0}, {y0 + h}) x columns [{x0}, {x0 + w}) is not "
                         f"inside the {H}x{W} image")
    return [(ty, tx) for ty in range(y0 // th, (y0 + h - 1) // th + 1)
            for tx in range(x0 // tw, (x0 + w - 1) // tw + 1)]


def tiles_host(img: np.ndarray, th: int, tw: int) -> np.ndarray:
    """numpy restatement of the tiling rule for one image [C, H, W]: its tiles
    [nh * nw, C, th, tw] in entry order, the pad by clamped indices."""
    img = np.asarray(img)
    C, H, W = img.shape
    ((nh, nw),) = TileLayout([(H, W)], C, (th, tw)).grids
    n = nh * nw
    ys = np.minimum(np.arange(nh * th), H - 1)
    xs = np.minimum(np.arange(nw * tw), W - 1)
    p = img[:, ys][:, :, xs]
    return p.reshape(C, nh, th, nw, tw).transpose(1, 3, 0, 2, 4).reshape(n, C, th, tw)


# ------------------------------------------------------------------ memory layouts
LAYOUTS = ("chw", "hwc")


def check_layout(layout) -> str:
    if layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r} is not one of {LAYOUTS}")
    return layout


def planes(t: torch.Tensor, layout: str) -> torch.Tensor:
    """A [C, H, W] view of a tensor whose dimensions are in `layout`'s order (no copy)."""
    return t if layout == "chw" else t.permute(2, 0, 1)


def _shape_in(layout: str, C: int, H: int, W: int) -> tuple:
    return (C, H, W) if layout == "chw" else (H, W, C)


def is_dense_planar(v: torch.Tensor) -> bool:
    """Whether the [C, H, W] view v is what a five-field table row names: strides (H*W, W, 1).
    The stride of a dimension of size 1 addresses nothing and is not looked at."""
    C, H, W = v.shape
    return all(n == 1 or s == want for n, s, want in zip(v.shape, v.stride(), (H * W, W, 1)))


def check_no_overlap(v: torch.Tensor, what: str):
    """Raises unless no two elements of v share a byte: with the dimensions sorted by stride,
    each stride is at least the previous stride times the previous size, and none is zero
    (dimensions of size 1 aside).  Sufficient, and what every view carved out of a dense tensor
    by slicing and permuting meets."""
    dims = sorted((s, n) for n, s in zip(v.shape, v.stride()) if n > 1)
    reach = 1
    for s, n in dims:
        if s < reach:
            raise ValueError(f"{what} of shape {tuple(v.shape)}, strides {tuple(v.stride())} "
                             "addresses a byte twice; a decode needs an output without overlap")
        reach = s * n


def _require_contiguous(images):
    """Raises for a tensor among images (a batch tensor, or a list's tensors) that is not
    contiguous: what encode refuses while no layout is named."""
    if isinstance(images, torch.Tensor):
        if not images.is_contiguous():
            raise ValueError("the image batch is not contiguous (name its layout to code a view: "
                             "layout='chw')")
        return
    for i, t in enumerate(images):
        if isinstance(t, torch.Tensor) and not t.is_contiguous():
            raise ValueError(f"image {i} is not contiguous (name the layout to code a view: "
                             "layout='chw')")


def as_chw(images, layout):
    """images as encode takes them in `layout` -> the same as "chw" input: [C, H, W] views of the
    tensors (of the batch tensor: [B, C, H, W]), no copy.  layout None: "chw" with every tensor
    contiguous, encode's contract before layouts.  Whatever is no tensor of the right rank is
    passed on for source_views to refuse."""
    if layout is None:
        images = images if isinstance(images, torch.Tensor) else list(images)
        _require_contiguous(images)
        return images
    if check_layout(layout) == "chw":
        return images
    if isinstance(images, torch.Tensor):
        return images.permute(0, 3, 1, 2) if images.dim() == 4 else images
    return [t.permute(2, 0, 1) if isinstance(t, torch.Tensor) and t.dim() == 3 else t
            for t in images]


_COPY_AS = {torch.uint16: torch.int16}


def _dtype_name(dtype) -> str:
    return str(dtype).rpartition(".")[2]


def source_views(images, C: int, dev, layout=None, dtype=torch.uint8, host_ok: bool = False,
                 owner: str = None) -> list:
    """images as encode takes them -> their [C, H_i, W_i] views, checked: of dtype, on dev, C
    channels, no zero-sized dimension; with a layout named any strides (they go into the tile
    table), with None contiguous tensors only.  host_ok: a host tensor is copied to dev, not
    refused.  owner: who the messages say holds the device and the channel count, where that is
    no engine and no model."""
    images = as_chw(images, layout)
    layout = layout or "chw"
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("images: a list of [C, H, W] tensors or one [B, C, H, W] tensor "
                             "(layout='hwc': [H, W, C], [B, H, W, C])")
        images = [images[i] for i in range(images.shape[0])]
    images = list(images)
    if not images:
        raise ValueError("no images to encode")
    for i, v in enumerate(images):
        if not isinstance(v, torch.Tensor) or v.dim() != 3:
            raise ValueError(f"image {i} is no [{', '.join(_shape_in(layout, 'C', 'H', 'W'))}] "
                             "tensor")
        if v.dtype != dtype:
            raise ValueError(f"image {i} is {v.dtype}, not {_dtype_name(dtype)}")
        if v.device != dev:
            if not host_ok or v.device.type != "cpu":
                raise ValueError(f"image {i} lies on {v.device}, the {owner or 'engine'} on "
                                 f"{dev}")
            # copies between tensors of unsigned 16-bit samples go through the signed view
            moved = _COPY_AS.get(dtype, dtype)
            images[i] = v.view(moved).to(dev).view(dtype)
        if v.shape[0] != C:
            raise ValueError(f"image {i} has {v.shape[0]} channels, the {owner or 'model'} {C}")
        if v.shape[1] < 1 or v.shape[2] < 1:
            raise ValueError(f"image {i} has a zero-sized dimension "
                             f"{_shape_in(layout, *v.shape)}")
    return images


def output_views(shapes, dev, layout: str = "chw", out=None, dtype=torch.uint8,
                 owner: str = None):
    """The tensors a decode writes: shapes = [(C, H, W)] per output -> (what the caller gets,
    their [C, H, W] views).  out None: new dense tensors in `layout`; else the caller's list,
    one tensor per shape, each of dtype on dev, of that shape in `layout`, of any strides that
    address no byte twice."""
    check_layout(layout)
    if out is None:
        out = [torch.empty(_shape_in(layout, *s), dtype=dtype, device=dev) for s in shapes]
        return out, [planes(t, layout) for t in out]
    out = list(out)
    if len(out) != len(shapes):
        raise ValueError(f"out holds {len(out)} tensors, the decode writes {len(shapes)}")
    for i, (t, s) in enumerate(zip(out, shapes)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"out[{i}] is no {_dtype_name(dtype)} tensor")
        if t.device != dev:
            raise ValueError(f"out[{i}] lies on {t.device}, the {owner or 'engine'} on {dev}")
        if tuple(t.shape) != _shape_in(layout, *s):
            raise ValueError(f"out[{i}] has shape {tuple(t.shape)}, the decode writes "
                             f"{_shape_in(layout, *s)} (layout {layout!r})")
        check_no_overlap(t, f"out[{i}]")
    return out, [planes(t, layout) for t in out]


def view_strides(views):
    """-> None where every [C, H, W] view is dense planar (five-field rows, the planar kernels),
    else [(sc, sy, sx)] per view in bytes (eight-field rows)."""
    if all(is_dense_planar(v) for v in views):
        return None
    return [tuple(v.stride()) for v in views]


# ------------------------------------------------------------------ device calls
def _check_table(table: torch.Tensor, n: int) -> int:
    """-> the fields of the table's rows: 8 for int64 [n_tiles, 8], else 5."""
    _lib.require_device(table, "tile table")
    fields = 8 if table.dim() == 2 and table.shape[1] == 8 else 5
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < n * fields:
        raise ValueError("tile table must be contiguous int64 [n_tiles, 5] or [n_tiles, 8]")
    return fields


def _entry(name: str, fields: int):
    """The entry point `name` (idf_tile_..._u8) for a table of that many fields."""
    return getattr(lib(), name if fields == 5 else name.replace("_u8", "_strided_u8"))


def device_gather(table: torch.Tensor, n: int, C: int, th: int, tw: int, out: torch.Tensor,
                  ld: int = 4):
    """table: device int64 [>= n, 5] rows (addr, H, W, y0, x0), or [>= n, 8] rows with the byte
    strides (sc, sy, sx) behind them -> out, the pixel-major (ld) float32 rows of n tiles
    (idf_tile_gather_u8, idf_tile_gather_strided_u8)."""
    fields = _check_table(table, n)
    _lib.require_device(out, "tile buffer")
    if out.dtype != torch.float32 or out.numel() < n * th * tw * ld:
        raise ValueError("gather output must be float32 and hold n * th * tw * ld values")
    check(_entry("idf_tile_gather_u8", fields)(_lib.stream_ptr(out.device), n, C, th, tw,
                                               ptr(table), ptr(out), ld), "tile gather")


def device_scatter(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                   bad: torch.Tensor, ld: int = 4):
    """The pixel-major rows of n tiles -> the uint8 buffers the table names
    (idf_tile_scatter_u8; idf_tile_scatter_strided_u8 for rows of eight fields); bad: int32[1],
    the off-grid count of the pixels written."""
    fields = _check_table(table, n)
    _lib.require_device(src, "tile buffer")
    _lib.require_device(bad, "off-grid counter")
    if src.dtype != torch.float32 or src.numel() < n * th * tw * ld:
        raise ValueError("scatter input must be float32 and hold n * th * tw * ld values")
    if bad.dtype != torch.int32 or bad.numel() < 1:
        raise ValueError("the off-grid counter is int32[1]")
    check(_entry("idf_tile_scatter_u8", fields)(_lib.stream_ptr(src.device), n, C, th, tw,
                                                ptr(src), ld, ptr(table), ptr(bad)),
          "tile scatter")


# ------------------------------------------------------------------ container
class _TiledSizes:
    """What both tiled containers derive from their sizes, C and tile_hw."""

    @property
    def layout(self) -> TileLayout:
        return TileLayout(self.sizes, self.C, self.tile_hw)

    @property
    def n_images(self) -> int:
        return len(self.sizes)

    def tile_counts(self) -> list:
        return self.layout.counts

    def n_subpixels(self) -> int:
        """of the unpadded images"""
        return self.layout.n_subpixels

    def bpd(self) -> float:
        """bits per sub-pixel of the unpadded images"""
        n = self.n_subpixels()
        return self.bits() / n if n else float("nan")


@dataclass
class TiledBitstream(_TiledSizes):
    stream: Bitstream           # N = sum of the images' tiles entries, one stream per (tile, level)
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)

    def bits(self) -> int:
        return self.stream.bits()

    def state_bits_per_subpixel(self) -> float:
        """The streams' final states (64 bits per (tile, level) and way) per unpadded
        sub-pixel; an image of full tiles pays 64 * ways * levels / (C * th * tw)."""
        n = self.n_subpixels()
        return 64 * int(self.stream.states.numel()) / n if n else float("nan")

    def padded_share(self) -> float:
        """The share of the coded pixels that is pad."""
        lay = self.layout
        coded = lay.n_tiles * lay.tile_hw[0] * lay.tile_hw[1]
        return 1.0 - sum(H * W for H, W in lay.sizes) / coded if coded else 0.0

    def to_bytes(self) -> bytes:
        inner = self.stream.to_bytes()
        return self.layout.pack(MAGIC) + struct.pack("<Q", len(inner)) + inner

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "TiledBitstream":
        lay, o = TileLayout.unpack(buf, MAGIC, "tiled bitstream", tail=8)
        (length,) = struct.unpack_from("<Q", buf, o)
        o += 8
        if len(buf) != o + length:
            raise ValueError(f"tiled bitstream holds {len(buf) - o} payload bytes, its header "
                             f"names {length}")
        try:
            stream = Bitstream.from_bytes(buf[o:], device)
        except struct.error as e:
            raise ValueError(f"truncated tiled bitstream ({e})") from None
        if stream.n_images != lay.n_tiles:
            raise ValueError(f"tiled bitstream of {lay.n_tiles} tiles holds {stream.n_images} "
                             "entries")
        return cls(stream, list(lay.sizes), lay.C, lay.tile_hw)


# ------------------------------------------------------------------ codec
class TiledCodec:
    """A list of uint8 images [C, H_i, W_i] of any sizes (layout="hwc": [H_i, W_i, C]) and any
    strides <-> TiledBitstream with an IDFlows.
    ways: interleaved rANS states per (tile, level) stream (codec.Bitstream.ways): a crop pays
    every touched tile's serial chain in full, ways times shorter for 64 (ways - 1) more bits
    per stream.  Decode follows the bitstream's own ways."""

    def __init__(self, model, max_batch: int = 256, ways: int = 1):
        from flows import ConditionalFlows, IDFlows
        if isinstance(model, ConditionalFlows):
            raise TypeError("TiledCodec: the condition of a ConditionalFlows is not built per "
                            "tile; use an IDFlows")
        if not isinstance(model, IDFlows):
            raise TypeError(f"TiledCodec takes an IDFlows, not {type(model).__name__}")
        model._check_batch_squeeze()
        max_batch = int(max_batch)
        if max_batch < 1:
            raise ValueError(f"max_batch {max_batch} must be at least 1")
        self.model = model
        self.max_batch = max_batch
        self.ways = check_ways(ways)
        self.C, self.tile_hw = model.C, (model.H, model.W)
        self._buf = None

    # -------------------------------------------------------------- encode
    def _sources(self, images, dev, layout=None):
        """images as encode takes them -> (their checked [C, H_i, W_i] views, their TileLayout,
        the table rows of their tiles: five fields where every image is dense planar, else
        eight)."""
        views = source_views(images, self.C, dev, layout)
        lay = TileLayout([v.shape[1:] for v in views], self.C, self.tile_hw)
        return views, lay, lay.rows([v.data_ptr() for v in views], view_strides(views))

    def _outputs(self, shapes, layout, out):
        """-> (the tensors a decode returns, their addresses, their strides or None): the
        arguments `place` takes."""
        outs, views = output_views(shapes, self._device(), layout, out)
        return outs, [v.data_ptr() for v in views], view_strides(views)

    @staticmethod
    def _device_table(rows, dev) -> torch.Tensor:
        """rows of five fields, or of eight -> device int64 [n, 5] or [n, 8]"""
        if not len(rows):
            return torch.zeros((0, 5), dtype=torch.int64, device=dev)
        tab = np.asarray(rows, dtype=np.int64).reshape(len(rows), -1)
        if tab.shape[1] not in (5, 8):
            raise ValueError(f"tile table rows have 5 or 8 fields, not {tab.shape[1]}")
        return dist._to_device(torch.from_numpy(tab), dev)  # pinned staging, no stream sync

    @torch.no_grad()
    def encode(self, images, layout=None) -> TiledBitstream:
        """images: a list of device uint8 tensors [C, H_i, W_i], or one [B, C, H, W] tensor;
        layout="hwc": [H_i, W_i, C] and [B, H, W, C].  With a layout named ("chw" or "hwc") any
        strides are taken and the bytes read where they lie; without one (None) the tensors are
        [C, H, W] and must be contiguous, as before."""
        ic = self.model.codec()
        eng = ic.engine
        dev = torch.device(eng.device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        # images: held until the last chunk's sync
        images, lay, rows = self._sources(images, dev, layout)
        C, (th, tw), N = self.C, self.tile_hw, lay.n_tiles
        table = self._device_table(rows, dev)
        px4 = th * tw * 4
        chunks = [(e0, min(self.max_batch, N - e0)) for e0 in range(0, N, self.max_batch)]

        def encode_chunk(e0, n):
            def fill():  # the source bytes straight into the engine's input
                ws = eng.workspace(n, 0)
                device_gather(table[e0:e0 + n], n, C, th, tw, ws["img"])
                return ws

            ws = fill()
            img = ws["img"]

            def lane_src(i, p0, m):  # an encode lane's tiles, read in place
                return img[p0 * px4:(p0 + m) * px4]

            # a flow only reads ws['img'], so the range guard's exact-f32 recompute finds it
            # intact; gather again only if the engine has dropped that workspace set meanwhile
            return ic._encode_guarded(lambda: ws if eng.workspace(n, 0) is ws else fill(),
                                      n, None, True, lane_src=lane_src, ways=self.ways)

        parts = [encode_chunk(e0, n) for e0, n in chunks]
        if len({p.meta["conv"] for p in parts}) > 1:
            # the range guard sent some chunk to the exact-f32 convs: one mode for all
            prev = eng.conv_mode
            eng.set_conv_mode("f32")
            try:
                parts = [p if p.meta["conv"] == "f32" else encode_chunk(e0, n)
                         for p, (e0, n) in zip(parts, chunks)]
            finally:
                eng.set_conv_mode(prev)
        return TiledBitstream(self._merge(parts, [n for _, n in chunks]), list(lay.sizes), C,
                              (th, tw))

    def _merge(self, parts, counts) -> Bitstream:
        """The chunks' Bitstreams (each level-major over its own entries) as one level-major
        Bitstream over all entries."""
        N = sum(counts)
        meta = {"n_subpixels": N * self.C * self.tile_hw[0] * self.tile_hw[1],
                "conv": parts[0].meta["conv"]}
        if len(parts) == 1:
            p = parts[0]
            return Bitstream(N, p.level_shapes, p.states, p.nwords, p.words, p.status, meta,
                             p.host_nwords, ways=p.ways)
        n_lvl = len(parts[0].level_shapes)
        nw_h = torch.cat([p.nwords_host() for p in parts])
        st, nw, w = dist.interleave_levels(
            torch.cat([p.states for p in parts]), torch.cat([p.nwords for p in parts]),
            torch.cat([p.words for p in parts]), len(parts), n_lvl, list(counts),
            total=int(nw_h.sum()), ways=parts[0].ways)
        idx = torch.tensor(dist._interleave_idx(list(counts), n_lvl), dtype=torch.int64)
        status = torch.cat([p.status for p in parts])[idx.to(st.device)]
        return Bitstream(N, parts[0].level_shapes, st, nw, w, status, meta, nw_h[idx],
                         ways=parts[0].ways)

    # -------------------------------------------------------------- decode
    def check_bitstream(self, tbs: TiledBitstream):
        if (tbs.C, tuple(tbs.tile_hw)) != (self.C, self.tile_hw):
            raise ValueError(f"tiled bitstream of C {tbs.C}, tiles {tuple(tbs.tile_hw)} does not "
                             f"match the model's C {self.C}, input {self.tile_hw}")
        N = tbs.layout.n_tiles
        if tbs.stream.n_images != N or tbs.stream.group != 1:
            raise ValueError(f"tiled bitstream of {N} tiles holds {tbs.stream.n_images} entries "
                             f"in stream groups of {tbs.stream.group}")

    def _device(self) -> torch.device:
        """The engine's device, without the engine: IDFlows.codec() walks every parameter to see
        whether the engine is current (1.7 ms for imagenet64's 1 404 tensors), so a decode call
        looks it up once, in _decode_entries, and not at all where no flow runs."""
        return next(self.model.parameters()).device

    def _chunks(self, ic, stream: Bitstream, entries):
        """Decodes entries `entries` of stream with the ImageCodec ic, at most max_batch at a
        time.  Yields (k, m, info): the pixel-major rows of tiles entries[k:k + m] fill the
        start of self._buf, info is their decode's."""
        n, px4 = len(entries), self.tile_hw[0] * self.tile_hw[1] * 4
        m_max = min(n, self.max_batch)
        if self._buf is None or self._buf.numel() < m_max * px4:
            self._buf = torch.empty(m_max * px4, dtype=torch.float32, device=ic.engine.device)
        whole = entries == list(range(stream.n_images)) and n <= self.max_batch
        for k in range(0, n, self.max_batch):
            m = min(self.max_batch, n - k)
            sub = stream if whole else stream.select(entries[k:k + m])
            yield k, m, ic.decode_into(sub, self._buf[:m * px4])

    def _decode_tiles(self, ic, stream: Bitstream, entries, rows, verify: bool, seal=None):
        """Decodes entries `entries` of stream with the ImageCodec ic and scatters tile k into
        the buffer rows[k] names (addr, H, W, y0, x0).  seal: a sealed file's check
        (idfcodec.integrity), shown every chunk's rows where the scatter reads them."""
        dev = ic.engine.device
        C, (th, tw) = self.C, self.tile_hw
        table = self._device_table(rows, dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        states, status = [], []
        for k, m, part in self._chunks(ic, stream, entries):
            device_scatter(table[k:k + m], m, C, th, tw, self._buf, bad)
            if seal is not None:
                seal.kept_chunk(k, m, self._buf)
            states.append(part["final_states"])
            status.append(part["status"])
        if not states:  # decode(images=[])
            states = [torch.zeros(0, dtype=torch.int64, device=dev)]
            status = [torch.zeros(0, dtype=torch.int32, device=dev)]
        # per chunk of at most max_batch entries, level-major within the chunk
        info = {"final_states": torch.cat(states), "status": torch.cat(status),
                "off_grid": bad, "tiles": len(entries)}
        if verify:
            info["ok"] = int(bad.item()) == 0 and streams_ok(info["final_states"], info["status"])
        return info

    def _decode_entries(self, tbs: TiledBitstream, entries, rows, verify: bool, seal=None):
        """Entries `entries` of tbs into the buffers rows[k] names; -> the decode info."""
        return self._decode_tiles(self._codec_for(seal), tbs.stream, entries, rows, verify, seal)

    def _codec_for(self, seal):
        """The model's ImageCodec; a seal that has looked it up already brings it along."""
        ic = seal.ic if seal is not None else None
        return ic if ic is not None else self.model.codec()

    @torch.no_grad()
    def decode(self, tbs, images=None, verify: bool = True, layout: str = "chw", out=None):
        """-> (list of uint8 [C, H_i, W_i], info).  images: the indices of the images to
        decode (default: all), returned in the order asked; only their tiles are decoded.
        layout="hwc": [H_i, W_i, C].  out: a list of the caller's tensors to decode into, one
        per image asked, in `layout`, of any strides that address no byte twice; it is what is
        returned, and no other byte of it is written."""
        self.check_bitstream(tbs)
        lay = tbs.layout
        want, entries, rows = lay.image_rows(images)
        outs, addrs, strides = self._outputs([(self.C, *lay.sizes[i]) for i in want], layout, out)
        return outs, self._decode_entries(tbs, entries, lay.place(rows, addrs, strides), verify)

    @torch.no_grad()
    def decode_region(self, tbs, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True, layout: str = "chw", out=None):
        """-> (uint8 [C, h, w], info): rows [y0, y0 + h) x columns [x0, x0 + w) of one image,
        from exactly the tiles that intersect them (info['tiles']).  layout, out: as decode's,
        out one tensor of the region's size."""
        self.check_bitstream(tbs)
        lay = tbs.layout
        entries, rows = lay.region_rows(image, y0, x0, h, w)
        outs, addrs, strides = self._outputs([(self.C, int(h), int(w))], layout,
                                             None if out is None else [out])
        return outs[0], self._decode_entries(tbs, entries, lay.place(rows, addrs, strides),
                                             verify)


__all__ = ["MAGIC", "VERSION", "LAYOUTS", "Reader", "TileLayout", "TiledBitstream", "TiledCodec",
           "as_chw", "check_layout", "check_no_overlap", "device_gather", "device_scatter",
           "is_dense_planar", "output_views", "pack_bitmap", "pack_lengthed", "pack_words",
           "planes", "read_words", "region_tiles", "source_views", "tile_table", "tiles_host",
           "view_strides"]
