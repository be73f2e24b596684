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

All chunks of one bitstream are coded in one conv mode: if the split-f16 range guard sent any
chunk to exact-f32 convs, the others are re-encoded in "f32" and the bitstream records "f32".

Container IDFT (little-endian): magic "IDFT", u16 version 1, u16 flags 0, u32 n_images, u32 C,
u32 tile_h, u32 tile_w, n_images x (u32 H, u32 W), u64 byte length, the inner IDFB container
(codec.Bitstream.to_bytes; its n_images field holds N).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import RANS_L, Bitstream, check_ways

MAGIC = b"IDFT"
VERSION = 1
_HDR = "<4sHHIIII"


# ------------------------------------------------------------------ host arithmetic
def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def tile_table(sizes, th: int, tw: int):
    """sizes: [(H, W)] per image -> (tiles per image, [(image, ty, tx)] in entry order: by
    image, then tile row, then tile column).  Pure host arithmetic."""
    th, tw = int(th), int(tw)
    if th < 1 or tw < 1:
        raise ValueError(f"tile size {(th, tw)} must be positive")
    counts, entries = [], []
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"image {i} has a zero-sized dimension {(H, W)}")
        nh, nw = _ceil_div(H, th), _ceil_div(W, tw)
        counts.append(nh * nw)
        entries += [(i, ty, tx) for ty in range(nh) for tx in range(nw)]
    return counts, entries


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
    (n,), _ = tile_table([(H, W)], th, tw)
    nh, nw = _ceil_div(H, th), _ceil_div(W, tw)
    ys = np.minimum(np.arange(nh * th), H - 1)
    xs = np.minimum(np.arange(nw * tw), W - 1)
    p = img[:, ys][:, :, xs]
    return p.reshape(C, nh, th, nw, tw).transpose(1, 3, 0, 2, 4).reshape(n, C, th, tw)


# ------------------------------------------------------------------ device calls
def _check_table(table: torch.Tensor, n: int):
    _lib.require_device(table, "tile table")
    if table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < n * 5:
        raise ValueError("tile table must be contiguous int64 [n_tiles, 5]")


def device_gather(table: torch.Tensor, n: int, C: int, th: int, tw: int, out: torch.Tensor,
                  ld: int = 4):
    """table: device int64 [>= n, 5] rows (addr, H, W, y0, x0) -> out, the pixel-major (ld)
    float32 rows of n tiles (idf_tile_gather_u8)."""
    _check_table(table, n)
    _lib.require_device(out, "tile buffer")
    if out.dtype != torch.float32 or out.numel() < n * th * tw * ld:
        raise ValueError("gather output must be float32 and hold n * th * tw * ld values")
    check(lib().idf_tile_gather_u8(_lib.stream_ptr(out.device), n, C, th, tw, ptr(table),
                                   ptr(out), ld), "tile gather")


def device_scatter(table: torch.Tensor, n: int, C: int, th: int, tw: int, src: torch.Tensor,
                   bad: torch.Tensor, ld: int = 4):
    """The pixel-major rows of n tiles -> the uint8 buffers the table names
    (idf_tile_scatter_u8); bad: int32[1], the off-grid count of the pixels written."""
    _check_table(table, n)
    _lib.require_device(src, "tile buffer")
    _lib.require_device(bad, "off-grid counter")
    if src.dtype != torch.float32 or src.numel() < n * th * tw * ld:
        raise ValueError("scatter input must be float32 and hold n * th * tw * ld values")
    if bad.dtype != torch.int32 or bad.numel() < 1:
        raise ValueError("the off-grid counter is int32[1]")
    check(lib().idf_tile_scatter_u8(_lib.stream_ptr(src.device), n, C, th, tw, ptr(src), ld,
                                    ptr(table), ptr(bad)), "tile scatter")


# ------------------------------------------------------------------ container
@dataclass
class TiledBitstream:
    stream: Bitstream           # N = sum of the images' tiles entries, one stream per (tile, level)
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)

    @property
    def n_images(self) -> int:
        return len(self.sizes)

    def tile_counts(self) -> list:
        return tile_table(self.sizes, *self.tile_hw)[0]

    def n_subpixels(self) -> int:
        """of the unpadded images"""
        return sum(self.C * int(H) * int(W) for H, W in self.sizes)

    def bits(self) -> int:
        return self.stream.bits()

    def bpd(self) -> float:
        """bits per sub-pixel of the unpadded images"""
        n = self.n_subpixels()
        return self.bits() / n if n else float("nan")

    def state_bits_per_subpixel(self) -> float:
        """The streams' final states (64 bits per (tile, level) and way) per unpadded
        sub-pixel; an image of full tiles pays 64 * ways * levels / (C * th * tw)."""
        n = self.n_subpixels()
        return 64 * int(self.stream.states.numel()) / n if n else float("nan")

    def padded_share(self) -> float:
        """The share of the coded pixels that is pad."""
        th, tw = self.tile_hw
        coded = sum(self.tile_counts()) * th * tw
        return 1.0 - sum(int(H) * int(W) for H, W in self.sizes) / coded if coded else 0.0

    def to_bytes(self) -> bytes:
        inner = self.stream.to_bytes()
        hdr = struct.pack(_HDR, MAGIC, VERSION, 0, len(self.sizes), self.C, *self.tile_hw)
        sizes = b"".join(struct.pack("<II", int(H), int(W)) for H, W in self.sizes)
        return hdr + sizes + struct.pack("<Q", len(inner)) + inner

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "TiledBitstream":
        n_hdr = struct.calcsize(_HDR)
        if len(buf) < n_hdr:
            raise ValueError("truncated tiled bitstream (header)")
        magic, ver, flags, n, C, th, tw = struct.unpack_from(_HDR, buf, 0)
        if magic != MAGIC:
            raise ValueError("not an IDF tiled bitstream")
        if ver != VERSION:
            raise ValueError(f"unknown tiled bitstream version {ver}")
        if flags:
            raise ValueError(f"unknown tiled bitstream flags {flags:#x}")
        if min(n, C, th, tw) < 1:
            raise ValueError("tiled bitstream header holds a zero size")
        o = n_hdr + 8 * n
        if len(buf) < o + 8:
            raise ValueError("truncated tiled bitstream (image sizes)")
        sizes = [struct.unpack_from("<II", buf, n_hdr + 8 * i) for i in range(n)]
        if any(min(s) < 1 for s in sizes):
            raise ValueError("tiled bitstream holds an image with a zero size")
        (length,) = struct.unpack_from("<Q", buf, o)
        o += 8
        if len(buf) != o + length:
            raise ValueError(f"tiled bitstream holds {len(buf) - o} payload bytes, its header "
                             f"names {length}")
        try:
            stream = Bitstream.from_bytes(buf[o:], device)
        except struct.error as e:
            raise ValueError(f"truncated tiled bitstream ({e})") from None
        N = sum(tile_table(sizes, th, tw)[0])
        if stream.n_images != N:
            raise ValueError(f"tiled bitstream of {N} tiles holds {stream.n_images} entries")
        return cls(stream, [tuple(s) for s in sizes], C, (th, tw))


# ------------------------------------------------------------------ codec
class TiledCodec:
    """A list of uint8 images [C, H_i, W_i] of any sizes <-> TiledBitstream with an IDFlows.
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
    def _image_list(self, images, dev):
        C = self.C
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise ValueError("images: a list of [C, H, W] tensors or one [B, C, H, W] tensor")
            if not images.is_contiguous():
                raise ValueError("the image batch is not contiguous")
            images = [images[i] for i in range(images.shape[0])]
        images = list(images)
        if not images:
            raise ValueError("no images to encode")
        for i, t in enumerate(images):
            if not isinstance(t, torch.Tensor) or t.dim() != 3:
                raise ValueError(f"image {i} is no [C, H, W] tensor")
            if t.dtype != torch.uint8:
                raise ValueError(f"image {i} is {t.dtype}, not uint8")
            if t.device != dev:
                raise ValueError(f"image {i} lies on {t.device}, the engine on {dev}")
            if t.shape[0] != C:
                raise ValueError(f"image {i} has {t.shape[0]} channels, the model {C}")
            if t.shape[1] < 1 or t.shape[2] < 1:
                raise ValueError(f"image {i} has a zero-sized dimension {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"image {i} is not contiguous")
        return images

    @staticmethod
    def _device_table(rows, dev) -> torch.Tensor:
        from .dist import _to_device
        tab = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
        if not len(tab):
            return torch.zeros((0, 5), dtype=torch.int64, device=dev)
        return _to_device(torch.from_numpy(tab), dev)  # pinned staging, no stream sync

    @torch.no_grad()
    def encode(self, images) -> TiledBitstream:
        """images: a list of device uint8 tensors [C, H_i, W_i], or one [B, C, H, W] tensor."""
        ic = self.model.codec()
        eng = ic.engine
        dev = torch.device(eng.device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        images = self._image_list(images, dev)  # held until the last chunk's sync
        C, (th, tw) = self.C, self.tile_hw
        sizes = [(int(t.shape[1]), int(t.shape[2])) for t in images]
        counts, entries = tile_table(sizes, th, tw)
        N = len(entries)
        table = self._device_table(
            [(images[i].data_ptr(), *sizes[i], ty * th, tx * tw) for i, ty, tx in entries], dev)
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
        return TiledBitstream(self._merge(parts, [n for _, n in chunks]), sizes, C, (th, tw))

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
        from . import dist
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
        N = sum(tbs.tile_counts())
        if tbs.stream.n_images != N or tbs.stream.group != 1:
            raise ValueError(f"tiled bitstream of {N} tiles holds {tbs.stream.n_images} entries "
                             f"in stream groups of {tbs.stream.group}")

    def _decode_tiles(self, ic, tbs: TiledBitstream, entries, rows, verify: bool):
        """Decodes entries `entries` of tbs with the ImageCodec ic and scatters tile k into the
        buffer rows[k] names (addr, H, W, y0, x0)."""
        eng = ic.engine
        dev = eng.device
        C, (th, tw) = self.C, self.tile_hw
        n, px4 = len(entries), th * tw * 4
        m_max = min(n, self.max_batch)
        if self._buf is None or self._buf.numel() < m_max * px4:
            self._buf = torch.empty(m_max * px4, dtype=torch.float32, device=dev)
        buf = self._buf
        whole = entries == list(range(tbs.stream.n_images)) and n <= self.max_batch
        nothing = lambda i, b0, m, ws: None  # noqa: E731  (the lanes write into buf)
        states, status = [], []
        table = self._device_table(rows, dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        for k in range(0, n, self.max_batch):
            m = min(self.max_batch, n - k)
            sub = tbs.stream if whole else tbs.stream.select(entries[k:k + m])
            part = ic._decode_lanes(sub, None, nothing, img_out=buf[:m * px4])
            device_scatter(table[k:k + m], m, C, th, tw, buf, bad)
            states.append(part["final_states"])
            status.append(part["status"])
        if not states:  # decode(images=[])
            states = [torch.zeros(0, dtype=torch.int64, device=dev)]
            status = [torch.zeros(0, dtype=torch.int32, device=dev)]
        # per chunk of at most max_batch entries, level-major within the chunk
        info = {"final_states": torch.cat(states), "status": torch.cat(status),
                "off_grid": bad, "tiles": n}
        if verify:
            ok = int(bad.item()) == 0 and bool((info["final_states"] == RANS_L).all().item())
            info["ok"] = ok and not bool(
                (info["status"] & ~_lib.STREAM_WORDS_LEFT).any().item())
        return info

    @torch.no_grad()
    def decode(self, tbs: TiledBitstream, images=None, verify: bool = True):
        """-> (list of uint8 [C, H_i, W_i], info).  images: the indices of the images to
        decode (default: all), returned in the order asked; only their tiles are decoded."""
        self.check_bitstream(tbs)
        th, tw = self.tile_hw
        counts = tbs.tile_counts()
        first = [0]
        for c in counts:
            first.append(first[-1] + c)
        want = list(range(len(counts))) if images is None else [int(i) for i in images]
        for i in want:
            if not 0 <= i < len(counts):
                raise ValueError(f"image {i} is outside the bitstream's {len(counts)} images")
        # looked up once: IDFlows.codec() walks every parameter to see whether the engine is
        # current (1.7 ms for imagenet64's 1 404 tensors)
        ic = self.model.codec()
        dev = ic.engine.device
        outs, entries, rows = [], [], []
        for i in want:
            H, W = tbs.sizes[i]
            out = torch.empty((self.C, H, W), dtype=torch.uint8, device=dev)
            outs.append(out)
            nw = _ceil_div(W, tw)
            for j in range(counts[i]):
                entries.append(first[i] + j)
                rows.append((out.data_ptr(), H, W, (j // nw) * th, (j % nw) * tw))
        info = self._decode_tiles(ic, tbs, entries, rows, verify)
        return outs, info

    @torch.no_grad()
    def decode_region(self, tbs: TiledBitstream, image: int, y0: int, x0: int, h: int, w: int,
                      verify: bool = True):
        """-> (uint8 [C, h, w], info): rows [y0, y0 + h) x columns [x0, x0 + w) of one image,
        from exactly the tiles that intersect them (info['tiles'])."""
        self.check_bitstream(tbs)
        image = int(image)
        if not 0 <= image < tbs.n_images:
            raise ValueError(f"image {image} is outside the bitstream's {tbs.n_images} images")
        th, tw = self.tile_hw
        H, W = tbs.sizes[image]
        tiles = region_tiles((H, W), y0, x0, h, w, th, tw)
        first = sum(tbs.tile_counts()[:image])
        nw = _ceil_div(W, tw)
        ic = self.model.codec()
        out = torch.empty((self.C, int(h), int(w)), dtype=torch.uint8, device=ic.engine.device)
        entries = [first + ty * nw + tx for ty, tx in tiles]
        rows = [(out.data_ptr(), int(h), int(w), ty * th - int(y0), tx * tw - int(x0))
                for ty, tx in tiles]
        info = self._decode_tiles(ic, tbs, entries, rows, verify)
        return out, info


__all__ = ["MAGIC", "VERSION", "TiledBitstream", "TiledCodec", "device_gather", "device_scatter",
           "region_tiles", "tile_table", "tiles_host"]
