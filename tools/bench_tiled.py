"""Images of any size through the tiled codec (idfcodec.tiled) on one GPU: a benchmark and the
file tool.

  python tools/bench_tiled.py bench [--steps K] [--warmup W] [--seal]
                                    [--escape [--predict [--predict-ways N [N ...]]
                                                         [--smallest]]]
  python tools/bench_tiled.py bench --channels N [--steps K] [--warmup W] [--escape [--predict]]
  python tools/bench_tiled.py compress OUT FILE... [--config NAME|YAML] [--checkpoint PT]
                                                   [--ways 1|8|16|32|64]
                                                   [--seal]  (with every combination below)
                                                   [--escape [--max-ratio R] [--check status|decode]
                                                             [--predict [--colour]
                                                              [--predict-ways 1|8|16|32|64]
                                                              [--smallest [--no-shortlist]]]]
  python tools/bench_tiled.py decompress IN DIR    [--config NAME|YAML] [--checkpoint PT]
  python tools/bench_tiled.py verify IN            [--config NAME|YAML] [--checkpoint PT]

bench: the imagenet64 model with seeded synthetic weights (no checkpoint exists), synthetic
uint8 images resident in HBM.  Set (a): 4 images of 512x512 = 256 full tiles, the batch of
bench.py.  Set (b): a ragged set, 500x375, 640x427, 64x64 and 33x70.  One step = TiledCodec.encode
then decode.  For (a) the plain model.encode / model.decode of the same 256 tiles as a
[256, 3, 64, 64] batch is timed in the same process, the two paths alternating step by step: the
plain codec is existing code and the yardstick, and its own spread over the steps says how small
a difference between the two can be told.  Prints one JSON line: per path the median, minimum
and maximum ms of encode and decode over the steps, Mpx/s of source pixels, the exactness of
every timed round trip, the padded-pixel share, the state bits per sub-pixel, and the device
time of the gather / scatter kernels beside idf_dequant_u8 / idf_quant_u8 on the same pixel
count.  kernels_by_layout, for both sets: the device time of the five kernels that touch a
caller's image (gather, scatter, raw gather, raw scatter, tile CRC) over the same tiles in three
memory shapes -- dense planar (the five-field table), dense HWC and planar rows with a pitch (the
eight-field table with strides).  With random weights and random pixels the bits per sub-pixel
say nothing about a trained model.

--escape (idfcodec.safe.SafeTiledCodec, container IDFS): every tile is coded by the flow or, where
its streams would not decode to the source or would cost more than --max-ratio (default 1.0) times
its bytes, stored raw; the file then always decodes to the source and, at a ratio <= 1, is at most
the source plus its headers.  decompress picks the codec by the file's magic.  bench --escape adds,
for both sets, SafeTiledCodec at max_ratio 1.0 and inf, stepped alternately with the rows above in
the same process, and the three escape kernels' device times.

--escape --predict (idfcodec.predict.PredictiveTileCodec, container IDFP): the escaped tiles are
coded on the device by a MED predictor and rANS, and stored that way where it is smaller than
their bytes.  bench --escape --predict adds, for both sets, that codec at max_ratio 1.0 stepped
alternately with the other rows (encode / decode ms, tiles raw / packed / kept, file bytes over
source bytes), a set (c) of smooth images (ramps plus noise 0..3) through SafeTiledCodec and
PredictiveTileCodec, and the device time of idf_predict_prep_u8 and idf_predict_decode_u8 beside
idf_tile_gather_raw_u8 and beside idf_rans_decode_streams on the very same streams.

compress --escape --predict --colour (PredictiveTileCodec(colour=True), container IDFQ): every
escaped tile is also coded with planes 0 and 2 as differences to plane 1 and the smaller coding is
kept.  bench --escape --predict adds a set (d) of correlated images (per tile a shared luminance
with small chroma offsets): the IDFS size, the IDFP and the IDFQ codec alternating step by step
(sizes, encode / decode ms, tiles raw / packed / colour), and the device time of
idf_predict_prep2_u8 beside idf_predict_prep_u8, of idf_predict_decode2_u8 on the colour and on
the plain streams beside idf_predict_decode_u8 on the latter, and of the inverse transform.

--predict-ways N (PredictiveTileCodec(predict_ways=N)): every predictive stream is coded by N
interleaved states, its symbols ordered along a pixel wavefront, so that one wave decodes up to N
pixels a step; decompress reads N from the file.  bench --escape --predict --predict-ways N [N ...]
steps, in sets (a), (b) and (c), the codec at each N beside the one-way codec (the unchanged
idf_predict_decode_u8, the baseline) in the same loop, and adds per N the device time of the prep
and decode kernels over all tiles of (a) and (c), ns per symbol per wave, and -- the number the
ways exist for -- the latency of decoding ONE full packed entry: decode_region inside one tile of
a smooth image, wall clock, and the decode kernel alone on that entry, by events.

--smallest (PredictiveTileCodec.encode(choose="smallest")): every tile is stored in the smallest
of its three codings; idf_predict_cost_u8 prices the predictor on every tile and only the tiles it
may win are coded (--no-shortlist: all).  The files are ordinary IDFP / IDFQ files.  compress
prints per tile the flow's bytes, the estimate, the predictor's bytes and the choice.  bench
--escape --predict --smallest steps, in sets (a), (b) and (c), choose="smallest" with the
shortlist (smallest_ratio_1) and without (smallest_all_ratio_1) beside choose="escaped"
(predict_ratio_1): encode / decode ms, tiles kept / packed / raw / moved off the flow / coded by
the predictor, file bytes.  The kernels of --predict always include idf_predict_cost_u8 beside
prep + encode + gather over the same tiles, and the estimate's gap to the coder in words.

--seal (idfcodec.integrity.SealedCodec, container IDFC around the IDFT or IDFS file, with
--escape --predict [--colour] [--predict-ways N] [--smallest] around the IDFP / IDFQ file): a
CRC-32 of every tile's source bytes, computed on the device, and the model's fingerprint.
decompress reads such a file by its magic and its inner file's, refuses one written by other
weights and names the damaged tiles.  verify decodes a sealed file, prints each damaged tile as
(image, tile row, tile column), writes nothing and exits 1 if a tile is damaged or the model does
not match.  bench --seal adds, for both sets, the sealed codecs stepped alternately with their
unsealed ones in the same process, the three CRC kernels' device times and the fingerprint's
one-off cost; with --escape --predict [--smallest] also, in sets (a), (b) and (c), the sealed
predictive codec (sealed_predict_ratio_1, sealed_smallest_ratio_1) beside predict_ratio_1 and
smallest_ratio_1.

Plane sets (idfcodec.planes.PlaneSetCodec, container IDFM): compress takes sources of another
channel count than the model's -- a PGM (grey), a .npy of 1, 2, 4 or more channels (grey + alpha,
RGBA, ...); every file of one call the same count -- and writes an IDFM file around the file the
flags above name: the model's first C channels go to that codec, the others are extra planes,
each tile's stored as one byte where it is constant, else coded by the predictor (--predict-ways
applies) or stored raw; with fewer channels than C all are extra planes and no flow runs.  --seal
with such sources exits with the codec's refusal (a seal would not cover the extra planes).
Files of the model's own channel count keep their path and their bytes.  decompress reads an IDFM
file by its magic and its base by its own.  bench --channels N [--escape [--predict]]: 4 sources
of 512x512 and N channels (the flow's planes noise, the others smooth), once with an opaque alpha
and once with a disc, through model.tiled_planes over the base the flags name and, step by step
beside it, that base alone over the same base planes: encode / decode ms and Mpx/s, the units per
class, the file's bytes and the extra planes' share of them.

16-bit sources (.npy of uint16; binary P5 / P6 with maxval 256..65535, whose big-endian samples
are swapped on the host) go through idfcodec.deep's DeepTiledCodec instead, no model: compress
writes an IDFD file, decompress reads it by its magic and writes PGM / PPM with maxval 65535.
bench --deep: four seeded 512 x 512 16-bit images: bits per sample, the class shares, the shifts,
the escape count, encode and decode Mpx/s, and the device time of idf_deep_decode_u16 beside
idf_predict_decode_u8 at one way on the high bytes of the same tiles.  compress --deep-ways N
writes units of N interleaved states; bench --deep --deep-ways 8 16 32 64 steps those codecs
beside the one-way codec, alternating step by step: file bytes, encode and decode ms, the decode
kernel's device time with every unit decoded as packed and the decode_region latency of one unit.

compress / decompress: inputs are .npy (uint8, HWC or CHW, or HW) or binary PPM / PGM (P6 / P5,
maxval <= 255).  A file's pixel bytes are uploaded as they are stored and coded with
layout="hwc" (a planar .npy as a permuted view): the kernels read interleaved pixels in place, and
the decode writes them interleaved, so no image is transposed on the host.  decompress writes
image_0000.ppm (.pgm for one channel, .npy otherwise) ... into DIR.  Without --checkpoint the seeded synthetic weights are used: they round-trip exactly but do
not compress.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "finalproject-losslessimagecompression_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

RAGGED = ((500, 375), (640, 427), (64, 64), (33, 70))


# ------------------------------------------------------------------ bench
def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _stats(ms, px):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "mpx_s": round(px / med / 1e3, 3)}


def _tables(tc, imgs):
    """-> (the TileLayout of imgs, its device table over imgs, empty outputs of their sizes, the
    table over those)."""
    from idfcodec.tiled import TileLayout
    lay = TileLayout([t.shape[1:] for t in imgs], tc.C, tc.tile_hw)
    outs = [torch.empty_like(t) for t in imgs]
    return (lay, tc._device_table(lay.rows([t.data_ptr() for t in imgs]), imgs[0].device), outs,
            tc._device_table(lay.rows([t.data_ptr() for t in outs]), imgs[0].device))


def _kernel_times(tc, imgs, reps: int = 20) -> dict:
    """Device time (events) of the two index kernels over all tiles of imgs, and of
    idf_dequant_u8 / idf_quant_u8 on the same number of pixels."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    from idfcodec.tiled import device_gather, device_scatter
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, outs, otab = _tables(tc, imgs)
    n = lay.n_tiles
    buf = torch.empty(n * th * tw * 4, dtype=torch.float32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = _lib.stream_ptr(torch.device("cuda"))
    flat = torch.zeros((n, C, th, tw), dtype=torch.uint8, device="cuda")
    runs = {  # in this order: the scatter, last, writes what the gather read
        "dequant_u8": lambda: check(lib().idf_dequant_u8(s, n, C, th, tw, ptr(flat), ptr(buf), 4)),
        "quant_u8": lambda: check(lib().idf_quant_u8(s, n, C, th, tw, ptr(buf), 4, ptr(flat),
                                                     ptr(bad))),
        "tile_gather_u8": lambda: device_gather(table, n, C, th, tw, buf),
        "tile_scatter_u8": lambda: device_scatter(otab, n, C, th, tw, buf, bad),
    }
    out = {"tiles": n}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
    assert all(torch.equal(o, t) for o, t in zip(outs, imgs))
    return out


def _as_layout(imgs, kind: str):
    """The planar images imgs in another memory shape -> ([C, H, W] views of copies of them, views
    of the same shape to decode into): "planar" dense [C, H, W], "hwc" dense [H, W, C], "pitched"
    planar rows of W + 5 bytes inside a larger buffer."""
    def make(t, fill):
        C, H, W = t.shape
        if kind == "planar":
            buf = torch.empty((C, H, W), dtype=torch.uint8, device=t.device)
            v = buf
        elif kind == "hwc":
            buf = torch.empty((H, W, C), dtype=torch.uint8, device=t.device)
            v = buf.permute(2, 0, 1)
        else:
            buf = torch.empty((C, H + 1, W + 5), dtype=torch.uint8, device=t.device)
            v = buf[:, :H, 2:2 + W]
        if fill:
            v.copy_(t)
        return v
    return [make(t, True) for t in imgs], [make(t, False) for t in imgs]


def _layout_kernel_times(tc, imgs, reps: int = 20) -> dict:
    """Device time (events) of the five kernels that touch a caller's image -- gather, scatter,
    raw gather, raw scatter, tile CRC -- over all tiles of imgs, per memory shape of the same
    pixels: "planar" (five-field rows, the planar entry points), "hwc" and "pitched" (eight-field
    rows, the strided ones; _as_layout).  Every scatter is checked against the source and every
    CRC against the planar one."""
    from idfcodec.integrity import device_tile_crc32
    from idfcodec.safe import device_gather_raw, device_scatter_raw, raw_offsets
    from idfcodec.tiled import TileLayout, device_gather, device_scatter, view_strides
    th, tw = tc.tile_hw
    C, dev = tc.C, imgs[0].device
    lay = TileLayout([t.shape[1:] for t in imgs], C, tc.tile_hw)
    n, rects = lay.n_tiles, lay.rects
    offs, n_raw = raw_offsets([True] * n, rects, C)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    raw = torch.empty(n_raw, dtype=torch.uint8, device=dev)
    buf = torch.empty(n * th * tw * 4, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out, crcs = {"tiles": n}, {}
    for kind in ("planar", "hwc", "pitched"):
        src, dst = _as_layout(imgs, kind)
        table, otab = (tc._device_table(lay.rows([v.data_ptr() for v in vs], view_strides(vs)),
                                        dev) for vs in (src, dst))
        crcs[kind] = torch.empty(n, dtype=torch.int32, device=dev)
        runs = {  # the gathers first: the scatters write what they read
            "tile_gather": lambda: device_gather(table, n, C, th, tw, buf),
            "tile_gather_raw": lambda: device_gather_raw(table, n, C, th, tw, d_off, raw),
            "tile_crc32": lambda: device_tile_crc32(table, n, C, th, tw, crcs[kind]),
            "tile_scatter": lambda: device_scatter(otab, n, C, th, tw, buf, bad),
            "tile_scatter_raw": lambda: device_scatter_raw(otab, n, C, th, tw, raw, d_off, d_rect),
        }
        row = {"table_fields": int(table.shape[1])}
        for name, fn in runs.items():
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            row[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
            if "scatter" in name:
                assert all(torch.equal(o, t) for o, t in zip(dst, imgs)), (kind, name)
                for o in dst:
                    o.zero_()
        assert torch.equal(crcs[kind], crcs["planar"]) and int(bad.item()) == 0, kind
        out[kind] = row
    return out


def _escape_kernel_times(tc, imgs, reps: int = 20) -> dict:
    """Device time (events) of the three escape kernels over all tiles of imgs: the raw gather,
    the raw scatter of what it stored, and the verify of the gathered tiles against the source."""
    from idfcodec.safe import device_gather_raw, device_scatter_raw, device_verify, raw_offsets
    from idfcodec.tiled import device_gather
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, outs, otab = _tables(tc, imgs)
    n, rects = lay.n_tiles, lay.rects
    dev = imgs[0].device
    offs, n_raw = raw_offsets([True] * n, rects, C)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    raw = torch.empty(n_raw, dtype=torch.uint8, device=dev)
    buf = torch.empty(n * th * tw * 4, dtype=torch.float32, device=dev)
    device_gather(table, n, C, th, tw, buf)
    mism = torch.zeros(n, dtype=torch.int32, device=dev)
    runs = {
        "tile_gather_raw_u8": lambda: device_gather_raw(table, n, C, th, tw, d_off, raw),
        "tile_scatter_raw_u8": lambda: device_scatter_raw(otab, n, C, th, tw, raw, d_off, d_rect),
        "tile_verify_u8": lambda: device_verify(table, n, C, th, tw, buf, mism),
    }
    out = {}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
    assert all(torch.equal(o, t) for o, t in zip(outs, imgs)) and int(mism.abs().sum()) == 0
    return out


def _predict_kernel_times(tc, imgs, reps: int = 5) -> dict:
    """Device time (events, back-to-back launches) of the predictive coder's two kernels over
    all tiles of imgs, one stream per tile: idf_predict_prep_u8, idf_predict_decode_u8 and, on
    the very same streams (their words, means and scales), idf_rans_decode_streams -- the flow's
    decoder, which is handed every symbol's mean and scale and so runs its table producer."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    from idfcodec import predict as pr
    from idfcodec.safe import device_gather_raw
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, _, _ = _tables(tc, imgs)
    n, rects = lay.n_tiles, lay.rects
    dev = imgs[0].device
    counts = pr.entry_bytes(rects, C)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    nsym = int(off_h[-1])
    off = torch.from_numpy(off_h).to(dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    x, mean, scale = (torch.empty(nsym, dtype=torch.float32, device=dev) for _ in range(3))
    sel_h, states, nw, status, words = pr.device_predict_encode(table, counts, C, th, tw)
    assert not status.any()
    w_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    d_woff, d_nw, d_st = t64(w_off[:n]), t64(nw), t64(states)
    d_sel = torch.from_numpy(sel_h.view(np.int32).copy()).to(dev)
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    raw = torch.empty(nsym, dtype=torch.uint8, device=dev)
    want = torch.empty(nsym, dtype=torch.uint8, device=dev)
    device_gather_raw(table, n, C, th, tw, off[:n].contiguous(), want)
    final = torch.empty(n, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    xo = torch.empty(nsym, dtype=torch.float32, device=dev)
    wsb = int(lib().idf_rans_decode_workspace_bytes(nsym))
    wsp = torch.empty(wsb, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)

    def shape(v, fn):  # the decoder's other search shapes (timing only; the launcher reads this)
        os.environ["IDF_PREDICT_SEARCH"] = v
        try:
            fn()
        finally:
            del os.environ["IDF_PREDICT_SEARCH"]

    runs = {
        "predict_prep_u8": lambda: pr.device_predict_prep(table, n, C, th, tw, off, sel, x, mean,
                                                          scale),
        "predict_decode_u8": lambda: pr.device_predict_decode(
            n, C, th, tw, words, d_woff, d_nw, d_st, d_sel, d_rect, off, raw, final, st),
        "predict_decode_u8_five_a_lane": lambda: shape("1", runs["predict_decode_u8"]),
        "predict_decode_u8_two_rounds": lambda: shape("2", runs["predict_decode_u8"]),
        "rans_decode_same_streams": lambda: check(lib().idf_rans_decode_streams(
            s, n, nsym, ptr(off), ptr(d_woff), ptr(d_nw), ptr(words), ptr(mean), ptr(scale),
            ptr(d_st), ptr(final), ptr(xo), ptr(st), ptr(wsp), wsb)),
    }
    # what pricing an entry costs beside coding it: idf_predict_cost_u8 against the three
    # launches of device_predict_encode over the same tiles (the host reads between them left out)
    init = torch.full((n,), 1 << 32, dtype=torch.int64, device=dev)
    efinal = torch.empty(n, dtype=torch.int64, device=dev)
    scratch = torch.empty(nsym, dtype=torch.int32, device=dev)
    e_nw = torch.empty(n, dtype=torch.int64, device=dev)
    e_st = torch.empty(n, dtype=torch.int32, device=dev)
    ewb = int(lib().idf_rans_encode_workspace_bytes(nsym))
    ewsp = torch.empty(ewb, dtype=torch.uint8, device=dev)
    gathered = torch.empty(max(int(w_off[-1]), 1), dtype=torch.int32, device=dev)

    def code():
        runs["predict_prep_u8"]()
        check(lib().idf_rans_encode_streams(s, n, nsym, ptr(off), ptr(x), ptr(mean), ptr(scale),
                                            ptr(init), ptr(efinal), ptr(scratch), ptr(e_nw),
                                            ptr(e_st), ptr(ewsp), ewb))
        check(lib().idf_gather_words(s, n, ptr(off), ptr(d_nw), ptr(d_woff), ptr(scratch),
                                     ptr(gathered)))

    runs["predict_cost_u8"] = lambda: pr.device_predict_cost(table, n, C, th, tw)
    runs["predict_prep_encode_gather"] = code
    out = {"predict_symbols": nsym, "predict_words": int(w_off[-1])}
    for name, fn in runs.items():
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
        if name.startswith("predict_decode_u8"):
            assert torch.equal(raw, want) and bool((final == 1 << 32).all()) and not bool(st.any())
        if name == "rans_decode_same_streams":
            assert torch.equal(xo, x) and bool((final == 1 << 32).all())
        if name == "predict_prep_encode_gather":
            assert torch.equal(gathered[:int(w_off[-1])], words) and not bool(e_st.any())
    est = pr.estimate_bytes(pr.device_predict_cost(table, n, C, th, tw).cpu().numpy())
    gap = (est - (pr.entry_overhead() + 4 * nw)) // 4
    out["estimate_minus_coder_words"] = {str(k): int((gap == k).sum()) for k in np.unique(gap)}
    longest = int(counts.max())
    for name in ("predict_decode_u8", "predict_decode_u8_five_a_lane",
                 "predict_decode_u8_two_rounds", "rans_decode_same_streams"):
        # the streams run side by side: a launch lasts as long as its longest chain
        out[name + "_ns_per_symbol"] = round(out[name + "_us"] * 1e3 / longest, 1)
    return out


def _predict_ways_kernel_times(tc, imgs, ways_list, reps: int = 5) -> dict:
    """Per N of ways_list (1: the one-way kernels, the baseline): device time (events) of the
    prep and decode kernels over all tiles of imgs, one stream per tile, and of the decode kernel
    on the first tile alone; every decode is checked against the source bytes."""
    from idfcodec import predict as pr
    from idfcodec.safe import device_gather_raw
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, _, _ = _tables(tc, imgs)
    n, rects = lay.n_tiles, lay.rects
    dev = imgs[0].device
    counts = pr.entry_bytes(rects, C)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    nsym = int(off_h[-1])
    off = torch.from_numpy(off_h).to(dev)
    want = torch.empty(nsym, dtype=torch.uint8, device=dev)
    device_gather_raw(table, n, C, th, tw, off[:n].contiguous(), want)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)  # noqa: E731
                                     .reshape(-1)).to(dev)
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    x, mean, scale = (torch.empty(nsym, dtype=torch.float32, device=dev) for _ in range(3))
    raw = torch.empty(nsym, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    out = {"symbols": nsym, "tiles": n, "longest_stream": int(counts.max())}

    def timed(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / reps * 1e3, 2)

    for N in ways_list:
        sel_h, states, nw, status, words = pr.device_predict_encode(table, counts, C, th, tw, N)
        assert not status.any()
        w_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(nw, out=w_off[1:])
        d_woff, d_nw, d_st = t64(w_off[:n]), t64(nw), t64(states)
        d_sel = torch.from_numpy(sel_h.view(np.int32).copy()).to(dev)
        final = torch.empty(n * N, dtype=torch.int64, device=dev)

        def dec(m):
            if N == 1:
                pr.device_predict_decode(m, C, th, tw, words, d_woff, d_nw, d_st, d_sel, d_rect,
                                         off, raw, final, st)
            else:
                pr.device_predict_decode_ways(m, N, C, th, tw, words, d_woff, d_nw, d_st, d_sel,
                                              None, None, 0, d_rect, off, raw, final, st)
        row = {"words": int(w_off[-1]),
               "prep_us": timed(lambda: pr.device_predict_prep(table, n, C, th, tw, off, sel, x,
                                                               mean, scale, N))}
        raw.zero_()
        row["decode_us"] = timed(lambda: dec(n))
        assert torch.equal(raw, want) and bool((final == 1 << 32).all()) and not bool(st.any())
        # the streams run side by side: a launch lasts as long as its longest chain
        row["decode_ns_per_symbol_per_wave"] = round(row["decode_us"] * 1e3 / int(counts.max()), 1)
        raw.zero_()
        row["decode_one_entry_us"] = timed(lambda: dec(1))
        assert torch.equal(raw[:int(counts[0])], want[:int(counts[0])])
        out[f"ways_{N}"] = row
    return out


def _entry_latency(model, ways_list, steps: int, warmup: int) -> dict:
    """The decode latency of a single full packed entry: one smooth image of the model's tile
    size, decode_region inside it, the codecs of ways_list alternating step by step; wall clock
    with a synchronise on both sides (host work included), every crop checked."""
    th, tw = model.tiled().tile_hw
    img = smooth_images(1, model.tiled().C, th, tw, seed=9)[0].cuda()
    codecs = {N: model.tiled_safe(predict=True, predict_ways=N) for N in ways_list}
    files = {N: pc.encode([img]) for N, pc in codecs.items()}
    ms = {N: [] for N in ways_list}
    y0, x0, h, w = th // 8, tw // 8, th // 2, tw // 2
    exact = True
    for step in range(warmup + steps):
        for N, pc in codecs.items():
            (crop, info), t = _timed(lambda: pc.decode_region(files[N], 0, y0, x0, h, w))
            exact = exact and bool(info["ok"]) and torch.equal(crop, img[:, y0:y0 + h, x0:x0 + w])
            if step >= warmup:
                ms[N].append(t)
    return {"tile": [th, tw], "region": [y0, x0, h, w], "exact": exact,
            **{f"ways_{N}": {"packed_tiles": files[N].n_packed,
                             "entry_bytes": len(files[N].to_bytes()),
                             "ms_median": round(statistics.median(ms[N]), 4),
                             "ms_min": round(min(ms[N]), 4), "ms_max": round(max(ms[N]), 4)}
               for N in ways_list}}


def _seal_kernel_times(tc, imgs, reps: int = 20) -> dict:
    """Device time (events) of the three CRC kernels over all tiles of imgs: the source tiles,
    the gathered pixel-major tiles, and the stored raw runs; each result against the first."""
    from idfcodec.integrity import (device_crc32_segments, device_tile_crc32,
                                    device_tile_crc32_pm)
    from idfcodec.safe import device_gather_raw, raw_offsets
    from idfcodec.tiled import device_gather
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, _, _ = _tables(tc, imgs)
    n, rects = lay.n_tiles, lay.rects
    dev = imgs[0].device
    offs, n_raw = raw_offsets([True] * n, rects, C)
    raw = torch.empty(n_raw, dtype=torch.uint8, device=dev)
    device_gather_raw(table, n, C, th, tw, torch.tensor(offs, dtype=torch.int64, device=dev), raw)
    buf = torch.empty(n * th * tw * 4, dtype=torch.float32, device=dev)
    device_gather(table, n, C, th, tw, buf)
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    seg = torch.tensor([(raw.data_ptr() + o, C * h * w) for o, (h, w) in zip(offs, rects)],
                       dtype=torch.int64, device=dev)
    got = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("u8", "pm", "seg")}
    runs = {
        "tile_crc32_u8": lambda: device_tile_crc32(table, n, C, th, tw, got["u8"]),
        "tile_crc32_pm": lambda: device_tile_crc32_pm(buf, n, C, th, tw, d_rect, got["pm"]),
        "crc32_segments_u8": lambda: device_crc32_segments(seg, n, got["seg"]),
    }
    out = {}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
    assert torch.equal(got["u8"], got["pm"]) and torch.equal(got["u8"], got["seg"])
    return out


def _fingerprint_ms(model) -> float:
    """The one-off cost of the model's fingerprint: the engine's cached value is dropped first."""
    from idfcodec.integrity import model_fingerprint
    eng = model.engine()
    eng._fingerprint = None
    return round(_timed(lambda: model_fingerprint(model))[1], 3)


SAFE_RATIOS = (("safe_ratio_1", 1.0), ("safe_ratio_inf", float("inf")))


def _sealed_step(zc, imgs, kw):
    """One timed encode + decode of a SealedCodec -> (bitstream, encode ms, decode ms, exact)."""
    zbs, te = _timed(lambda: zc.encode(imgs, **kw))
    (out, _), td = _timed(lambda: zc.decode(zbs, verify=False))
    return zbs, te, td, int(all(torch.equal(a, b) for a, b in zip(out, imgs)))


def _sealed_paths(model, escape: bool, predict: bool = False, smallest: bool = False,
                  base: bool = True) -> list:
    """[(row name, SealedCodec, encode keywords)]: one sealed path per unsealed one timed.
    predict: the predictive codec's (_PredictBench's rows predict_ratio_1 and, with smallest,
    smallest_ratio_1); base=False: those alone."""
    paths = [("sealed_tiled", model.tiled_sealed(safe=False), {})] if base else []
    if escape and base:
        paths += [("sealed_" + n, model.tiled_sealed(safe=True), {"max_ratio": r})
                  for n, r in SAFE_RATIOS]
    if predict:
        zc = model.tiled_safe(predict=True, seal=True)
        paths.append(("sealed_predict_ratio_1", zc, {"max_ratio": 1.0}))
        if smallest:
            paths.append(("sealed_smallest_ratio_1", zc,
                          {"max_ratio": 1.0, "choose": "smallest"}))
    return paths


class _SealedBench:
    """The sealed paths of one image set, stepped beside the unsealed ones."""

    def __init__(self, model, escape: bool, predict: bool = False, smallest: bool = False,
                 base: bool = True):
        self.paths = _sealed_paths(model, escape, predict, smallest, base)
        self.t = {n + k: [] for n, _, _ in self.paths for k in ("_enc", "_dec")}
        self.exact = {n: 0 for n, _, _ in self.paths}
        self.last = {}

    def step(self, imgs, timed: bool):
        for name, zc, kw in self.paths:
            self.last[name], te, td, ok = _sealed_step(zc, imgs, kw)
            if timed:
                self.t[name + "_enc"].append(te)
                self.t[name + "_dec"].append(td)
                self.exact[name] += ok

    def rows(self, steps: int, px: int) -> dict:
        rows = {}
        for name, zc, _ in self.paths:
            zbs = self.last[name]
            _, info = zc.decode(zbs)
            inner = len(zbs.inner.to_bytes())
            trust = [_timed(lambda: zc.decode(zbs, verify=False, check_model=False))[1]
                     for _ in range(5)]
            rows[name] = {"encode": _stats(self.t[name + "_enc"], px),
                          "decode": _stats(self.t[name + "_dec"], px),
                          "decode_no_model_check": _stats(trust, px),
                          "round_trip_exact_steps": f"{self.exact[name]}/{steps}",
                          "verified_ok": bool(info["ok"]), "crc_bad": info["crc_bad"],
                          "tiles": len(zbs.crc), "container_bytes": len(zbs.to_bytes()),
                          "seal_bytes": len(zbs.to_bytes()) - inner}
            if "packed_tiles" in info:      # a predictive file: what the three checks summed
                rows[name].update(kept_tiles=zbs.inner.n_kept, raw_tiles=info["raw_tiles"],
                                  packed_tiles=info["packed_tiles"])
        return rows


def _safe_step(sc, imgs, ratio, **kw):
    """One timed encode + decode of SafeTiledCodec -> (bitstream, encode ms, decode ms, exact).
    kw: more of encode's keywords."""
    sbs, te = _timed(lambda: sc.encode(imgs, max_ratio=ratio, **kw))
    (out, _), td = _timed(lambda: sc.decode(sbs, verify=False))
    return sbs, te, td, int(all(torch.equal(a, b) for a, b in zip(out, imgs)))


def _safe_rows(t, exact, last, steps, px, src_bytes, names=tuple(n for n, _ in SAFE_RATIOS)):
    rows = {}
    for name in names:
        sbs = last[name]
        rows[name] = {"encode": _stats(t[name + "_enc"], px),
                      "decode": _stats(t[name + "_dec"], px),
                      "round_trip_exact_steps": f"{exact[name]}/{steps}",
                      "raw_tiles": int(sbs.escaped.sum()), "tiles": len(sbs.escaped),
                      "escaped_share": round(sbs.escaped_share(), 5), "bpd": round(sbs.bpd(), 5),
                      "container_bytes": len(sbs.to_bytes()), "source_bytes": src_bytes}
    return rows


class _PredictBench:
    """PredictiveTileCodec at max_ratio 1 on one image set, stepped beside the other paths."""

    def __init__(self, model, colour: bool = False, predict_ways: int = 1, smallest=None):
        """smallest: None, choose="escaped"; True / False, choose="smallest" with / without the
        shortlist."""
        # a codec of its own: tiled_safe caches one codec a kind, and the rows alternate
        from idfcodec.predict import PredictiveTileCodec
        self.pc = (model.tiled_safe(predict="colour" if colour else True) if predict_ways == 1
                   else PredictiveTileCodec(model, colour=colour, predict_ways=predict_ways))
        self.kw = {} if smallest is None else {"choose": "smallest", "shortlist": bool(smallest)}
        kind = ("colour" if colour else "predict") if smallest is None else (
            "smallest" if smallest else "smallest_all")
        self.name = kind + "_ratio_1" + (f"_ways_{predict_ways}" if predict_ways != 1 else "")
        self.t = {"enc": [], "dec": []}
        self.exact, self.last = 0, None

    def step(self, imgs, timed: bool):
        self.last, te, td, ok = _safe_step(self.pc, imgs, 1.0, **self.kw)
        if timed:
            self.t["enc"].append(te)
            self.t["dec"].append(td)
            self.exact += ok

    def rows(self, steps: int, px: int, src_bytes: int) -> dict:
        pbs = self.last
        _, info = self.pc.decode(pbs)
        n_raw = int(pbs.stored_raw.sum())
        size = len(pbs.to_bytes())
        return {self.name: {
            "encode": _stats(self.t["enc"], px), "decode": _stats(self.t["dec"], px),
            "round_trip_exact_steps": f"{self.exact}/{steps}", "verified_ok": bool(info["ok"]),
            "raw_tiles": n_raw, "packed_tiles": pbs.n_packed, "colour_tiles": pbs.n_colour,
            "kept_tiles": pbs.n_kept, "moved_tiles": int(((pbs.reasons & 8) != 0).sum()),
            "predictor_coded_tiles": int((pbs.pred_bytes >= 0).sum()),
            "tiles": pbs.n_entries, "bpd": round(pbs.bpd(), 5), "container_bytes": size,
            "source_bytes": src_bytes, "container_over_source": round(size / src_bytes, 5)}}


def smooth_images(n: int, C: int, H: int, W: int, seed: int = 0):
    """Ramps plus small noise, uint8 [n, C, H, W]: content a causal predictor codes well."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H).view(1, 1, H, 1)
    xx = torch.arange(W).view(1, 1, 1, W)
    k = torch.arange(n * C).view(n, C, 1, 1)
    base = (yy * (1 + k % 3) + xx * (2 + k % 2)) // 4 + 16 * k
    return ((base + torch.randint(0, 4, (n, C, H, W), generator=g)) % 256).to(torch.uint8)


def _smooth_set(model, steps: int, warmup: int, predict_ways=(), smallest: bool = False,
                seal: bool = False) -> dict:
    """Set (c), with --predict only: 4 smooth images of 512x512 through SafeTiledCodec and
    PredictiveTileCodec at max_ratio 1 (and at each N of predict_ways), alternating step by
    step.  seal: the sealed predictive rows beside them."""
    imgs = list(smooth_images(4, 3, 512, 512, seed=5).cuda())
    sc, pb = model.tiled_safe(), _PredictBench(model)
    more = [_PredictBench(model, predict_ways=N) for N in predict_ways]
    more += [_PredictBench(model, smallest=s) for s in (True, False)] if smallest else []
    st, sexact, sbs = {"safe_ratio_1_enc": [], "safe_ratio_1_dec": []}, 0, None
    zb = _SealedBench(model, True, True, smallest, base=False) if seal else None
    for step in range(warmup + steps):
        sbs, se, sd, ok = _safe_step(sc, imgs, 1.0)
        if seal:
            zb.step(imgs, step >= warmup)
        for p in [pb, *more]:
            p.step(imgs, step >= warmup)
        if step >= warmup:
            st["safe_ratio_1_enc"].append(se)
            st["safe_ratio_1_dec"].append(sd)
            sexact += ok
    px, src = 4 * 512 * 512, 4 * 3 * 512 * 512
    res = {"images": [[512, 512]] * 4, "data": "ramps plus noise 0..3"}
    res.update({"safe_ratio_1": _safe_rows(st, {"safe_ratio_1": sexact}, {"safe_ratio_1": sbs},
                                           steps, px, src, names=("safe_ratio_1",))
                ["safe_ratio_1"]})
    for p in [pb, *more]:
        res.update(p.rows(steps, px, src))
    if seal:
        res.update(zb.rows(steps, px))
    res["kernels"] = _predict_kernel_times(model.tiled(), imgs)
    if predict_ways:
        res["kernels_by_ways"] = _predict_ways_kernel_times(model.tiled(), imgs,
                                                            [1, *predict_ways])
    return res


def correlated_images(n: int, H: int, W: int, tile: int = 64, seed: int = 0):
    """Shared luminance, small chroma, uint8 [n, 3, H, W]: every tile x tile block is a ramp plus
    a random walk along its rows (30..250) in all three planes, offset by +20, 0 and -15, plus
    noise 0..2 a plane -- content whose planes share their structure."""
    out = np.empty((n, 3, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:tile, 0:tile]
    for i in range(n):
        for ty in range(0, H, tile):
            for tx in range(0, W, tile):
                r = np.random.default_rng([seed, i, ty, tx])
                lum = ((yy * 3 + xx * 2) // 2 + r.integers(0, 24, (tile, tile)).cumsum(1) % 64
                       + 30)
                block = np.clip([lum + d + r.integers(0, 3, (tile, tile))
                                 for d in (20, 0, -15)], 0, 255)
                out[i, :, ty:ty + tile, tx:tx + tile] = block[:, :H - ty, :W - tx]
    return torch.from_numpy(out)


def _colour_kernel_times(tc, imgs, reps: int = 5) -> dict:
    """Device time (events, back-to-back launches) of the colour mode's kernels over all tiles of
    imgs: idf_predict_prep2_u8 beside idf_predict_prep_u8, idf_predict_decode2_u8 on every tile's
    colour stream and on every tile's plain stream beside idf_predict_decode_u8 on the same plain
    streams, idf_predict_colour_inverse_u8 alone, and the encoder's other two launches over one
    candidate and over both: idf_rans_encode_streams on n and on 2 n streams, idf_gather_words
    over every plain stream and over the chosen streams of the 2 n."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    from idfcodec import predict as pr
    from idfcodec.safe import device_gather_raw
    th, tw = tc.tile_hw
    C = tc.C
    lay, table, _, _ = _tables(tc, imgs)
    n, rects = lay.n_tiles, lay.rects
    dev = imgs[0].device
    counts = pr.entry_bytes(rects, C)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    nsym = int(off_h[-1])
    off = torch.from_numpy(off_h).to(dev)
    off2_h = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(np.repeat(counts, 2), out=off2_h[1:])
    off2 = torch.from_numpy(off2_h).to(dev)
    sel1 = torch.empty(n, dtype=torch.int32, device=dev)
    sel3 = torch.empty((n, 3), dtype=torch.int32, device=dev)
    x, mean, scale = (torch.empty(2 * nsym, dtype=torch.float32, device=dev) for _ in range(3))
    sel_h, states, nw, status, words = pr.device_predict_encode2(table, counts, C, th, tw)
    assert not status.any()
    w_off = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)  # noqa: E731
    d_rect = torch.tensor(rects, dtype=torch.int32, device=dev)
    raw = torch.empty(nsym, dtype=torch.uint8, device=dev)
    want = torch.empty(nsym, dtype=torch.uint8, device=dev)
    device_gather_raw(table, n, C, th, tw, off[:n].contiguous(), want)
    final = torch.empty(n, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    args = {}
    for kind, k in (("plain", 0), ("colour", 1)):   # stream 2t + k of every tile
        args[kind] = (t64(w_off[k:2 * n:2]), t64(nw[k::2]), t64(states[k::2]),
                      t32(sel_h[:, k].copy()))
    d_sel2 = t32(sel_h[:, 2].copy())
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)
    # the encoder: n streams of prep's symbols, 2 n of prep2's (each prep refills x, mean, scale
    # in its own layout just before its encoder run is timed)
    init = torch.full((2 * n,), 1 << 32, dtype=torch.int64, device=dev)
    efinal = torch.empty(2 * n, dtype=torch.int64, device=dev)
    scratch = torch.empty(2 * nsym, dtype=torch.int32, device=dev)
    enw = torch.empty(2 * n, dtype=torch.int64, device=dev)
    est = torch.empty(2 * n, dtype=torch.int32, device=dev)
    wbytes = int(lib().idf_rans_encode_workspace_bytes(2 * nsym))
    ewsp = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    gout = torch.empty(int(nw.sum()), dtype=torch.int32, device=dev)

    def rans(m, msym, o):
        check(lib().idf_rans_encode_streams(s, m, msym, ptr(o), ptr(x), ptr(mean), ptr(scale),
                                            ptr(init), ptr(efinal), ptr(scratch), ptr(enw),
                                            ptr(est), ptr(ewsp), wbytes), "rans encode")

    _, pick, hit = pr.choose_streams(nw, status, counts)
    chosen = pick[hit]
    g_all = (n, off, t64(nw[0::2]), t64(np.concatenate([[0], np.cumsum(nw[0::2])[:-1]])))
    g_best = (len(chosen), t64(off2_h[chosen]), t64(nw[chosen]),
              t64(np.concatenate([[0], np.cumsum(nw[chosen])[:-1]])))

    def gather(m, o, cnt, dst):
        check(lib().idf_gather_words(s, m, ptr(o), ptr(cnt), ptr(dst), ptr(scratch), ptr(gout)),
              "gather words")

    runs = {
        "predict_prep_u8": lambda: pr.device_predict_prep(table, n, C, th, tw, off, sel1, x, mean,
                                                          scale),
        "rans_encode_one_candidate": lambda: rans(n, nsym, off),
        "gather_words_one_candidate": lambda: gather(*g_all),
        "predict_prep2_u8": lambda: pr.device_predict_prep2(table, n, C, th, tw, off2, sel3, x,
                                                            mean, scale),
        "rans_encode_both_candidates": lambda: rans(2 * n, 2 * nsym, off2),
        "gather_words_chosen_of_both": lambda: gather(*g_best),
        "predict_decode_u8_plain": lambda: pr.device_predict_decode(
            n, C, th, tw, words, *args["plain"], d_rect, off, raw, final, st),
        "predict_decode2_u8_plain": lambda: pr.device_predict_decode2(
            n, C, th, tw, words, *args["plain"], d_sel2, zeros, n, d_rect, off, raw, final, st),
        "predict_decode2_u8_colour": lambda: pr.device_predict_decode2(
            n, C, th, tw, words, *args["colour"], d_sel2, ones, n, d_rect, off, raw, final, st),
    }
    out = {"colour_symbols": nsym, "plain_words": int(nw[0::2].sum()),
           "colour_words": int(nw[1::2].sum())}
    for name, fn in runs.items():
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
        if "decode" in name:
            assert torch.equal(raw, want) and bool((final == 1 << 32).all()) and not bool(st.any())
    # the inverse alone: its input does not matter to its time (raw is not read again: repeated
    # launches leave it transformed several times over)
    inv = lambda: check(lib().idf_predict_colour_inverse_u8(  # noqa: E731
        s, n, C, th, tw, ptr(ones), ptr(d_rect), ptr(off), ptr(raw)))
    inv()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        inv()
    b.record()
    torch.cuda.synchronize()
    out["predict_colour_inverse_u8_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
    longest = int(counts.max())
    for name in runs:
        if "decode" in name:  # the streams run side by side: a launch lasts as its longest chain
            out[name + "_ns_per_symbol"] = round(out[name + "_us"] * 1e3 / longest, 1)
    return out


def _correlated_set(model, steps: int, warmup: int) -> dict:
    """Set (d), with --predict only: 4 correlated images of 512x512 through SafeTiledCodec once
    (its size) and through PredictiveTileCodec without and with the colour mode at max_ratio 1,
    alternating step by step."""
    imgs = list(correlated_images(4, 512, 512, seed=9).cuda())
    pb, qb = _PredictBench(model), _PredictBench(model, colour=True)
    for step in range(warmup + steps):
        pb.step(imgs, step >= warmup)
        qb.step(imgs, step >= warmup)
    px, src = 4 * 512 * 512, 4 * 3 * 512 * 512
    safe_size = len(model.tiled_safe().encode(imgs, max_ratio=1.0).to_bytes())
    res = {"images": [[512, 512]] * 4,
           "data": "per tile: shared ramp plus random walk, chroma offsets, noise 0..2",
           "safe_ratio_1": {"container_bytes": safe_size, "source_bytes": src,
                            "container_over_source": round(safe_size / src, 5)}}
    res.update(pb.rows(steps, px, src))
    res.update(qb.rows(steps, px, src))
    res["kernels"] = _colour_kernel_times(model.tiled(), imgs)
    return res


def bench(steps: int = 7, warmup: int = 2, escape: bool = False, seal: bool = False,
          predict: bool = False, predict_ways=(), smallest: bool = False) -> dict:
    from idfcodec import configs, synthetic

    def small(model):  # choose="smallest" beside "escaped": with the shortlist and without
        return [_PredictBench(model, smallest=s) for s in (True, False)] if smallest else []
    model = synthetic.build_model(configs.get("imagenet64")).cuda()
    tc = model.tiled()
    sc = model.tiled_safe() if escape else None
    safe_keys = [n + k for n, _ in SAFE_RATIOS for k in ("_enc", "_dec")] if escape else []
    res = {"metric": "tiled encode+decode of images of any size (imagenet64, seeded weights)",
           "steps": steps, "warmup": warmup, "max_batch": tc.max_batch,
           "data": "synthetic uint8, seeded weights"}
    # (a) 4 x 512x512 = 256 full tiles, beside the plain codec on the same tiles
    imgs = list(synthetic.images(4, 3, 512, 512, seed=2).cuda())
    tiles = torch.stack(imgs).view(4, 3, 8, 64, 8, 64).permute(0, 2, 4, 1, 3, 5).reshape(
        256, 3, 64, 64).contiguous()
    t = {k: [] for k in ("tiled_enc", "tiled_dec", "plain_enc", "plain_dec")}
    st = {k: [] for k in safe_keys}
    exact = {"tiled": 0, "plain": 0}
    sexact, slast = {n: 0 for n, _ in SAFE_RATIOS}, {}
    same_bytes = None
    zb = _SealedBench(model, escape, predict, smallest) if seal else None
    pbl = [_PredictBench(model), *(_PredictBench(model, predict_ways=N)
                                   for N in predict_ways), *small(model)] if predict else []
    for step in range(warmup + steps):
        tbs, te = _timed(lambda: tc.encode(imgs))
        (out, _), td = _timed(lambda: tc.decode(tbs, verify=False))
        bs, pe = _timed(lambda: model.encode(tiles))
        (pout, _), pd = _timed(lambda: model.decode(bs, verify=False))
        for name, ratio in SAFE_RATIOS if escape else ():
            slast[name], se, sd, ok = _safe_step(sc, imgs, ratio)
            if step >= warmup:
                st[name + "_enc"].append(se)
                st[name + "_dec"].append(sd)
                sexact[name] += ok
        if seal:
            zb.step(imgs, step >= warmup)
        for pb in pbl:
            pb.step(imgs, step >= warmup)
        if step < warmup:
            continue
        for k, v in zip(t, (te, td, pe, pd)):
            t[k].append(v)
        exact["tiled"] += int(all(torch.equal(a, b) for a, b in zip(out, imgs)))
        exact["plain"] += int(torch.equal(pout, tiles))
        same_bytes = tbs.stream.to_bytes() == bs.to_bytes()
    px = 4 * 512 * 512
    res["full_tiles"] = {
        "images": [[512, 512]] * 4, "tiles": tbs.stream.n_images,
        "tiled": {"encode": _stats(t["tiled_enc"], px), "decode": _stats(t["tiled_dec"], px)},
        "plain_same_tiles": {"encode": _stats(t["plain_enc"], px),
                             "decode": _stats(t["plain_dec"], px)},
        "round_trip_exact_steps": {k: f"{v}/{steps}" for k, v in exact.items()},
        "inner_bytes_equal_plain": same_bytes, "padded_share": round(tbs.padded_share(), 5),
        "state_bits_per_subpixel": round(tbs.state_bits_per_subpixel(), 5),
        "bpd": round(tbs.bpd(), 5), "conv": tbs.stream.meta["conv"],
        "kernels": _kernel_times(tc, imgs),
        "kernels_by_layout": _layout_kernel_times(tc, imgs)}
    if escape:
        res["full_tiles"].update(_safe_rows(st, sexact, slast, steps, px, 4 * 3 * 512 * 512))
        res["full_tiles"]["safe_inf_inner_bytes_equal_tiled"] = (
            slast["safe_ratio_inf"].stream.to_bytes() == tbs.stream.to_bytes())
        res["full_tiles"]["kernels"].update(_escape_kernel_times(tc, imgs))
    if seal:
        res["full_tiles"].update(zb.rows(steps, px))
        res["full_tiles"]["sealed_inner_bytes_equal_tiled"] = (
            zb.last["sealed_tiled"].inner.to_bytes() == tbs.to_bytes())
        res["full_tiles"]["kernels"].update(_seal_kernel_times(tc, imgs))
        res["fingerprint_ms"] = _fingerprint_ms(model)
    if predict:
        for pb in pbl:
            res["full_tiles"].update(pb.rows(steps, px, 4 * 3 * 512 * 512))
        res["full_tiles"]["kernels"].update(_predict_kernel_times(tc, imgs))
        if predict_ways:
            res["full_tiles"]["kernels_by_ways"] = _predict_ways_kernel_times(
                tc, imgs, [1, *predict_ways])
    # (b) a ragged set
    rag = [synthetic.images(1, 3, H, W, seed=3 + i)[0].cuda() for i, (H, W) in enumerate(RAGGED)]
    t = {"enc": [], "dec": []}
    st = {k: [] for k in safe_keys}
    sexact, slast = {n: 0 for n, _ in SAFE_RATIOS}, {}
    n_exact = 0
    zb = _SealedBench(model, escape, predict, smallest) if seal else None
    pbl = [_PredictBench(model), *(_PredictBench(model, predict_ways=N)
                                   for N in predict_ways), *small(model)] if predict else []
    for step in range(warmup + steps):
        tbs, te = _timed(lambda: tc.encode(rag))
        (out, _), td = _timed(lambda: tc.decode(tbs, verify=False))
        for name, ratio in SAFE_RATIOS if escape else ():
            slast[name], se, sd, ok = _safe_step(sc, rag, ratio)
            if step >= warmup:
                st[name + "_enc"].append(se)
                st[name + "_dec"].append(sd)
                sexact[name] += ok
        if seal:
            zb.step(rag, step >= warmup)
        for pb in pbl:
            pb.step(rag, step >= warmup)
        if step < warmup:
            continue
        t["enc"].append(te)
        t["dec"].append(td)
        n_exact += int(all(torch.equal(a, b) for a, b in zip(out, rag)))
    px = sum(H * W for H, W in RAGGED)
    _, info = tc.decode(tbs)
    (crop, rinfo), region_ms = _timed(lambda: tc.decode_region(tbs, 1, 100, 100, 64, 64))
    res["ragged"] = {
        "images": [list(s) for s in RAGGED], "tiles": tbs.stream.n_images,
        "tiled": {"encode": _stats(t["enc"], px), "decode": _stats(t["dec"], px)},
        "round_trip_exact_steps": f"{n_exact}/{steps}", "verified_ok": bool(info["ok"]),
        "padded_share": round(tbs.padded_share(), 5),
        "state_bits_per_subpixel": round(tbs.state_bits_per_subpixel(), 5),
        "bpd": round(tbs.bpd(), 5), "conv": tbs.stream.meta["conv"],
        "region_64x64": {"tiles": rinfo["tiles"], "ms": round(region_ms, 3),
                         "exact": bool(rinfo["ok"])
                         and bool(torch.equal(crop, rag[1][:, 100:164, 100:164]))},
        "kernels_by_layout": _layout_kernel_times(tc, rag)}
    if escape:
        res["ragged"].update(_safe_rows(st, sexact, slast, steps, px,
                                        3 * sum(H * W for H, W in RAGGED)))
    if seal:
        res["ragged"].update(zb.rows(steps, px))
    if predict:
        for pb in pbl:
            res["ragged"].update(pb.rows(steps, px, 3 * sum(H * W for H, W in RAGGED)))
        res["smooth"] = _smooth_set(model, steps, warmup, predict_ways, smallest, seal)
        if predict_ways:
            res["single_entry"] = _entry_latency(model, [1, *predict_ways], steps, warmup)
        res["correlated"] = _correlated_set(model, steps, warmup)
    return res


def _base_of(model, escape: bool, predict: bool):
    """The tiled codec the flags name, the base of a plane set."""
    if predict:
        return model.tiled_safe(predict=True)
    return model.tiled_safe() if escape else model.tiled()


def plane_images(n: int, channels: int, C: int, H: int, W: int, alpha: str, seed: int = 0):
    """n synthetic sources of `channels` channels as dense [H, W, channels] device tensors.
    Against a model of C channels: the first C are noise (the flow's planes) and the others
    smooth, with fewer than C all are smooth; the last channel of 2, or of more than C, is
    alpha -- "opaque": 255 everywhere; "disc": 255 inside a centred disc of radius H / 3, else
    0, so the tiles its edge crosses are coded and the others constant."""
    from idfcodec import synthetic
    if channels >= C:
        parts = [synthetic.images(n, C, H, W, seed=seed)]
        if channels > C:
            parts.append(smooth_images(n, channels - C, H, W, seed=seed + 1))
    else:
        parts = [smooth_images(n, channels, H, W, seed=seed + 1)]
    x = torch.cat(parts, dim=1)
    if channels == 2 or channels > C:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        disc = ((yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= (H // 3) ** 2).to(torch.uint8) * 255
        x[:, -1] = 255 if alpha == "opaque" else disc
    return [t.permute(1, 2, 0).contiguous().cuda() for t in x]


def bench_planes(channels: int, steps: int = 7, warmup: int = 2, escape: bool = False,
                 predict: bool = False) -> dict:
    """bench --channels N: 4 sources of 512x512 and N channels (plane_images, opaque alpha and a
    disc) through model.tiled_planes over the base the flags name, beside that base alone over
    the same sources' base planes, alternating step by step."""
    from idfcodec import configs, synthetic
    model = synthetic.build_model(configs.get("imagenet64")).cuda()
    base = _base_of(model, escape, predict)
    pc = model.tiled_planes(channels, base=base)
    px = 4 * 512 * 512
    res = {"metric": "plane sets: encode+decode of images of another channel count than the "
                     "model's (imagenet64, seeded weights)",
           "channels": channels, "base_planes": pc.Cb, "extra_planes": pc.Ce,
           "base": type(base).__name__ if pc.Cb else None, "steps": steps, "warmup": warmup,
           "images": [[512, 512]] * 4}
    has_alpha = channels == 2 or channels > model.C     # plane_images' rule; else one set
    for alpha in ("opaque", "disc") if has_alpha else ("opaque",):
        imgs = plane_images(4, channels, model.C, 512, 512, alpha, seed=2)
        rgb = [t.permute(2, 0, 1)[:pc.Cb] for t in imgs]
        ms = {k: [] for k in ("enc", "dec", "base_enc", "base_dec")}
        exact = 0
        for step in range(warmup + steps):
            bs, te = _timed(lambda: pc.encode(imgs, layout="hwc"))
            (outs, info), td = _timed(lambda: pc.decode(bs, verify=False, layout="hwc"))
            be = bd = 0.0
            if pc.Cb:
                bbs, be = _timed(lambda: base.encode(rgb, layout="chw"))
                _, bd = _timed(lambda: base.decode(bbs, verify=False))
            if step < warmup:
                continue
            for k, v in zip(ms, (te, td, be, bd)):
                ms[k].append(v)
            exact += int(all(torch.equal(a, b) for a, b in zip(outs, imgs)))
        size, plane = len(bs.to_bytes()), len(bs.plane_section())
        row = {"encode": _stats(ms["enc"], px), "decode": _stats(ms["dec"], px),
               "base_only": ({"encode": _stats(ms["base_enc"], px),
                              "decode": _stats(ms["base_dec"], px)} if pc.Cb else None),
               "round_trip_exact_steps": f"{exact}/{steps}",
               "units": bs.n_units, "constant_units": bs.n_constant,
               "packed_units": bs.n_packed, "raw_units": int(bs.stored_raw.sum()),
               "file_bytes": size, "plane_section_bytes": plane,
               "extra_planes_share": round(plane / size, 6),
               "source_bytes": sum(t.numel() for t in imgs), "bpd": round(bs.bpd(), 5)}
        res[alpha + "_alpha" if has_alpha else "no_alpha"] = row
    return res


# ------------------------------------------------------------------ bench --deep
def deep_images(n: int = 4, H: int = 512, W: int = 512, seed: int = 0):
    """n seeded uint16 [1, H, W] images: a ramp with sigma 30 noise; the same with sigma 300; a
    12-bit sensor frame (smooth signal, shot noise, a masked border of zeros, hot pixels); half
    uniform 16-bit noise over half flat steps."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = 4000 + 60 * yy + 35 * xx
    sensor = 1800 + 1500 * np.sin(yy / 70) * np.cos(xx / 90)
    sensor = rng.poisson(np.maximum(sensor, 1)).astype(np.float64)
    sensor[:, :W // 8] = 0
    hot = rng.random((H, W)) < 1e-3
    sensor[hot] = 4095
    mixed = np.where(yy < H // 2, rng.integers(0, 65536, (H, W)), 5000 * (xx // 64) + 100)
    kinds = [ramp + rng.normal(0, 30, (H, W)), ramp + rng.normal(0, 300, (H, W)), sensor, mixed]
    return [np.clip(np.rint(kinds[i % 4]), 0, 65535).astype(np.uint16)[None] for i in range(n)]


def _event_us(fn, reps: int) -> float:
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / reps * 1e3, 2)


def _deep_kernel_times(imgs, tile, reps: int = 5) -> dict:
    """Device time (events) of idf_deep_decode_u16 with every unit of imgs decoded as a packed
    unit, and beside it the 8-bit predictive coder at one way on the same tiles of the samples'
    high bytes: idf_predict_decode_u8.  The units run side by side, so a decode launch lasts as
    long as its longest chain."""
    from idfcodec import _lib, deep
    from idfcodec import predict as pr
    from idfcodec._lib import check, lib, ptr
    from idfcodec.tiled import TileLayout, TiledCodec
    th, tw = tile
    dev = imgs[0].device
    lay = TileLayout([t.shape[1:] for t in imgs], 1, tile)
    rows = deep.unit_rows(lay.image_rows()[2], imgs, 1)
    ns = deep.unit_samples(lay.rects, 1)
    n, nsym = len(ns), int(ns.sum())
    out = {"units": n, "samples": nsym}
    p = deep.device_deep_prep(rows, ns, th, tw, dev)
    states, nw, status, words = pr._code_streams(p["off"], p["off_h"], p["x"], p["mean"],
                                                 p["scale"])
    assert not status.any()
    w_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    d_woff, d_nw, d_st, d_low, d_off, d_ne = (t64(w_off[:n]), t64(nw), t64(states),
                                              t64(p["low_h"][:n]), t64(p["off_h"][:n]),
                                              t64(p["nesc"]))
    d_cls = torch.ones(n, dtype=torch.uint8, device=dev)
    d_val = torch.zeros(n, dtype=torch.int16, device=dev)
    d_shift = torch.from_numpy(p["shift"].copy()).to(dev)
    d_sel = torch.from_numpy(p["sel"].view(np.int32).copy()).to(dev)
    d_rect = torch.tensor(lay.rects, dtype=torch.int32, device=dev)
    got = torch.empty(nsym, dtype=torch.int16, device=dev)
    final = torch.empty(n, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    s = _lib.stream_ptr(dev)
    out["deep_decode_u16_us"] = _event_us(lambda: check(lib().idf_deep_decode_u16(
        s, n, th, tw, ptr(d_cls), ptr(d_val), ptr(d_shift), ptr(d_sel), ptr(d_st), ptr(words),
        ptr(d_woff), ptr(d_nw), ptr(p["low"]), ptr(d_low), ptr(p["esc"]), ptr(d_off), ptr(d_ne),
        ptr(d_rect), ptr(d_off), ptr(got), ptr(final), ptr(st))), reps)
    want = deep.device_gather_raw16(rows, ns, th, tw, dev)
    assert torch.equal(got, want) and bool((final == 1 << 32).all()) and not bool(st.any())
    out["deep_words"] = int(w_off[-1])
    # the yardstick: the samples' high bytes through the 8-bit predictive coder, one way
    high = [(t.view(torch.int16).to(torch.int32) >> 8).to(torch.uint8).contiguous() for t in imgs]
    table = TiledCodec._device_table(lay.rows([t.data_ptr() for t in high]), dev)
    sel_h, st8, nw8, status8, words8 = pr.device_predict_encode(table, ns, 1, th, tw)
    assert not status8.any()
    w8 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nw8, out=w8[1:])
    off = t64(p["off_h"])
    raw = torch.empty(nsym, dtype=torch.uint8, device=dev)
    d8 = (t64(w8[:n]), t64(nw8), t64(st8), torch.from_numpy(sel_h.view(np.int32).copy()).to(dev))
    out["predict_decode_u8_us"] = _event_us(lambda: pr.device_predict_decode(
        n, 1, th, tw, words8, d8[0], d8[1], d8[2], d8[3], d_rect, off, raw, final, st), reps)
    assert bool((final == 1 << 32).all()) and not bool(st.any())
    longest = int(ns.max())
    for name in ("deep_decode_u16", "predict_decode_u8"):
        out[name + "_ns_per_symbol"] = round(out[name + "_us"] * 1e3 / longest, 1)
    out["decode_u16_over_u8"] = round(out["deep_decode_u16_us"] / out["predict_decode_u8_us"], 3)
    return out


def _deep_decode_kernel_us(imgs, tile, ways: int, reps: int = 5) -> float:
    """Device time (events) of the decode kernel of a `ways`-way file -- idf_deep_decode_u16 at
    one way, idf_deep_decode_ways_u16 above -- with every unit of imgs decoded as a packed unit,
    the output checked against the sources."""
    from idfcodec import _lib, deep
    from idfcodec import predict as pr
    from idfcodec._lib import check, lib, ptr
    from idfcodec.tiled import TileLayout
    th, tw = tile
    dev = imgs[0].device
    lay = TileLayout([t.shape[1:] for t in imgs], 1, tile)
    rows = deep.unit_rows(lay.image_rows()[2], imgs, 1)
    ns = deep.unit_samples(lay.rects, 1)
    n, nsym = len(ns), int(ns.sum())
    p = deep.device_deep_prep(rows, ns, th, tw, dev, ways)
    states, nw, status, words = pr._code_streams(p["off"], p["off_h"], p["x"], p["mean"],
                                                 p["scale"], ways=ways)
    assert not status.any()
    w_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    d_woff, d_nw, d_st, d_low, d_off, d_ne = (t64(w_off[:n]), t64(nw), t64(states.reshape(-1)),
                                              t64(p["low_h"][:n]), t64(p["off_h"][:n]),
                                              t64(p["nesc"]))
    d_cls = torch.ones(n, dtype=torch.uint8, device=dev)
    d_val = torch.zeros(n, dtype=torch.int16, device=dev)
    d_shift = torch.from_numpy(p["shift"].copy()).to(dev)
    d_sel = torch.from_numpy(p["sel"].view(np.int32).copy()).to(dev)
    d_rect = torch.tensor(lay.rects, dtype=torch.int32, device=dev)
    got = torch.empty(nsym, dtype=torch.int16, device=dev)
    final = torch.empty(n * ways, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    args = (ptr(d_cls), ptr(d_val), ptr(d_shift), ptr(d_sel), ptr(d_st), ptr(words), ptr(d_woff),
            ptr(d_nw), ptr(p["low"]), ptr(d_low), ptr(p["esc"]), ptr(d_off), ptr(d_ne),
            ptr(d_rect), ptr(d_off), ptr(got), ptr(final), ptr(st))
    s = _lib.stream_ptr(dev)
    if ways == 1:
        us = _event_us(lambda: check(lib().idf_deep_decode_u16(s, n, th, tw, *args)), reps)
    else:
        us = _event_us(lambda: check(lib().idf_deep_decode_ways_u16(s, n, ways, th, tw, *args)),
                       reps)
    want = deep.device_gather_raw16(rows, ns, th, tw, dev)
    assert torch.equal(got, want) and bool((final == 1 << 32).all()) and not bool(st.any())
    return us


def _deep_steps(hin: int, win: int, ways: int) -> int:
    """the wavefront steps of a unit (its samples at one way)"""
    if ways == 1:
        return hin * win
    nb = -(-hin // ways)
    return (nb - 1) * max(win, ways) + (hin - (nb - 1) * ways - 1) + win


def bench_deep_ways(host, imgs, tile, ways, steps: int, warmup: int) -> dict:
    """bench --deep --deep-ways: the one-way codec and the codecs of `ways` alternating step by
    step in one process -> per N: file bytes, encode and decode ms, the device time of the decode
    kernel with every unit decoded as packed (and per step of a full unit), and the decode_region
    latency of one packed unit of image 0."""
    from idfcodec import DeepTiledCodec
    codecs = {N: DeepTiledCodec(1, tile=tile, ways=N) for N in (1,) + tuple(ways)}
    t = {N: {"encode": [], "decode": [], "region": []} for N in codecs}
    px = sum(a.size for a in host)
    th, tw = tile
    files = {}
    for i in range(warmup + steps):
        for N, codec in codecs.items():
            bs, ms_e = _timed(lambda: codec.encode(imgs))
            (outs, info), ms_d = _timed(lambda: codec.decode(bs))
            assert info["ok"]
            (crop, info_r), ms_r = _timed(lambda: codec.decode_region(bs, 0, 0, 0, th, tw))
            assert info_r["ok"] and (info_r["tiles"], info_r["packed_planes"]) == (1, 1)
            if i >= warmup:
                t[N]["encode"].append(ms_e)
                t[N]["decode"].append(ms_d)
                t[N]["region"].append(ms_r)
            if i == 0:
                assert all(np.array_equal(_u16_to_host(o), a) for o, a in zip(outs, host))
                assert np.array_equal(_u16_to_host(crop), host[0][:, :th, :tw])
                files[N] = (len(bs.to_bytes()), int(bs.packed.sum()))
    out = {}
    for N in codecs:
        us = _deep_decode_kernel_us(imgs, tile, N)
        lat = t[N]["region"]
        out[str(N)] = {"container_bytes": files[N][0], "packed_units": files[N][1],
                       "encode": _stats(t[N]["encode"], px), "decode": _stats(t[N]["decode"], px),
                       "decode_kernel_us": us, "steps_per_unit": _deep_steps(th, tw, N),
                       "ns_per_step": round(us * 1e3 / _deep_steps(th, tw, N), 1),
                       "one_unit_region_ms": {"median": round(statistics.median(lat), 3),
                                              "min": round(min(lat), 3),
                                              "max": round(max(lat), 3)}}
    return out


def bench_deep(steps: int = 7, warmup: int = 2, tile=(64, 64), ways=()) -> dict:
    """bench --deep: seeded 16-bit images through DeepTiledCodec, and the kernels' device time
    beside the 8-bit predictive coder's on as many samples from the same build.  ways: instead,
    the codecs of those interleaved states beside the one-way codec (bench_deep_ways)."""
    from idfcodec import DeepTiledCodec
    host = deep_images()
    imgs = [_u16_to_device(a) for a in host]
    if ways:
        return {"bench": "deep-ways", "images": len(host), "size": list(host[0].shape[1:]),
                "tile": list(tile), "samples": sum(a.size for a in host), "steps": steps,
                "warmup": warmup, "ways": bench_deep_ways(host, imgs, tile, ways, steps, warmup)}
    codec = DeepTiledCodec(1, tile=tile)
    enc, dec, bs, outs = [], [], None, None
    for i in range(warmup + steps):
        bs, ms = _timed(lambda: codec.encode(imgs))
        (outs, info), ms_d = _timed(lambda: codec.decode(bs))
        assert info["ok"]
        if i >= warmup:
            enc.append(ms)
            dec.append(ms_d)
    assert all(np.array_equal(_u16_to_host(o), a) for o, a in zip(outs, host))
    px = sum(a.size for a in host)
    cls, raw = bs.classes, bs.to_bytes()
    return {"bench": "deep", "images": len(host), "size": list(host[0].shape[1:]),
            "tile": list(tile), "samples": px, "container_bytes": len(raw),
            "bits_per_sample": round(8 * len(raw) / px, 4),
            "class_share": {k: round(float((cls == v).mean()), 4)
                            for k, v in (("constant", 0), ("packed", 1), ("raw", 2))},
            "shifts": {str(k): int((bs.shift == k).sum()) for k in np.unique(bs.shift)},
            "escapes": int(len(bs.escapes)), "encode": _stats(enc, px), "decode": _stats(dec, px),
            "kernels": _deep_kernel_times(imgs, tile)}


# ------------------------------------------------------------------ files
def _pnm_header(data: bytes, path: str):
    """-> (magic, W, H, maxval, the offset of the samples) of a binary PNM's header."""
    fields, o = [], 0
    while len(fields) < 4:
        while o < len(data) and data[o:o + 1].isspace():
            o += 1
        if data[o:o + 1] == b"#":
            while o < len(data) and data[o:o + 1] != b"\n":
                o += 1
            continue
        e = o
        while e < len(data) and not data[e:e + 1].isspace():
            e += 1
        if e == o:
            raise ValueError(f"{path}: truncated PNM header")
        fields.append(data[o:e])
        o = e
    o += 1  # the single whitespace after maxval
    return fields[0], int(fields[1]), int(fields[2]), int(fields[3]), o


def _read_pnm_stored(path: str) -> np.ndarray:
    """Binary PPM (P6) / PGM (P5), maxval <= 255 -> uint8 [H, W, C], the pixel bytes as the file
    stores them (a read-only view of the file's buffer)."""
    with open(path, "rb") as f:
        data = f.read()
    magic, W, H, maxval, o = _pnm_header(data, path)
    if magic not in (b"P5", b"P6") or not 0 < maxval <= 255 or W < 1 or H < 1:
        raise ValueError(f"{path}: only binary P5 / P6 with maxval <= 255 are read")
    C = 3 if magic == b"P6" else 1
    if len(data) - o < H * W * C:
        raise ValueError(f"{path}: truncated pixel data")
    return np.frombuffer(data, np.uint8, H * W * C, o).reshape(H, W, C)


# ------------------------------------------------------------------ 16-bit files
def is_deep_source(path: str) -> bool:
    """Whether the file holds 16-bit samples: a .npy of uint16, or a binary P5 / P6 with maxval
    256..65535.  Such files go through DeepTiledCodec, every other where it went before."""
    if path.lower().endswith(".npy"):
        return np.load(path, mmap_mode="r", allow_pickle=False).dtype == np.uint16
    with open(path, "rb") as f:
        data = f.read(4096)
    try:
        magic, _, _, maxval, _ = _pnm_header(data, path)
    except ValueError:
        return False
    return magic in (b"P5", b"P6") and 256 <= maxval <= 65535


def read_image16(path: str) -> np.ndarray:
    """-> uint16 [H, W, C] in host byte order.  A PNM's samples are big-endian and are swapped
    here, on the host; a .npy of two dimensions is one plane, of three [H, W, C] unless its first
    dimension is the smaller one ([C, H, W])."""
    if path.lower().endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint16 or a.ndim not in (2, 3):
            raise ValueError(f"{path}: expected a uint16 array of 2 or 3 dimensions")
        if a.ndim == 2:
            return np.ascontiguousarray(a[:, :, None])
        return np.ascontiguousarray(a if a.shape[2] <= a.shape[0] else a.transpose(1, 2, 0))
    with open(path, "rb") as f:
        data = f.read()
    magic, W, H, maxval, o = _pnm_header(data, path)
    if magic not in (b"P5", b"P6") or not 256 <= maxval <= 65535 or W < 1 or H < 1:
        raise ValueError(f"{path}: only binary P5 / P6 with maxval 256..65535 are read here")
    C = 3 if magic == b"P6" else 1
    if len(data) - o < 2 * H * W * C:
        raise ValueError(f"{path}: truncated pixel data")
    return np.frombuffer(data, ">u2", H * W * C, o).astype(np.uint16).reshape(H, W, C)


def write_image16(dirname: str, i: int, hwc: np.ndarray) -> str:
    """hwc: uint16 [H, W, C] -> image_NNNN.pgm / .ppm with maxval 65535 (big-endian samples), or
    a .npy of [C, H, W] for other channel counts."""
    H, W, C = hwc.shape
    if C in (1, 3):
        path = os.path.join(dirname, f"image_{i:04d}." + ("pgm" if C == 1 else "ppm"))
        with open(path, "wb") as f:
            f.write(b"%s\n%d %d\n65535\n" % (b"P5" if C == 1 else b"P6", W, H))
            f.write(np.ascontiguousarray(hwc).astype(">u2").tobytes())
    else:
        path = os.path.join(dirname, f"image_{i:04d}.npy")
        np.save(path, np.ascontiguousarray(hwc.transpose(2, 0, 1)))
    return path


def _u16_to_device(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _u16_to_host(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def compress_deep(out: str, files, tile=(64, 64), ways: int = 1):
    """16-bit sources: an IDFD file (idfcodec.deep), no model; ways: its interleaved states."""
    from idfcodec import DeepTiledCodec
    imgs = [read_image16(p) for p in files]
    if len({a.shape[2] for a in imgs}) > 1:
        raise SystemExit(f"the files hold {sorted({a.shape[2] for a in imgs})} channels: a file "
                         "has one channel count")
    bs = DeepTiledCodec(imgs[0].shape[2], tile=tile, ways=ways).encode(
        [_u16_to_device(a) for a in imgs], layout="hwc")
    raw = bs.to_bytes()
    with open(out, "wb") as f:
        f.write(raw)
    cls = bs.classes
    print(json.dumps({"images": len(imgs), "channels": bs.C, "tiles": bs.layout.n_tiles,
                      "units": bs.n_units, "constant_units": int((cls == 0).sum()),
                      "packed_units": int((cls == 1).sum()), "raw_units": int((cls == 2).sum()),
                      "escapes": int(len(bs.escapes)), **({"ways": bs.ways} if ways != 1 else {}),
                      "source_bytes": 2 * sum(a.size for a in imgs), "container_bytes": len(raw),
                      "bits_per_sample": round(8 * len(raw) / sum(a.size for a in imgs), 5)}))


def decompress_deep(path: str, buf: bytes, dirname: str):
    from idfcodec import DeepTiledBitstream, DeepTiledCodec
    bs = DeepTiledBitstream.from_bytes(buf, device="cuda")
    outs, info = DeepTiledCodec(bs.C, tile=bs.tile_hw).decode(bs, layout="hwc")
    if not info["ok"]:
        raise SystemExit(f"{path}: damaged units {info['damaged_planes']}")
    os.makedirs(dirname, exist_ok=True)
    names = [write_image16(dirname, i, _u16_to_host(t)) for i, t in enumerate(outs)]
    print(json.dumps({"images": len(names), "tiles": info["tiles"], "first": names[0],
                      **{k: info[k] for k in ("constant_planes", "packed_planes", "raw_planes",
                                              "escapes")}}))


def _deep_or_not(files) -> bool:
    deep = [is_deep_source(p) for p in files]
    if any(deep) and not all(deep):
        raise SystemExit("8-bit and 16-bit sources do not share a file")
    return all(deep)


def _read_pnm(path: str) -> np.ndarray:
    """Binary PPM (P6) / PGM (P5), maxval <= 255 -> uint8 [C, H, W]."""
    return np.ascontiguousarray(_read_pnm_stored(path).transpose(2, 0, 1))


def read_image_stored(path: str, C: int):
    """-> (the file's uint8 array as it is stored, its layout "hwc" or "chw"): no transposition
    on the host; the codecs read either (encode(..., layout=...)).  A PPM / PGM is [H, W, C]; a
    .npy is what it holds ([H, W] is one plane, "chw")."""
    if path.lower().endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError(f"{path}: expected a uint8 array of 2 or 3 dimensions")
        layout = "hwc" if a.ndim == 3 and a.shape[0] != C and a.shape[2] == C else "chw"
        if a.ndim == 2:
            a = a[None]
    else:
        a, layout = _read_pnm_stored(path), "hwc"
    have = a.shape[2] if layout == "hwc" else a.shape[0]
    if have != C:
        raise ValueError(f"{path}: {have} channels, the model codes {C}")
    return a, layout


def file_channels(path: str, C: int) -> int:
    """The channels a source file holds.  A PGM holds 1, a PPM 3, a .npy of two dimensions 1.  A
    .npy of three whose first or last dimension is the model's C holds C (read_image_stored's
    rule); of any other the smaller of those two dimensions is the channels (a tie: the
    first)."""
    if not path.lower().endswith(".npy"):
        return int(_read_pnm_stored(path).shape[2])
    a = np.load(path, mmap_mode="r", allow_pickle=False)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"{path}: expected a uint8 array of 2 or 3 dimensions")
    if a.ndim == 2:
        return 1
    if C in (a.shape[0], a.shape[2]):
        return C
    return int(a.shape[2] if a.shape[2] < a.shape[0] else a.shape[0])


def plane_set_channels(files, C: int):
    """None where every file holds the model's C channels (the tiled codecs' own files); else
    the channel count all of them share: a plane set."""
    have = [file_channels(p, C) for p in files]
    if all(h == C for h in have):
        return None
    if len(set(have)) > 1:
        raise SystemExit(f"the files hold {sorted(set(have))} channels: a plane set has one "
                         "channel count")
    return have[0]


def compress_planes(out: str, files, model, Cs: int, base_args: dict, encode_args: dict,
                    predict_ways: int = 1):
    """Sources of another channel count than the model's: an IDFM file (idfcodec.planes) around
    the file the flags name.  base_args: model.tiled_safe's keywords, or {"plain": True} for
    model.tiled(); a sealed base exits with tiled_planes' refusal."""
    args = dict(base_args)
    plain, sealed_plain = args.pop("plain", False), args.pop("seal_plain", False)
    try:
        if plain or sealed_plain:
            base = (model.tiled_sealed(ways=args["ways"], safe=False) if sealed_plain else
                    model.tiled(ways=args["ways"]))
        else:
            base = model.tiled_safe(**args)
        pc = model.tiled_planes(Cs, base=base, predict_ways=predict_ways)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    imgs = [upload_hwc(p, Cs) for p in files]
    bs = pc.encode(imgs, layout="hwc", **(encode_args if pc.Cb else {}))
    raw = bs.to_bytes()
    with open(out, "wb") as f:
        f.write(raw)
    print(json.dumps({"images": len(imgs), "channels": Cs, "base_planes": bs.Cb,
                      "tiles": bs.layout.n_tiles, "units": bs.n_units,
                      "constant_units": bs.n_constant, "packed_units": bs.n_packed,
                      "raw_units": int(bs.stored_raw.sum()), "predict_ways": bs.predict_ways,
                      "base": type(bs.base).__name__ if bs.base is not None else None,
                      "base_bytes": len(bs.base.to_bytes()) if bs.base is not None else 0,
                      "plane_section_bytes": len(bs.plane_section()),
                      "source_bytes": sum(t.numel() for t in imgs), "container_bytes": len(raw),
                      "bpd": round(bs.bpd(), 5)}))


def upload_hwc(path: str, C: int) -> torch.Tensor:
    """The file's bytes on the device as they are stored, as an [H, W, C] tensor: a planar file
    is a permuted view of its upload, not a copy."""
    a, layout = read_image_stored(path, C)
    t = torch.from_numpy(np.array(a)).cuda()    # np.array: a writable buffer torch may wrap
    return t if layout == "hwc" else t.permute(1, 2, 0)


def read_image(path: str, C: int) -> np.ndarray:
    """-> uint8 [C, H, W]"""
    if path.lower().endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError(f"{path}: expected a uint8 array of 2 or 3 dimensions")
        if a.ndim == 2:
            a = a[None]
        elif a.shape[0] != C and a.shape[2] == C:  # HWC
            a = a.transpose(2, 0, 1)
        a = np.ascontiguousarray(a)
    else:
        a = _read_pnm(path)
    if a.shape[0] != C:
        raise ValueError(f"{path}: {a.shape[0]} channels, the model codes {C}")
    return a


def write_image(dirname: str, i: int, a: np.ndarray, layout: str = "chw") -> str:
    """a: uint8 [C, H, W], or [H, W, C] with layout="hwc" -- the order a PPM stores, written as
    it is.  The files are the same either way (a .npy holds [C, H, W])."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"layout {layout!r} is not 'chw' or 'hwc'")
    hwc = a if layout == "hwc" else a.transpose(1, 2, 0)
    H, W, C = hwc.shape
    if C in (1, 3):
        path = os.path.join(dirname, f"image_{i:04d}." + ("pgm" if C == 1 else "ppm"))
        with open(path, "wb") as f:
            f.write(b"%s\n%d %d\n255\n" % (b"P5" if C == 1 else b"P6", W, H))
            f.write(np.ascontiguousarray(hwc).tobytes())
    else:
        path = os.path.join(dirname, f"image_{i:04d}.npy")
        np.save(path, np.ascontiguousarray(hwc.transpose(2, 0, 1)))
    return path


def load_model(config: str, checkpoint: str | None):
    from idfcodec import configs, synthetic
    cfg = configs.load_yaml(config) if os.path.exists(config) else configs.get(config)
    model = synthetic.build_model(cfg)
    if checkpoint:
        sd = torch.load(checkpoint, map_location="cpu")
        model.load_state_dict(sd.get("model", sd) if isinstance(sd, dict) else sd)
    else:
        print("no --checkpoint: seeded synthetic weights; the round trip is exact but such "
              "weights do not compress", file=sys.stderr)
    return model.cuda()


def _seal_fields(zbs) -> dict:
    """What compress reports of a sealed file ({} for an unsealed one)."""
    if zbs is None:
        return {}
    return {"sealed": True, "fingerprint": f"{zbs.fingerprint:#010x}",
            "seal_bytes": 28 + 4 * len(zbs.crc)}


def compress_safe(out: str, files, config: str, checkpoint: str | None, ways: int = 1,
                  max_ratio: float = 1.0, check: str = "status", seal: bool = False,
                  predict: bool = False, colour: bool = False, predict_ways: int = 1,
                  smallest: bool = False, shortlist: bool = True):
    model = load_model(config, checkpoint)
    Cs = plane_set_channels(files, model.C)
    if Cs is not None:
        return compress_planes(
            out, files, model, Cs,
            dict(ways=ways, predict="colour" if colour else bool(predict),
                 predict_ways=predict_ways, seal=seal),
            dict(max_ratio=max_ratio, check=check,
                 **({"choose": "smallest" if smallest else "escaped", "shortlist": shortlist}
                    if predict else {})), predict_ways)
    imgs = [upload_hwc(p, model.C) for p in files]
    zbs = None
    if predict:  # an IDFP file, with colour an IDFQ file; with seal an IDFC file around it
        sbs = model.tiled_safe(ways=ways, predict="colour" if colour else True,
                               predict_ways=predict_ways, seal=seal).encode(
            imgs, max_ratio=max_ratio, check=check, layout="hwc",
            choose="smallest" if smallest else "escaped", shortlist=shortlist)
        if seal:
            zbs, sbs = sbs, sbs.inner
    elif seal:
        zbs = model.tiled_sealed(ways=ways, safe=True).encode(imgs, max_ratio=max_ratio,
                                                              check=check, layout="hwc")
        sbs = zbs.inner
    else:
        sbs = model.tiled_safe(ways=ways).encode(imgs, max_ratio=max_ratio, check=check,
                                                 layout="hwc")
    raw = (zbs or sbs).to_bytes()
    with open(out, "wb") as f:
        f.write(raw)
    reasons = {name: int(((sbs.reasons & bit) != 0).sum())
               for name, bit in (("status", 1), ("size", 2), ("verify", 4), ("smaller", 8))}
    packed = {"packed_tiles": sbs.n_packed} if predict else {}
    if smallest:  # per tile: the flow's bytes, the estimate, the predictor's bytes, the choice
        packed.update(choose="smallest", shortlist=shortlist, kept_tiles=sbs.n_kept,
                      predictor_coded_tiles=int((sbs.pred_bytes >= 0).sum()),
                      flow_bytes=(sbs.flow_bits // 8).tolist(), est_bytes=sbs.est_bytes.tolist(),
                      pred_bytes=sbs.pred_bytes.tolist(), choice=sbs.choice.tolist())
    if colour:
        packed["colour_tiles"] = sbs.n_colour
    if predict:
        packed["predict_ways"] = sbs.predict_ways
    n_raw = int(sbs.stored_raw.sum()) if predict else int(sbs.escaped.sum())
    share = (int(sbs.raw.numel()) / max(sbs.n_subpixels(), 1) if predict
             else sbs.escaped_share())
    print(json.dumps({"images": len(imgs), "tiles": len(sbs.escaped),
                      "raw_tiles": n_raw, **packed, "escape_reasons": reasons,
                      "source_bytes": sum(t.numel() for t in imgs), "container_bytes": len(raw),
                      "bpd": round(sbs.bpd(), 5), "escaped_share": round(share, 5),
                      "max_ratio": max_ratio, "check": check,
                      "conv": sbs.stream.meta["conv"] if sbs.stream is not None else None,
                      "ways": sbs.stream.ways if sbs.stream is not None else ways,
                      **_seal_fields(zbs)}))


def compress(out: str, files, config: str, checkpoint: str | None, ways: int = 1,
             seal: bool = False):
    model = load_model(config, checkpoint)
    Cs = plane_set_channels(files, model.C)
    if Cs is not None:
        return compress_planes(out, files, model, Cs,
                               {"ways": ways, "seal_plain" if seal else "plain": True}, {})
    imgs = [upload_hwc(p, model.C) for p in files]
    zbs = None
    if seal:
        zbs = model.tiled_sealed(ways=ways, safe=False).encode(imgs, layout="hwc")
        tbs = zbs.inner
    else:
        tbs = model.tiled(ways=ways).encode(imgs, layout="hwc")
    raw = (zbs or tbs).to_bytes()
    with open(out, "wb") as f:
        f.write(raw)
    src = sum(t.numel() for t in imgs)
    print(json.dumps({"images": len(imgs), "tiles": tbs.stream.n_images, "source_bytes": src,
                      "container_bytes": len(raw), "bpd": round(tbs.bpd(), 5),
                      "padded_share": round(tbs.padded_share(), 5),
                      "conv": tbs.stream.meta["conv"], "ways": tbs.stream.ways,
                      **_seal_fields(zbs)}))


def read_container(buf: bytes, device):
    """-> (TiledBitstream, SafeTiledBitstream or PredictiveTiledBitstream, whether its tiles may
    be escaped: one of the latter two), by the magic."""
    from idfcodec import predict, safe, tiled
    if buf[:4] in (predict.MAGIC, predict.MAGIC_COLOUR):
        return predict.PredictiveTiledBitstream.from_bytes(buf, device=device), True
    if buf[:4] == safe.MAGIC:
        return safe.SafeTiledBitstream.from_bytes(buf, device=device), True
    return tiled.TiledBitstream.from_bytes(buf, device=device), False


def read_file(buf: bytes, device):
    """-> (the bitstream, whether its tiles may be stored raw, whether it is sealed), by the
    magic: an IDFC file around an IDFT, IDFS, IDFP or IDFQ one, one of those alone, or an IDFD
    file."""
    from idfcodec import deep, integrity, tiled
    if buf[:4] == deep.MAGIC:   # 16-bit samples, no model: its raw units are its escape
        return deep.DeepTiledBitstream.from_bytes(buf, device=device), True, False
    if buf[:4] == integrity.MAGIC:
        zbs = integrity.SealedBitstream.from_bytes(buf, device=device)
        return zbs, not isinstance(zbs.inner, tiled.TiledBitstream), True
    return (*read_container(buf, device), False)


def _decode_file(path: str, model):
    """-> (bitstream, outputs [H, W, C], info, escape, sealed) of the file's decode by the codec
    its magic names, a sealed file's by its inner file's.  A sealed file written by other
    weights exits here."""
    from idfcodec import planes
    from idfcodec.predict import PredictiveTiledBitstream
    from idfcodec.safe import SafeTiledBitstream
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:4] == planes.MAGIC:  # a plane set, over the base its inner file's magic names
        bs = planes.PlaneSetBitstream.from_bytes(buf, device="cuda")
        base = None     # no base planes: no flow runs
        if isinstance(bs.base, PredictiveTiledBitstream):
            base = model.tiled_safe(predict=True)
        elif isinstance(bs.base, SafeTiledBitstream):
            base = model.tiled_safe()
        elif bs.base is not None:
            base = model.tiled()
        try:
            outs, info = model.tiled_planes(bs.Cs, base=base).decode(bs, layout="hwc")
        except ValueError as e:
            raise SystemExit(f"{path}: {e}") from None
        return bs, outs, info, "raw_tiles" in info, False
    tbs, escape, sealed = read_file(buf, "cuda")
    predict = isinstance(tbs.inner if sealed else tbs, PredictiveTiledBitstream)
    if sealed:
        try:
            zc = (model.tiled_safe(predict=predict, seal=True) if escape
                  else model.tiled_sealed(safe=False))
            outs, info = zc.decode(tbs, layout="hwc")
        except ValueError as e:
            raise SystemExit(f"{path}: {e}") from None
    else:
        outs, info = (model.tiled_safe(predict=predict) if escape
                      else model.tiled()).decode(tbs, layout="hwc")
    return tbs, outs, info, escape, sealed


def _damaged(tbs, info) -> str:
    from idfcodec.integrity import bad_tiles
    return ", ".join(f"(image {i}, tile row {ty}, tile column {tx})"
                     for i, ty, tx in bad_tiles(tbs, info["crc_bad"]))


def verify(path: str, config: str, checkpoint: str | None):
    model = load_model(config, checkpoint)
    tbs, _, info, escape, sealed = _decode_file(path, model)
    if not sealed:
        raise SystemExit(f"{path}: not a sealed file (no tile CRCs to verify)")
    from idfcodec.integrity import bad_tiles
    for i, ty, tx in bad_tiles(tbs, info["crc_bad"]):
        print(f"damaged: image {i}, tile row {ty}, tile column {tx}")
    print(json.dumps({"tiles": info["tiles"], "damaged": len(info["crc_bad"]),
                      "ok": bool(info["ok"])}))
    if not info["ok"]:
        raise SystemExit(1)


def decompress(path: str, dirname: str, config: str, checkpoint: str | None):
    with open(path, "rb") as f:
        head = f.read()
    if head[:4] == b"IDFD":     # 16-bit samples: no model
        return decompress_deep(path, head, dirname)
    model = load_model(config, checkpoint)
    tbs, outs, info, escape, sealed = _decode_file(path, model)
    if sealed and info["crc_bad"]:
        raise SystemExit(f"{path}: damaged tiles: {_damaged(tbs, info)}")
    if not info["ok"]:
        raise SystemExit(f"{path}: the decode did not verify (another model or a damaged file)")
    os.makedirs(dirname, exist_ok=True)
    names = [write_image(dirname, i, t.cpu().numpy(), layout="hwc") for i, t in enumerate(outs)]
    res = {"images": len(names), "tiles": info["tiles"], "first": names[0]}
    if escape:
        res["raw_tiles"] = info["raw_tiles"]
        if "packed_tiles" in info:
            res["packed_tiles"] = info["packed_tiles"]
    if sealed:
        res["sealed"] = True
    for k in ("constant_planes", "packed_planes", "raw_planes"):  # a plane set's extra planes
        if k in info:
            res[k] = info[k]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("bench")
    b.add_argument("--steps", type=int, default=7)
    b.add_argument("--warmup", type=int, default=2)
    b.add_argument("--escape", action="store_true",
                   help="also time SafeTiledCodec at max_ratio 1.0 and inf, and its kernels")
    b.add_argument("--seal", action="store_true",
                   help="also time the sealed codecs beside their unsealed ones (with --escape "
                        "--predict [--smallest] the predictive ones too), the CRC kernels and "
                        "the model's fingerprint")
    b.add_argument("--channels", type=int, default=None,
                   help="instead of the sets above: 4 images of 512x512 and this many channels "
                        "(1 grey, 2 grey + alpha, 4 RGBA, ...) through model.tiled_planes over "
                        "the base --escape / --predict name, beside that base alone: encode and "
                        "decode Mpx/s and the extra planes' share of the file")
    b.add_argument("--deep", action="store_true",
                   help="instead of the sets above: seeded synthetic 16-bit images through "
                        "DeepTiledCodec: bits per sample, class shares, escapes, encode and decode "
                        "Mpx/s, and the 8-bit predictive coder at one way on as many samples")
    c = sub.add_parser("compress")
    c.add_argument("out")
    c.add_argument("files", nargs="+")
    d = sub.add_parser("decompress")
    d.add_argument("inp")
    d.add_argument("dir")
    v = sub.add_parser("verify")
    v.add_argument("inp")
    c.add_argument("--seal", action="store_true",
                   help="wrap the file (IDFT, with --escape IDFS, with --predict IDFP / IDFQ) in "
                        "an IDFC container: a CRC-32 per tile and the model's fingerprint, "
                        "checked at decompress / verify")
    c.add_argument("--ways", type=int, default=1, choices=(1, 8, 16, 32, 64),
                   help="interleaved rANS states per (tile, level) stream: a shorter serial "
                        "chain for 64 more bits per extra way (decompress reads it from the file)")
    c.add_argument("--escape", action="store_true",
                   help="write an IDFS file: tiles that would not decode to the source, or cost "
                        "more than --max-ratio times their bytes, are stored raw")
    c.add_argument("--max-ratio", type=float, default=None,
                   help="with --escape: coded bits over raw bits above which a tile is stored raw "
                        "(default 1.0; inf: only tiles that would lose data)")
    c.add_argument("--check", choices=("status", "decode"), default=None,
                   help="with --escape: trust the encoder's flags (default), or also decode every "
                        "kept tile and compare it with the source")
    c.add_argument("--colour", action="store_true",
                   help="with --escape --predict: write an IDFQ file: every escaped tile is also "
                        "coded with planes 0 and 2 as differences to plane 1, and the smaller "
                        "coding is kept")
    c.add_argument("--predict", action="store_true",
                   help="with --escape: write an IDFP file: the escaped tiles are coded by a MED "
                        "predictor and rANS where that is smaller than their bytes")
    b.add_argument("--predict", action="store_true",
                   help="with --escape: also time PredictiveTileCodec at max_ratio 1.0, its two "
                        "kernels, and a smooth image set the predictor packs")
    c.add_argument("--smallest", action="store_true",
                   help="with --escape --predict: choose=\"smallest\": every tile in the smallest "
                        "of its three codings -- flow, predictor, raw -- the predictor priced on "
                        "every tile by idf_predict_cost_u8 and run where it may win")
    c.add_argument("--no-shortlist", action="store_true",
                   help="with --smallest: code every tile with the predictor, whatever its "
                        "estimate says")
    b.add_argument("--smallest", action="store_true",
                   help="with --escape --predict: also step choose=\"smallest\" with and without "
                        "the shortlist beside choose=\"escaped\"")
    c.add_argument("--predict-ways", type=int, default=1, choices=(1, 8, 16, 32, 64),
                   help="with --escape --predict: interleaved states per predictive stream, its "
                        "symbols along a pixel wavefront: a wave decodes that many pixels a step, "
                        "for 8 more bytes per extra way and packed tile (decompress reads it from "
                        "the file)")
    b.add_argument("--predict-ways", type=int, nargs="+", default=[], choices=(8, 16, 32, 64),
                   help="with --escape --predict: also step the codec at each of these beside "
                        "the one-way codec, time their kernels and the decode latency of one "
                        "packed entry")
    c.add_argument("--deep-ways", type=int, default=1, choices=(1, 8, 16, 32, 64),
                   help="16-bit sources: interleaved states per packed unit, its samples along a "
                        "pixel wavefront: a wave decodes that many samples a step, for 8 more "
                        "bytes per extra way and packed unit (decompress reads it from the file)")
    b.add_argument("--deep-ways", type=int, nargs="+", default=[], choices=(8, 16, 32, 64),
                   help="with --deep: instead, step the 16-bit codec at each of these beside the "
                        "one-way codec: file bytes, encode and decode ms, the decode kernel's "
                        "device time and the decode_region latency of one unit")
    for p in (c, d, v):
        p.add_argument("--config", default="imagenet64")
        p.add_argument("--checkpoint", default=None)
    a = ap.parse_args()
    if a.cmd == "bench":
        if a.predict and not a.escape:
            ap.error("--predict needs --escape")
        if a.predict_ways and not a.predict:
            ap.error("--predict-ways needs --escape --predict")
        if a.smallest and not a.predict:
            ap.error("--smallest needs --escape --predict")
        if a.deep_ways and not a.deep:
            ap.error("--deep-ways needs --deep")
        if a.deep:
            print(json.dumps(bench_deep(a.steps, a.warmup, ways=tuple(a.deep_ways))), flush=True)
            return
        if a.channels is not None:
            if a.channels < 1 or a.seal or a.predict_ways or a.smallest:
                ap.error("--channels N >= 1 goes with --escape and --predict alone")
            print(json.dumps(bench_planes(a.channels, a.steps, a.warmup, a.escape, a.predict)),
                  flush=True)
            return
        print(json.dumps(bench(a.steps, a.warmup, a.escape, a.seal, a.predict,
                               tuple(a.predict_ways), a.smallest)), flush=True)
    elif a.cmd == "compress" and _deep_or_not(a.files):
        compress_deep(a.out, a.files, ways=a.deep_ways)
    elif a.cmd == "compress":
        if not a.escape and (a.max_ratio is not None or a.check is not None):
            ap.error("--max-ratio and --check need --escape")
        if a.colour and not a.predict:
            ap.error("--colour needs --escape --predict")
        if a.predict_ways != 1 and not a.predict:
            ap.error("--predict-ways needs --escape --predict")
        if a.smallest and not a.predict:
            ap.error("--smallest needs --escape --predict")
        if a.no_shortlist and not a.smallest:
            ap.error("--no-shortlist needs --smallest")
        if a.predict and not a.escape:
            ap.error("--predict needs --escape")
        if a.escape:
            compress_safe(a.out, a.files, a.config, a.checkpoint, a.ways,
                          1.0 if a.max_ratio is None else a.max_ratio, a.check or "status",
                          a.seal, a.predict, a.colour, a.predict_ways, a.smallest,
                          not a.no_shortlist)
        else:
            compress(a.out, a.files, a.config, a.checkpoint, a.ways, a.seal)
    elif a.cmd == "verify":
        verify(a.inp, a.config, a.checkpoint)
    else:
        decompress(a.inp, a.dir, a.config, a.checkpoint)


if __name__ == "__main__":
    main()
