"""The raw-tile escape with a predictive coder: the tiles SafeTiledCodec stores as their bytes,
coded on the device with a MED predictor and rANS where that is smaller.

PredictiveTileCodec makes exactly SafeTiledCodec's keep-or-escape decision (idfcodec.safe) and
writes the same inner stream; then every escaped entry's in-image rectangle uint8 [C][hin][win]
is coded as one rANS stream of C * hin * win symbols (initial state L, one way) whose model is
causal and per plane (include/idf_codec.h "the predictive coder of escaped tiles" states it;
csrc/idf_predict.h holds its literals): idf_predict_prep_u8 reads the bytes where they lie,
chooses the entry's u32 `sel` (a scale per context bucket) and writes the symbols in stream
order; idf_rans_encode_streams and idf_gather_words code them as they code the flow's.  An
escaped entry is *packed* iff its stream's status is 0 and 16 + 4 * nwords < C * hin * win (sel
4, state 8, count 4 bytes; a tie stores raw); else it stays raw.  An entry's model reads nothing
outside its rectangle, so the decision, sel and the words depend on nothing but its bytes, and a
crop decodes from the tiles it touches: idf_predict_decode_u8 (one wave per entry) writes the
bytes in the raw layout and idf_tile_scatter_raw_u8 places them.

Container IDFP (little-endian): the TileLayout header with magic "IDFP" (idfcodec.tiled), the
escape bitmap (N bits in entry order, LSB first), the packed bitmap (E bits over the escaped
entries in entry order, LSB first), u64 raw length, the raw bytes of the escaped entries that are
not packed, u64 packed-section length, the packed section -- u32 P, u32 sel[P], u64 state[P], u32
nwords[P], then the words as u32 in entry order and push order -- u64 inner length, the inner
IDFB container over the kept entries (length 0 and absent when none is kept).

The colour mode (PredictiveTileCodec(model, colour=True), C >= 3; include/idf_codec.h "colour
entries" states the model): every escaped entry is coded twice in one pass -- as above, and with
planes 0 and 2 replaced by their difference to plane 1 mod 256 and a second scale table sel2 for
those two planes (idf_predict_prep2_u8 writes both candidates' symbols, the encoder runs once over
twice as many streams) -- and the entry is a *colour* entry iff 20 + 4 * nw_c < 16 + 4 * nw_p (a
tie stays plain); it is packed iff the smaller cost is below its bytes.  Every entry then costs at
most what it costs without the mode.  idf_predict_decode2_u8 decodes plain and colour entries in
one launch and undoes the transform in place.

Container IDFQ: IDFP's layout with magic "IDFQ" and two additions: the colour bitmap (P bits over
the packed entries in entry order, LSB first) follows the packed bitmap, and u32 Q, u32 sel2[Q]
(the colour entries in entry order) lie between nwords[P] and the words.  A colour entry's sel,
state, count and words are those of its colour stream.  IDFP files are written (colour=False) and
read as before; from_bytes tells the two by their magic.

Interleaved streams (PredictiveTileCodec(model, predict_ways=N), N in 8, 16, 32, 64; include/
idf_codec.h "interleaved predictive streams" states the order): the same symbols, ordered along a
pixel wavefront -- rows rho = ch * hin + y in bands of N, pixel (rho, x) at step (rho // N) *
max(win, N) + rho % N + x, slot rho % N, ascending (step, slot) -- so that the symbols of a step
are independent, and coded by N states (idf_rans_encode_streams_ways).  A packed entry then costs
8 + 8 N + 4 * nwords bytes (a colour entry 4 more) and idf_predict_decode_ways_u8 decodes a step
of up to N pixels at once.  The header's u16 flags holds N (0 for one way, whose files are byte
for byte as before) and the packed section's states are u64 [P][N], entry-major and way-minor.
Decode follows the file's own N.

The smallest coding (encode(..., choose="smallest"); PredictiveTileCodec.encode has the rule): an
entry SafeTiledCodec would keep is still escaped where the predictor or its bytes are smaller than
the flow's streams.  idf_predict_cost_u8 prices the predictor on every entry without coding it --
per symbol 24 * 256 - log2_q8(the encoder's own frequency), in integers -- and only the entries
whose estimate is below the flow's cost are coded; the choice itself is made on the actual word
counts (final_choice).  The decision lives in the escape and packed bitmaps, so the files are
ordinary IDFP / IDFQ files and the decoder derives nothing.

Sealed files (idfcodec.integrity.SealedCodec around this codec, container IDFC): the IDFP / IDFQ
file is wrapped untouched with a CRC-32 of every entry's source bytes and the model's fingerprint.
_decode_entries then takes the seal's check along: the kept and the raw entries are summed as
SafeTiledCodec has it, a packed entry by idf_crc32_segments_u8 over its run of the dense buffer
the decoders above fill, once they have left the source bytes there; the runs' table rides in the
copy that brings the word offsets, counts, output offsets and states to the device.
"""
from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import RANS_L, Bitstream
from .dist import _to_device
from .safe import (REASON_SMALLER, SafeTiledBitstream, SafeTiledCodec, _check_kept,
                   _read_inner, device_gather_raw, device_scatter_raw, file_size_bound,
                   raw_offsets)
from .tiled import (Reader, TileLayout, _ceil_div, _check_table, _TiledSizes, check_words,
                    pack_bitmap, pack_lengthed, pack_words, read_words)

MAGIC = b"IDFP"
NAME = "predictive tiled bitstream"
ENTRY_BYTES = 16            # what a packed entry adds besides its words: sel 4, state 8, count 4
SYMBOLS_PER_PASS = 1 << 22  # the encoder's working set: 40 bytes a symbol, both candidates counted
MAGIC_COLOUR = b"IDFQ"
NAME_COLOUR = "colour predictive tiled bitstream"
ENTRY_BYTES_COLOUR = 20     # a colour entry adds sel2
COLOUR_MIN_C = 3
PREDICT_WAYS = (1, 8, 16, 32, 64)   # states per predictive stream; the header's flags hold N > 1


def check_predict_ways(ways) -> int:
    """predict_ways as an int, or ValueError unless the kernels code it (PREDICT_WAYS)."""
    if isinstance(ways, bool) or not isinstance(ways, (int, np.integer)) or \
            int(ways) not in PREDICT_WAYS:
        raise ValueError(f"predict_ways {ways!r} is not one of {PREDICT_WAYS}")
    return int(ways)


def entry_overhead(ways: int = 1, colour: bool = False) -> int:
    """What a packed entry adds besides its words: sel 4, count 4, 8 a state; sel2 4 more."""
    return 8 + 8 * int(ways) + (4 if colour else 0)


def order(C: int, hin: int, win: int, ways: int) -> np.ndarray:
    """int64 [C, hin, win]: the rank q of every pixel in the wavefront order of `ways` states
    (idf_predict_order; host only, no device).  Pixel q is symbol C * hin * win - 1 - q."""
    q = np.empty(int(C) * int(hin) * int(win), dtype=np.int64)
    check(lib().idf_predict_order(int(C), int(hin), int(win), int(ways),
                                  q.ctypes.data_as(ctypes.c_void_p)), "idf_predict_order")
    return q.reshape(int(C), int(hin), int(win))


def ways_supported(C: int, th: int, tw: int, ways: int) -> bool:
    """Whether idf_predict_decode_ways_u8 decodes tiles of C x th x tw at `ways` > 1
    (idf_predict_ways_supported; host only): False where an entry does not fit its LDS."""
    rc = lib().idf_predict_ways_supported(int(C), int(th), int(tw), int(ways))
    if rc == _lib.IDF_ERR_UNSUPPORTED:
        return False
    check(rc, "idf_predict_ways_supported")
    return True


# ------------------------------------------------------------------ host arithmetic
def tables():
    """-> (the 16 f32 scale candidates, the 15 int64 thresholds) of csrc/idf_predict.h
    (idf_predict_tables; host only, no device)."""
    scale = (ctypes.c_float * 16)()
    t = (ctypes.c_int64 * 15)()
    check(lib().idf_predict_tables(scale, t), "idf_predict_tables")
    return np.array(scale, dtype=np.float32), np.array(t, dtype=np.int64)


def is_packed(status, nwords, n_bytes, ways: int = 1) -> np.ndarray:
    """bool per escaped entry: the stream decodes (status 0) and the entry's 8 + 8 * ways bytes
    (16 with one way) plus its words are fewer than its raw bytes.  A tie stores raw."""
    nw = np.asarray(nwords, dtype=np.int64)
    return ((np.asarray(status) == 0)
            & (entry_overhead(ways) + 4 * nw < np.asarray(n_bytes, dtype=np.int64)))


def entry_bytes(rects, C: int) -> np.ndarray:
    """int64 per entry: C * hin * win"""
    return int(C) * np.array([h * w for h, w in rects], dtype=np.int64).reshape(len(rects))


def is_colour(nwords_plain, nwords_colour) -> np.ndarray:
    """bool per escaped entry: its colour stream with 20 bytes costs less than its plain stream
    with 16.  A tie stays plain."""
    return (ENTRY_BYTES_COLOUR + 4 * np.asarray(nwords_colour, dtype=np.int64)
            < ENTRY_BYTES + 4 * np.asarray(nwords_plain, dtype=np.int64))


def file_size_bound_packed(sizes, C: int, th: int, tw: int, levels: int, kept: bool = True,
                           colour: bool = False) -> int:
    """The bytes an IDFP file coded with max_ratio <= 1 cannot exceed: safe.file_size_bound (a
    packed entry costs less than its raw bytes, so the raw and packed bytes together stay within
    the escaped entries' source bytes) plus the packed bitmap (at most ceil(N / 8) bytes), the
    packed section's u64 length and its u32 count.  colour: an IDFQ file's -- a colour entry's 20
    bytes and words are fewer than its raw bytes too -- which adds the colour bitmap (at most
    ceil(N / 8) bytes) and the u32 count of sel2."""
    N = TileLayout(sizes, C, (th, tw)).n_tiles
    bound = file_size_bound(sizes, C, th, tw, levels, kept) + _ceil_div(N, 8) + 8 + 4
    return bound + (_ceil_div(N, 8) + 4 if colour else 0)


# ------------------------------------------------------------------ the smallest coding
CHOICE_FLOW, CHOICE_PREDICT, CHOICE_RAW = 0, 1, 2
COST_ONE = 24 * 256         # a symbol of frequency 1 of 2^24, in 1/256 bit
COST_WORD = 32 * 256        # a word of the stream


def log2_q8(freq) -> np.ndarray:
    """int32 per value: log2 in 1/256 bit by integers alone (idf_predict_log2_q8; host only, no
    device), the cost kernel's: 0 <= 256 log2(f) - log2_q8(f) < 1 + 2^-13, log2_q8(0) = 0."""
    f = np.ascontiguousarray(np.asarray(freq, dtype=np.uint32).reshape(-1))
    out = np.empty(f.size, dtype=np.int32)
    check(lib().idf_predict_log2_q8(f.ctypes.data_as(ctypes.c_void_p), f.size,
                                    out.ctypes.data_as(ctypes.c_void_p)), "idf_predict_log2_q8")
    return out


def estimate_bytes(cost_q8, ways: int = 1, colour: bool = False) -> np.ndarray:
    """cost_q8: int64 [N, 2] of idf_predict_cost_u8 -> int64 [N], what the predictor is expected
    to cost an entry in a file: its overhead + 4 * floor(cost / 8192), the words of a stream of
    that many bits.  colour: the smaller of the two candidates with their own overheads (a tie
    stays plain, as is_colour has it)."""
    c = np.asarray(cost_q8, dtype=np.int64).reshape(-1, 2)
    est = entry_overhead(ways) + 4 * (c[:, 0] // COST_WORD)
    if colour:
        est_c = entry_overhead(ways, True) + 4 * (c[:, 1] // COST_WORD)
        est = np.where(est_c < est, est_c, est)
    return est


def predictor_codes(eligible, flow_bits, est_bytes=None, choose: str = "escaped",
                    shortlist: bool = True) -> np.ndarray:
    """bool [N]: the entries the predictor codes.  Those the keep rule does not keep (not
    `eligible`), always; with choose="smallest" the kept ones too -- all of them without the
    shortlist, with it those whose estimate is below the flow's cost, 8 * est_bytes < flow_bits."""
    el = np.asarray(eligible, dtype=bool)
    if choose == "escaped":
        return ~el
    if not shortlist:
        return np.ones(len(el), dtype=bool)
    return ~el | (8 * np.asarray(est_bytes, dtype=np.int64) < np.asarray(flow_bits, dtype=np.int64))


def final_choice(eligible, flow_bits, raw_bytes, pred_ok, pred_bytes,
                 choose: str = "escaped") -> np.ndarray:
    """uint8 [N] of CHOICE_*, from the actual numbers alone.  pred_ok: the predictor coded the
    entry and its status is 0; pred_bytes: what it then costs (its overhead and words).
    choose="escaped": an eligible entry is the flow's; another is the predictor's iff pred_ok and
    pred_bytes < raw_bytes (is_packed), else raw.
    choose="smallest": the smallest of flow_bits (eligible entries), 8 * pred_bytes (pred_ok) and
    8 * raw_bytes wins; a tie goes to the flow, then to raw."""
    el = np.asarray(eligible, dtype=bool)
    fb = np.asarray(flow_bits, dtype=np.int64)
    raw = 8 * np.asarray(raw_bytes, dtype=np.int64)
    pb = 8 * np.asarray(pred_bytes, dtype=np.int64)
    packs = np.asarray(pred_ok, dtype=bool) & (pb < raw)    # a tie stores raw
    rest = np.where(packs, pb, raw)                         # the best coding that is not the flow
    flow = el if choose == "escaped" else el & (fb <= rest)
    return np.where(flow, CHOICE_FLOW, np.where(packs, CHOICE_PREDICT, CHOICE_RAW)).astype(np.uint8)


def device_predict_cost(table: torch.Tensor, n: int, C: int, th: int, tw: int,
                        colour: bool = False) -> torch.Tensor:
    """The predictor's cost of the n tiles the table names, without coding them -> device int64
    [n, 2] in 1/256 bit: the plain candidate's, and the colour candidate's or 0
    (idf_predict_cost_u8; asynchronous)."""
    if _check_table(table, n) != 5:
        raise ValueError("the predictor reads dense planar tiles: table rows of five fields")
    cost = torch.empty((n, 2), dtype=torch.int64, device=table.device)
    check(lib().idf_predict_cost_u8(_lib.stream_ptr(table.device), n, C, th, tw, ptr(table),
                                    int(bool(colour)), ptr(cost)), "predict cost")
    return cost


# ------------------------------------------------------------------ device calls
def device_predict_prep(table: torch.Tensor, n: int, C: int, th: int, tw: int,
                        sym_off: torch.Tensor, sel: torch.Tensor, x: torch.Tensor,
                        mean: torch.Tensor, scale: torch.Tensor, ways: int = 1):
    """The n tiles the table names -> sel[t] and their symbols (x, mean, scale: float32, stream
    order) at sym_off[t] (idf_predict_prep_u8).  sym_off: int64 [n + 1] built from the same
    table: entry t holds C * hin * win symbols.  ways > 1: in the wavefront order of that many
    states (idf_predict_prep_ways_u8)."""
    _check_table(table, n)
    _lib.require_device(sym_off, "symbol offsets")
    if sym_off.dtype != torch.int64 or not sym_off.is_contiguous() or sym_off.numel() < n + 1:
        raise ValueError("symbol offsets must be contiguous int64 [n_tiles + 1]")
    _lib.require_device(sel, "sel")
    if sel.dtype != torch.int32 or not sel.is_contiguous() or sel.numel() < n:
        raise ValueError("sel must be contiguous int32 [n_tiles]")
    for name, t in (("x", x), ("mean", mean), ("scale", scale)):
        _lib.require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != x.numel():
            raise ValueError(f"{name} must be contiguous float32, one value per symbol")
    if ways != 1:
        check(lib().idf_predict_prep_ways_u8(_lib.stream_ptr(x.device), n, C, th, tw, ptr(table),
                                             ptr(sym_off), ptr(sel), ptr(x), ptr(mean),
                                             ptr(scale), int(ways)), "predict prep")
        return
    check(lib().idf_predict_prep_u8(_lib.stream_ptr(x.device), n, C, th, tw, ptr(table),
                                    ptr(sym_off), ptr(sel), ptr(x), ptr(mean), ptr(scale)),
          "predict prep")


def device_predict_decode(n: int, C: int, th: int, tw: int, words: torch.Tensor,
                          word_off: torch.Tensor, nwords: torch.Tensor, states: torch.Tensor,
                          sel: torch.Tensor, rect: torch.Tensor, out_off: torch.Tensor,
                          out: torch.Tensor, final_states: torch.Tensor, status: torch.Tensor):
    """n predictive streams -> their bytes uint8 [C][hin][win] at out[out_off[t]:]
    (idf_predict_decode_u8; asynchronous).  The caller sizes out and the words from the same
    tables: entry t reads words[word_off[t]:word_off[t] + nwords[t]] and writes C * hin * win
    bytes."""
    for name, t, dt, m in (("words", words, torch.int32, 1), ("word offsets", word_off,
                                                              torch.int64, n),
                           ("word counts", nwords, torch.int64, n),
                           ("states", states, torch.int64, n), ("sel", sel, torch.int32, n),
                           ("rectangles", rect, torch.int32, 2 * n),
                           ("output offsets", out_off, torch.int64, n),
                           ("output bytes", out, torch.uint8, 1),
                           ("final states", final_states, torch.int64, n),
                           ("status", status, torch.int32, n)):
        _lib.require_device(t, name)
        if t.dtype != dt or not t.is_contiguous() or t.numel() < m:
            raise ValueError(f"{name} must be contiguous {dt} of at least {m} values")
    check(lib().idf_predict_decode_u8(_lib.stream_ptr(out.device), n, C, th, tw, ptr(words),
                                      ptr(word_off), ptr(nwords), ptr(states), ptr(sel),
                                      ptr(rect), ptr(out_off), ptr(out), ptr(final_states),
                                      ptr(status)), "predict decode")


def device_predict_encode(table: torch.Tensor, counts, C: int, th: int, tw: int, ways: int = 1):
    """The predictive streams of the tiles the table names, counts[t] = C * hin * win symbols
    each -> (sel uint32 [n], states uint64 [n] ([n, ways] with ways > 1), nwords int64 [n],
    status int32 [n] as numpy, the words int32 [sum nwords] on the device, entry order and push
    order).  One pass: the caller bounds sum(counts)."""
    dev, n = table.device, len(counts)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off_h[1:])
    nsym = int(off_h[-1])
    off = _to_device(torch.from_numpy(off_h), dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    x, mean, scale = (torch.empty(max(nsym, 1), dtype=torch.float32, device=dev)
                      for _ in range(3))
    device_predict_prep(table, n, C, th, tw, off, sel, x, mean, scale, ways)
    states, nw_h, status, words = _code_streams(off, off_h, x, mean, scale, ways=ways)
    return sel.cpu().numpy().view(np.uint32), states, nw_h, status, words


def _code_streams(off: torch.Tensor, off_h: np.ndarray, x, mean, scale, keep=None,
                  ways: int = 1):
    """The streams of symbols [off[k], off[k + 1]) of (x, mean, scale), initial state L, one way
    -> (states uint64, nwords int64, status int32 as numpy, the words int32 on the device in
    stream order and push order): one idf_rans_encode_streams, one idf_gather_words.
    ways > 1: idf_rans_encode_streams_ways codes them, the states are uint64 [n, ways].
    keep(nwords, status) -> the streams whose words are wanted, in rising order (default: all):
    the gather then compacts those alone."""
    dev, n, nsym = x.device, len(off_h) - 1, int(off_h[-1])
    init = torch.full((n,), RANS_L, dtype=torch.int64, device=dev)
    final = torch.empty(n * ways, dtype=torch.int64, device=dev)
    scratch = torch.empty(max(nsym, 1), dtype=torch.int32, device=dev)
    nwords = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    wbytes = int(lib().idf_rans_encode_workspace_bytes(nsym))
    wsp = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)
    if ways != 1:
        check(lib().idf_rans_encode_streams_ways(s, int(ways), n, nsym, ptr(off), ptr(x),
                                                 ptr(mean), ptr(scale), ptr(final), ptr(scratch),
                                                 ptr(nwords), ptr(status), ptr(wsp), wbytes),
              "predict rans encode")
    else:
        check(lib().idf_rans_encode_streams(s, n, nsym, ptr(off), ptr(x), ptr(mean), ptr(scale),
                                            ptr(init), ptr(final), ptr(scratch), ptr(nwords),
                                            ptr(status), ptr(wsp), wbytes), "predict rans encode")
    nw_h = nwords.to("cpu").numpy()  # the one sync: the compacted size
    status_h = status.cpu().numpy()
    src_off, m = off, n
    if keep is not None:  # the chosen streams' offsets and counts, a few values a stream
        idx = np.asarray(keep(nw_h, status_h), dtype=np.int64)
        m = len(idx)
        src_off = _to_device(torch.from_numpy(off_h[idx]), dev)
        nwords = _to_device(torch.from_numpy(nw_h[idx]), dev)
    dst_h = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(nw_h if keep is None else nw_h[idx], out=dst_h[1:])
    total = int(dst_h[-1])
    dst_off = _to_device(torch.from_numpy(dst_h[:m].copy()), dev)
    words = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if m:
        check(lib().idf_gather_words(s, m, ptr(src_off), ptr(nwords), ptr(dst_off), ptr(scratch),
                                     ptr(words)), "predict gather words")
    states = final.cpu().numpy().view(np.uint64)
    return states if ways == 1 else states.reshape(n, ways), nw_h, status_h, words[:total]


def device_predict_prep2(table: torch.Tensor, n: int, C: int, th: int, tw: int,
                         sym_off: torch.Tensor, sel: torch.Tensor, x: torch.Tensor,
                         mean: torch.Tensor, scale: torch.Tensor, ways: int = 1):
    """Both candidates of the n tiles the table names (idf_predict_prep2_u8; C >= 3): stream 2t
    is tile t's plain candidate, stream 2t + 1 its colour candidate; sym_off: int64 [2 n + 1];
    sel: int32 [n, 3] = (the plain sel, the colour sel, the colour sel2)."""
    _check_table(table, n)
    _lib.require_device(sym_off, "symbol offsets")
    if sym_off.dtype != torch.int64 or not sym_off.is_contiguous() or sym_off.numel() < 2 * n + 1:
        raise ValueError("symbol offsets must be contiguous int64 [2 * n_tiles + 1]")
    _lib.require_device(sel, "sel")
    if sel.dtype != torch.int32 or not sel.is_contiguous() or sel.numel() < 3 * n:
        raise ValueError("sel must be contiguous int32 [n_tiles, 3]")
    for name, t in (("x", x), ("mean", mean), ("scale", scale)):
        _lib.require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != x.numel():
            raise ValueError(f"{name} must be contiguous float32, one value per symbol")
    if ways != 1:  # the wavefront order of that many states (idf_predict_prep2_ways_u8)
        check(lib().idf_predict_prep2_ways_u8(_lib.stream_ptr(x.device), n, C, th, tw,
                                              ptr(table), ptr(sym_off), ptr(sel), ptr(x),
                                              ptr(mean), ptr(scale), int(ways)),
              "predict prep of both candidates")
        return
    check(lib().idf_predict_prep2_u8(_lib.stream_ptr(x.device), n, C, th, tw, ptr(table),
                                     ptr(sym_off), ptr(sel), ptr(x), ptr(mean), ptr(scale)),
          "predict prep of both candidates")


def choose_streams(nwords, status, counts, ways: int = 1):
    """From both candidates' word counts and status [2 n] and the entries' bytes [n] -> (colour
    bool [n], pick int64 [n]: the stream of each entry's cheaper candidate, packed bool [n]: that
    candidate's cost is below the entry's bytes and its status 0)."""
    nw = np.asarray(nwords, dtype=np.int64)
    col = is_colour(nw[0::2], nw[1::2])
    pick = 2 * np.arange(len(col), dtype=np.int64) + col
    cost = np.where(col, entry_overhead(ways, True), entry_overhead(ways)) + 4 * nw[pick]
    hit = (np.asarray(status)[pick] == 0) & (cost < np.asarray(counts, dtype=np.int64))
    return col, pick, hit


def device_predict_encode2(table: torch.Tensor, counts, C: int, th: int, tw: int,
                           best: bool = False, ways: int = 1):
    """device_predict_encode for both candidates of every tile in one pass -> (sel uint32 [n, 3]
    as device_predict_prep2 orders it, states uint64 [2 n], nwords int64 [2 n], status int32
    [2 n] as numpy, the words int32 on the device): stream 2t is tile t's plain candidate, 2t + 1
    its colour candidate.  best: the words are those of the streams choose_streams picks and
    packs alone, in entry order -- the one gather compacts nothing else.  The caller bounds
    2 * sum(counts)."""
    dev, n = table.device, len(counts)
    off_h = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(np.repeat(np.asarray(counts, dtype=np.int64), 2), out=off_h[1:])
    nsym = int(off_h[-1])
    off = _to_device(torch.from_numpy(off_h), dev)
    sel = torch.empty((n, 3), dtype=torch.int32, device=dev)
    x, mean, scale = (torch.empty(max(nsym, 1), dtype=torch.float32, device=dev)
                      for _ in range(3))
    device_predict_prep2(table, n, C, th, tw, off, sel, x, mean, scale, ways)
    def chosen(nw, status):
        _, pick, hit = choose_streams(nw, status, counts, ways)
        return pick[hit]
    states, nw_h, status, words = _code_streams(off, off_h, x, mean, scale,
                                                chosen if best else None, ways=ways)
    return sel.cpu().numpy().view(np.uint32), states, nw_h, status, words


def device_predict_decode2(n: int, C: int, th: int, tw: int, words: torch.Tensor,
                           word_off: torch.Tensor, nwords: torch.Tensor, states: torch.Tensor,
                           sel: torch.Tensor, sel2: torch.Tensor | None,
                           colour: torch.Tensor | None, n_colour: int, rect: torch.Tensor,
                           out_off: torch.Tensor, out: torch.Tensor, final_states: torch.Tensor,
                           status: torch.Tensor):
    """device_predict_decode over plain and colour entries (idf_predict_decode2_u8; asynchronous):
    colour uint8 [n] flags the colour entries, n_colour of them, and sel2 int32 [n] holds their
    second table; with n_colour == 0 neither is read."""
    checks = [("words", words, torch.int32, 1), ("word offsets", word_off, torch.int64, n),
              ("word counts", nwords, torch.int64, n), ("states", states, torch.int64, n),
              ("sel", sel, torch.int32, n), ("rectangles", rect, torch.int32, 2 * n),
              ("output offsets", out_off, torch.int64, n), ("output bytes", out, torch.uint8, 1),
              ("final states", final_states, torch.int64, n), ("status", status, torch.int32, n)]
    if n_colour:
        checks += [("sel2", sel2, torch.int32, n), ("colour flags", colour, torch.uint8, n)]
    for name, t, dt, m in checks:
        _lib.require_device(t, name)
        if t.dtype != dt or not t.is_contiguous() or t.numel() < m:
            raise ValueError(f"{name} must be contiguous {dt} of at least {m} values")
    check(lib().idf_predict_decode2_u8(_lib.stream_ptr(out.device), n, int(n_colour), C, th, tw,
                                       ptr(words), ptr(word_off), ptr(nwords), ptr(states),
                                       ptr(sel), ptr(sel2), ptr(colour), ptr(rect), ptr(out_off),
                                       ptr(out), ptr(final_states), ptr(status)),
          "predict decode of plain and colour entries")


def device_predict_decode_ways(n: int, ways: int, C: int, th: int, tw: int, words: torch.Tensor,
                               word_off: torch.Tensor, nwords: torch.Tensor,
                               states: torch.Tensor, sel: torch.Tensor,
                               sel2: torch.Tensor | None, colour: torch.Tensor | None,
                               n_colour: int, rect: torch.Tensor, out_off: torch.Tensor,
                               out: torch.Tensor, final_states: torch.Tensor,
                               status: torch.Tensor):
    """device_predict_decode2 over streams of `ways` interleaved states in the wavefront order
    (idf_predict_decode_ways_u8; asynchronous): states and final_states hold n * ways values,
    entry-major and way-minor."""
    checks = [("words", words, torch.int32, 1), ("word offsets", word_off, torch.int64, n),
              ("word counts", nwords, torch.int64, n),
              ("states", states, torch.int64, n * ways), ("sel", sel, torch.int32, n),
              ("rectangles", rect, torch.int32, 2 * n),
              ("output offsets", out_off, torch.int64, n), ("output bytes", out, torch.uint8, 1),
              ("final states", final_states, torch.int64, n * ways),
              ("status", status, torch.int32, n)]
    if n_colour:
        checks += [("sel2", sel2, torch.int32, n), ("colour flags", colour, torch.uint8, n)]
    for name, t, dt, m in checks:
        _lib.require_device(t, name)
        if t.dtype != dt or not t.is_contiguous() or t.numel() < m:
            raise ValueError(f"{name} must be contiguous {dt} of at least {m} values")
    check(lib().idf_predict_decode_ways_u8(_lib.stream_ptr(out.device), n, int(n_colour),
                                           int(ways), C, th, tw, ptr(words), ptr(word_off),
                                           ptr(nwords), ptr(states), ptr(sel), ptr(sel2),
                                           ptr(colour), ptr(rect), ptr(out_off), ptr(out),
                                           ptr(final_states), ptr(status)),
          "predict decode of interleaved streams")


def passes(counts, limit: int = None):
    """counts: the symbols of every unit, in order -> yields (k, m): units k .. k + m - 1 are
    one pass, as many as stay within `limit` symbols (default: SYMBOLS_PER_PASS, as it stands at
    the call); a single unit above the limit is a pass of its own."""
    limit = SYMBOLS_PER_PASS if limit is None else limit
    k = 0
    while k < len(counts):
        m, n = 1, int(counts[k])
        while k + m < len(counts) and n + int(counts[k + m]) <= limit:
            n += int(counts[k + m])
            m += 1
        yield k, m
        k += m


def _pick_words(words: torch.Tensor, nwords, have, use, dev) -> torch.Tensor:
    """words: the streams of the entries `have` flags, in entry order (nwords[k] words of entry
    k) -> those of the entries `use` flags, a subset of them."""
    have, use = np.asarray(have, dtype=bool), np.asarray(use, dtype=bool)
    if np.array_equal(have, use):
        return words
    off = np.zeros(len(have) + 1, dtype=np.int64)
    np.cumsum(np.where(have, np.asarray(nwords, dtype=np.int64), 0), out=off[1:])
    idx = [np.arange(off[k], off[k + 1]) for k in np.flatnonzero(use)]
    if not idx:
        return words[:0]
    return words[_to_device(torch.from_numpy(np.concatenate(idx)), dev)]


# ------------------------------------------------------------------ container
def packed_index(escaped, packed) -> list:
    """entry -> its index among the packed entries, -1 if it is not packed"""
    out, k = [], 0
    for e, p in zip(escaped, packed):
        hit = bool(e) and bool(p)
        out.append(k if hit else -1)
        k += 1 if hit else 0
    return out


def pack_tables(P: int, sel, states, nwords) -> bytes:
    """The tables IDFP, IDFQ and IDFM open their packed section with: u32 P, u32 sel[P], u64
    state[P] ([P][ways]), u32 nwords[P]."""
    return (struct.pack("<I", P) + np.asarray(sel, dtype="<u4").tobytes()
            + np.asarray(states, dtype="<u8").tobytes()
            + np.asarray(nwords, dtype=np.int64).astype("<u4").tobytes())


def read_count(s: Reader, n_sect: int, n_packed: int, of: str) -> int:
    """s: at the start of a packed section of n_sect bytes -> the u32 count P it opens with,
    which must be the n_packed `of` (tiles, units) the packed bitmap flags."""
    if n_sect < 4:
        raise ValueError(f"{s.name} holds a packed section of {n_sect} bytes, too short for "
                         "its count")
    P = s.u32()
    if P != n_packed:
        raise ValueError(f"{s.name} names {P} packed {of}, its bitmap {n_packed}")
    return P


def read_tables(s: Reader, n_sect: int, n_packed: int, W: int, of: str):
    """s: at the start of a packed section of n_sect bytes whose bitmap flags n_packed `of`, W
    states each -> (sel uint32 [P], states uint64 [P] or [P, W], nwords int64 [P], the bytes of
    these tables, the count included)."""
    P = read_count(s, n_sect, n_packed, of)
    n_tab = 4 + entry_overhead(W) * P      # the count; sel 4, W states, count 4 a row
    if n_sect < n_tab:
        raise ValueError(f"{s.name} holds a packed section of {n_sect} bytes, too short for "
                         f"the tables of {P} {of}" + (f" of {W} ways" if W > 1 else ""))
    sel = s.array("<u4", P).astype(np.uint32)
    states = s.array("<u8", P * W).astype(np.uint64)
    nwords = s.array("<u4", P).astype(np.int64)
    return sel, states.reshape(P, W) if W > 1 else states, nwords, n_tab


def read_section_words(s: Reader, n_sect: int, n_tab: int, nwords, W: int) -> torch.Tensor:
    """The words a packed section of n_sect bytes ends with, behind n_tab bytes of tables."""
    total = int(nwords.sum())
    if n_sect != n_tab + 4 * total:
        raise ValueError(f"{s.name} holds a packed section of {n_sect} bytes, its word counts "
                         f"name {total} words: {n_tab + 4 * total} bytes"
                         + (f" at {W} ways" if W > 1 else ""))
    return read_words(s, total)


@dataclass
class PredictiveTiledBitstream(_TiledSizes):
    stream: Bitstream | None    # the K kept entries in entry order; None when K == 0
    sizes: list                 # [(H, W)] per image
    C: int
    tile_hw: tuple              # (th, tw)
    escaped: np.ndarray         # bool [N], entry order
    packed: np.ndarray          # bool [N]: escaped and coded by the predictor
    raw: torch.Tensor           # uint8: the escaped, not packed entries' bytes, entry order
    sel: np.ndarray             # uint32 [P], the packed entries in entry order
    states: np.ndarray          # uint64 [P]
    nwords: np.ndarray          # int64 [P]
    words: torch.Tensor         # int32 [sum nwords]: entry order, push order
    reasons: np.ndarray | None = None   # uint8 [N] of safe.REASON_* from encode; not serialised
    colour: np.ndarray | None = None    # bool [N]: packed as a colour entry; None: an IDFP stream
    sel2: np.ndarray | None = None      # uint32 [Q], the colour entries in entry order
    predict_ways: int = 1               # states per packed entry; > 1: states is uint64 [P, ways]
    # what encode saw, per entry; not serialised
    flow_bits: np.ndarray | None = None     # int64 [N]: safe.entry_bits of the flow's streams
    est_bytes: np.ndarray | None = None     # int64 [N]: estimate_bytes; -1 with choose="escaped"
    pred_bytes: np.ndarray | None = None    # int64 [N]: overhead + 4 * nwords; -1 where not coded

    @property
    def magic(self) -> bytes:
        return MAGIC if self.colour is None else MAGIC_COLOUR

    @property
    def n_colour(self) -> int:
        return 0 if self.colour is None else int(np.count_nonzero(self.colour))

    @property
    def n_entries(self) -> int:
        return len(self.escaped)

    @property
    def n_kept(self) -> int:
        return int(self.n_entries - int(np.count_nonzero(self.escaped)))

    @property
    def n_packed(self) -> int:
        return int(np.count_nonzero(self.packed))

    @property
    def stored_raw(self) -> np.ndarray:
        """bool [N]: escaped and stored as bytes"""
        return np.asarray(self.escaped, dtype=bool) & ~np.asarray(self.packed, dtype=bool)

    @property
    def choice(self) -> np.ndarray:
        """uint8 [N] of CHOICE_*: the coding every entry is stored in"""
        return np.where(np.asarray(self.packed, dtype=bool), CHOICE_PREDICT,
                        np.where(np.asarray(self.escaped, dtype=bool), CHOICE_RAW,
                                 CHOICE_FLOW)).astype(np.uint8)

    def rects(self) -> list:
        return self.layout.rects

    def bits(self) -> int:
        """The inner stream's bits + 8 per raw byte + 64 + 64 * predict_ways + 32 per word of
        every packed entry (32 more of a colour entry)."""
        return ((self.stream.bits() if self.stream is not None else 0) + 8 * int(self.raw.numel())
                + 8 * entry_overhead(self.predict_ways) * self.n_packed
                + 32 * int(np.sum(self.nwords))
                + 8 * (ENTRY_BYTES_COLOUR - ENTRY_BYTES) * self.n_colour)

    def check(self):
        """Raises unless the parts fit each other."""
        lay, N = self.layout, self.n_entries
        if N != lay.n_tiles or len(self.packed) != N:
            raise ValueError(f"{N} escape and {len(self.packed)} packed flags for "
                             f"{lay.n_tiles} tiles")
        if (np.asarray(self.packed, dtype=bool) & ~np.asarray(self.escaped, dtype=bool)).any():
            raise ValueError(f"{NAME} packs a tile it keeps")
        _, n_raw = raw_offsets(self.stored_raw, lay.rects, self.C)
        if self.raw.dtype != torch.uint8 or int(self.raw.numel()) != n_raw:
            raise ValueError(f"{NAME} holds {self.raw.numel()} raw bytes, its raw tiles "
                             f"{n_raw}")
        P, W = self.n_packed, check_predict_ways(self.predict_ways)
        if not (len(self.sel) == len(self.states) == len(self.nwords) == P):
            raise ValueError(f"{NAME} packs {P} tiles, its tables hold {len(self.sel)}, "
                             f"{len(self.states)} and {len(self.nwords)} rows")
        if int(np.asarray(self.states).size) != P * W:
            raise ValueError(f"{NAME} packs {P} tiles of {W} ways, its states number "
                             f"{int(np.asarray(self.states).size)}")
        check_words(NAME, self.nwords, self.words)
        if self.colour is None:
            if self.sel2 is not None and len(self.sel2):
                raise ValueError(f"{NAME} holds {len(self.sel2)} second tables and no colour "
                                 "flags")
            return
        if len(self.colour) != N:
            raise ValueError(f"{len(self.colour)} colour flags for {N} tiles")
        if (np.asarray(self.colour, dtype=bool) & ~np.asarray(self.packed, dtype=bool)).any():
            raise ValueError(f"{NAME_COLOUR} flags a tile it does not pack")
        n_sel2 = 0 if self.sel2 is None else len(self.sel2)
        if n_sel2 != self.n_colour:
            raise ValueError(f"{NAME_COLOUR} flags {self.n_colour} tiles, its second tables "
                             f"hold {n_sel2} rows")
        if self.n_colour and self.C < COLOUR_MIN_C:
            raise ValueError(f"{NAME_COLOUR} of C {self.C} flags colour tiles")

    def to_bytes(self) -> bytes:
        self.check()
        _check_kept(self.n_kept, self.stream)
        inner = self.stream.to_bytes() if self.n_kept else b""
        maps = pack_bitmap(self.escaped) + pack_bitmap(self.packed, over=self.escaped)
        second = b""
        if self.colour is not None:
            maps += pack_bitmap(self.colour, over=self.packed)
            second = (struct.pack("<I", self.n_colour)
                      + np.asarray(self.sel2 if self.n_colour else [], dtype="<u4").tobytes())
        sect = (pack_tables(self.n_packed, self.sel, self.states, self.nwords) + second
                + pack_words(self.words))
        flags = self.predict_ways if self.predict_ways > 1 else 0
        return (self.layout.pack(self.magic, flags) + maps + pack_lengthed(self.raw)
                + pack_lengthed(sect) + pack_lengthed(inner))

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "PredictiveTiledBitstream":
        """An IDFP or an IDFQ file, told apart by the magic."""
        two = bytes(buf[:4]) == MAGIC_COLOUR
        name = NAME_COLOUR if two else NAME
        lay, o = TileLayout.unpack(buf, MAGIC_COLOUR if two else MAGIC, name,
                                   flags_ok=(0,) + PREDICT_WAYS[1:])
        W = struct.unpack_from("<H", buf, 6)[0] or 1    # the header's flags: predict_ways > 1
        r = Reader(buf, name, o)
        escaped = r.bitmap(lay.n_tiles, "escape", "tiles")
        packed = r.sub_bitmap(escaped, "packed", "escaped tiles", then=0 if two else 8)
        colour = None
        if two:
            colour = r.sub_bitmap(packed, "colour", "packed tiles", then=8)
            if colour.any() and lay.C < COLOUR_MIN_C:
                raise ValueError(f"{name} of C {lay.C} flags colour tiles")
        _, want = raw_offsets(escaped & ~packed, lay.rects, lay.C)
        raw = torch.from_numpy(r.lengthed(want, "raw bytes", "raw tiles", then=8).copy())
        n_sect = r.u64()
        s = r.section(n_sect, "packed section", then=8)
        sel, states, nwords, n_tab = read_tables(s, n_sect, int(packed.sum()), W, "tiles")
        sel2 = None
        if two:
            if n_sect < n_tab + 4:
                raise ValueError(f"{name} holds a packed section of {n_sect} bytes, too short "
                                 "for the count of its second tables")
            Q = s.u32()
            if Q != int(colour.sum()):
                raise ValueError(f"{name} names {Q} colour tiles, its bitmap "
                                 f"{int(colour.sum())}")
            if n_sect < n_tab + 4 + 4 * Q:
                raise ValueError(f"{name} holds a packed section of {n_sect} bytes, too short "
                                 f"for the second tables of {Q} tiles")
            sel2 = s.array("<u4", Q).astype(np.uint32)
            n_tab += 4 + 4 * Q
        words = read_section_words(s, n_sect, n_tab, nwords, W)
        stream = _read_inner(r, lay.n_tiles - int(escaped.sum()), device)
        if device:
            raw, words = raw.to(device), words.to(device)
        return cls(stream, list(lay.sizes), lay.C, lay.tile_hw, escaped, packed, raw, sel,
                   states, nwords, words, colour=colour, sel2=sel2, predict_ways=W)


# ------------------------------------------------------------------ codec
class PredictiveTileCodec(SafeTiledCodec):
    """SafeTiledCodec whose escaped tiles are coded by the predictor where that is smaller
    (the module's doc has the rule) <-> PredictiveTiledBitstream.  decode and decode_region are
    TiledCodec's; their info['packed_tiles'] of the info['tiles'] tiles were decoded by
    idf_predict_decode_u8 (info['colour_tiles'] of them as colour entries, by
    idf_predict_decode2_u8), info['raw_tiles'] copied, and where all are either no flow runs.
    A codec reads IDFP and IDFQ streams alike; `colour` says which one encode writes."""

    def __init__(self, model, max_batch: int = 256, ways: int = 1, colour: bool = False,
                 predict_ways: int = 1):
        """colour: code every escaped entry both ways and keep the smaller (the module's doc has
        the colour mode); encode then returns IDFQ streams.  C >= 3.
        predict_ways: the interleaved states of every predictive stream encode writes (the
        module's doc has the wavefront order); `ways` stays the kept tiles' flow streams'.  A
        tile geometry the N-way decoder cannot hold is refused here, before any file exists."""
        super().__init__(model, max_batch=max_batch, ways=ways)
        self.colour = bool(colour)
        if self.colour and self.C < COLOUR_MIN_C:
            raise ValueError(f"the colour mode needs C >= {COLOUR_MIN_C}, the model has C "
                             f"{self.C}")
        self.predict_ways = check_predict_ways(predict_ways)
        if self.predict_ways > 1 and not ways_supported(self.C, *self.tile_hw, self.predict_ways):
            raise ValueError(f"predict_ways {self.predict_ways} does not decode tiles of C "
                             f"{self.C}, {self.tile_hw}: an entry does not fit the decoder's LDS")

    # -------------------------------------------------------------- encode
    def _planar_rows(self, rows, rects, dev):
        """-> (table rows of five fields naming the same bytes, what holds them).  The predictor
        reads each byte's causal neighbours in dense planar rectangles: rows of eight fields are
        copied entry by entry into the raw layout [C][hin][win] and the copies named."""
        if not rows or len(rows[0]) != 8:
            return rows, None
        C, (th, tw) = self.C, self.tile_hw
        offs = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(entry_bytes(rects, C), out=offs[1:])
        staging = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        device_gather_raw(self._device_table(rows, dev), len(rows), C, th, tw,
                          _to_device(torch.from_numpy(offs[:-1].copy()), dev), staging)
        base = staging.data_ptr()
        return [(base + int(o), h, w, 0, 0) for o, (h, w) in zip(offs, rects)], staging

    def _predict_coded(self, rows, rects, dev):
        """The predictive streams of the tiles rows names, at most SYMBOLS_PER_PASS symbols a
        pass (an entry's stream depends on its own bytes only): device_predict_encode's values
        (colour: device_predict_encode2's with best=True -- two streams an entry, both counted,
        and the words of the chosen, packed streams alone), the passes joined."""
        C, (th, tw) = self.C, self.tile_hw
        counts = entry_bytes(rects, C)
        rows, _staging = self._planar_rows(rows, rects, dev)  # held to the end of the passes
        per = 2 if self.colour else 1
        kw = {"best": True} if self.colour else {}
        kw["ways"] = self.predict_ways
        code = device_predict_encode2 if self.colour else device_predict_encode
        parts = [code(self._device_table(rows[k:k + m], dev), counts[k:k + m], C, th, tw, **kw)
                 for k, m in passes(per * counts)]
        sel, states, nw, status = (np.concatenate([p[i] for p in parts]) for i in range(4))
        return sel, states, nw, status, torch.cat([p[4] for p in parts])

    @torch.no_grad()
    def encode(self, images, max_ratio: float = 1.0, check: str = "status", layout=None,
               choose: str = "escaped", shortlist: bool = True) -> PredictiveTiledBitstream:
        """images, max_ratio, check, layout: as SafeTiledCodec.encode.  Sources that are not dense
        planar are copied entry by entry into the raw layout first
        (idf_tile_gather_raw_strided_u8): an entry's model reads nothing outside its rectangle,
        so the streams are those of the planar copy.

        choose="escaped": SafeTiledCodec's decision and inner stream; the escaped tiles are then
        coded by the predictor where that is smaller than their bytes.

        choose="smallest": every tile in the smallest of its three codings.  An entry is
        *flow-eligible* iff SafeTiledCodec would keep it (no failed status, flow_bits <= max_ratio
        * 8 * raw, and with check="decode" its streams decode to the source).  idf_predict_cost_u8
        prices the predictor on every entry without coding it (estimate_bytes); the predictor
        then codes every entry that is not eligible and, of the eligible ones, those whose
        estimate is below the flow's cost (shortlist=False: all of them).  The choice is made on
        the actual numbers alone (final_choice): flow_bits if eligible, 8 * (overhead + 4 *
        nwords) if coded with status 0 and below the entry's bytes, 8 * raw; the smallest wins, a
        tie goes to the flow, then to raw.  An eligible entry that leaves the flow carries
        REASON_SMALLER.  The estimate decides only what is coded: no byte of the file and no
        bound rests on it.  The flow is never chosen above raw, so max_ratio matters only below
        1 and file_size_bound_packed holds for every max_ratio.  The file is an ordinary IDFP /
        IDFQ file, never larger than choose="escaped" writes (up to the bitmaps' bytes).

        The returned stream reports, per entry, flow_bits, est_bytes (-1 with choose="escaped"),
        pred_bytes (-1 where the predictor did not code it) and the choice (CHOICE_*)."""
        if choose not in ("escaped", "smallest"):
            raise ValueError(f"choose {choose!r} is not 'escaped' or 'smallest'")
        C, (th, tw), W = self.C, self.tile_hw, self.predict_ways
        priced = {}

        def price(rows, lay, dev):
            # queued behind the flow's work and read behind its status: no host wait of its own
            priced["rows"], priced["staging"] = self._planar_rows(rows, lay.rects, dev)
            priced["cost"] = device_predict_cost(self._device_table(priced["rows"], dev),
                                                 lay.n_tiles, C, th, tw, self.colour)

        d = self._decide(images, max_ratio, check, layout,
                         price if choose == "smallest" else None)
        dev, rects, N = d.dev, d.layout.rects, d.layout.n_tiles
        reasons, eligible = d.reasons.copy(), d.reasons == 0
        counts = entry_bytes(rects, C)
        est = np.full(N, -1, dtype=np.int64)
        if choose == "smallest":
            est = estimate_bytes(priced["cost"].cpu().numpy(), W, self.colour)
        idx = np.flatnonzero(predictor_codes(eligible, d.flow_bits, est, choose, bool(shortlist)))
        pred_bytes = np.full(N, -1, dtype=np.int64)
        pred_ok = np.zeros(N, dtype=bool)
        col = np.zeros(len(idx), dtype=bool)
        have = np.ones(len(idx), dtype=bool)
        sel = np.zeros(0, dtype=np.uint32)
        sel2 = np.zeros(0, dtype=np.uint32) if self.colour else None
        states = np.zeros(0, dtype=np.uint64)
        nwords = np.zeros(0, dtype=np.int64)
        words = torch.zeros(0, dtype=torch.int32, device=dev)
        if len(idx):
            rows = priced.get("rows", d.rows)
            sel, st_all, nw_all, status, words = self._predict_coded(
                [rows[e] for e in idx], [rects[e] for e in idx], dev)
            # what the model guarantees (every byte inside the window, every frequency >= 1)
            assert not status.any(), f"predictive encode status {status[status != 0][:8]}"
            if self.colour:
                # stream 2k: entry k's plain candidate, 2k + 1 its colour candidate; `words`
                # holds the chosen streams that are below their bytes (the same rule, in the pass)
                col, pick, have = choose_streams(nw_all, status, counts[idx], W)
                sel, sel2 = np.where(col, sel[:, 1], sel[:, 0]), sel[:, 2]
                states, nwords, status = st_all[pick], nw_all[pick], status[pick]
            else:
                states, nwords = st_all, nw_all
            pred_ok[idx] = status == 0
            pred_bytes[idx] = (np.where(col, entry_overhead(W, True), entry_overhead(W))
                               + 4 * nwords)
        choice = final_choice(eligible, d.flow_bits, counts, pred_ok, pred_bytes, choose)
        escaped, packed = choice != CHOICE_FLOW, choice == CHOICE_PREDICT
        reasons[eligible & escaped] |= REASON_SMALLER
        use = packed[idx]
        words = _pick_words(words, nwords, have, use, dev)
        colour = None
        if self.colour:
            colour = np.zeros(N, dtype=bool)
            colour[idx[use & col]] = True
            sel2 = sel2[use & col]
        sel, states, nwords = sel[use], states[use], nwords[use]
        inner, raw = self._assemble(d, escaped, escaped & ~packed)
        if W > 1:
            states = np.asarray(states, dtype=np.uint64).reshape(-1, W)
        return PredictiveTiledBitstream(inner, d.sizes, C, (th, tw), escaped, packed, raw, sel,
                                        states, nwords, words, reasons, colour, sel2, W,
                                        d.flow_bits, est, pred_bytes)

    # -------------------------------------------------------------- decode
    def check_bitstream(self, pbs: PredictiveTiledBitstream):
        if (pbs.C, tuple(pbs.tile_hw)) != (self.C, self.tile_hw):
            raise ValueError(f"{NAME} of C {pbs.C}, tiles {tuple(pbs.tile_hw)} does not match "
                             f"the model's C {self.C}, input {self.tile_hw}")
        pbs.check()
        _check_kept(pbs.n_kept, pbs.stream, one_per_entry=True)

    def _decode_entries(self, pbs: PredictiveTiledBitstream, entries, rows, verify: bool,
                        seal=None):
        """Entries `entries` of pbs into the buffers rows[k] names: the kept and the raw ones as
        SafeTiledCodec does, the packed ones through idf_predict_decode_u8 and the same byte
        scatter.  seal: a sealed file's check (idfcodec.integrity): the kept and the raw entries
        are summed as SafeTiledCodec has it, the packed ones over their runs of the dense buffer,
        after the decode that leaves the source bytes there."""
        dev = self._device()
        C, (th, tw) = self.C, self.tile_hw
        p_ent = [k for k, e in enumerate(entries) if pbs.packed[e]]
        rest = [k for k, e in enumerate(entries) if not pbs.packed[e]]
        # the kept and raw entries: a safe bitstream over the same layout whose escaped entries
        # are the raw ones (the packed ones are not asked of it)
        view = SafeTiledBitstream(pbs.stream, pbs.sizes, pbs.C, pbs.tile_hw,
                                  np.asarray(pbs.escaped, dtype=bool), pbs.raw)
        view_offs = raw_offsets(pbs.stored_raw, pbs.rects(), C)[0]
        if seal is not None:
            seal.within(rest)
        info = SafeTiledCodec._decode_entries(self, view, [entries[k] for k in rest],
                                              [rows[k] for k in rest], verify, seal=seal,
                                              raw_offs=view_offs)
        info["tiles"] = len(entries)
        info["packed_tiles"] = len(p_ent)
        col = (np.zeros(len(p_ent), dtype=bool) if pbs.colour is None else
               np.asarray(pbs.colour, dtype=bool)[[entries[k] for k in p_ent]])
        info["colour_tiles"] = int(col.sum())
        if not p_ent:
            return info
        rects = pbs.rects()
        pidx = packed_index(pbs.escaped, pbs.packed)
        which = [pidx[entries[k]] for k in p_ent]
        w_off = np.zeros(len(pbs.nwords) + 1, dtype=np.int64)
        np.cumsum(pbs.nwords, out=w_off[1:])
        p_rects = [rects[entries[k]] for k in p_ent]
        out_h = np.zeros(len(p_ent) + 1, dtype=np.int64)
        np.cumsum(entry_bytes(p_rects, C), out=out_h[1:])
        n = len(p_ent)
        words = pbs.words if pbs.words.device == dev else pbs.words.to(dev)
        words = words.contiguous()
        if not words.numel():  # streams of no word still name a buffer
            words = torch.zeros(1, dtype=torch.int32, device=dev)
        W = pbs.predict_ways
        out = torch.empty(max(int(out_h[-1]), 1), dtype=torch.uint8, device=dev)
        # a seal's segment table (address, bytes per packed entry) rides in the same copy
        runs = (np.zeros(0, dtype=np.int64) if seal is None else
                seal.packed_rows(p_ent, out.data_ptr(), out_h[:n]))
        host = torch.from_numpy(np.concatenate([
            w_off[which], np.asarray(pbs.nwords, dtype=np.int64)[which], out_h[:n], runs,
            np.ascontiguousarray(np.asarray(pbs.states, dtype=np.uint64)[which])
            .view(np.int64).reshape(-1)]))
        d64 = _to_device(host, dev)
        d_runs = d64[3 * n:3 * n + len(runs)]
        d_states = d64[3 * n + len(runs):]  # [n] or [n, W]: entry-major, way-minor
        d64 = d64[:3 * n].view(3, n)
        d_sel = _to_device(torch.from_numpy(
            np.asarray(pbs.sel, dtype=np.uint32)[which].view(np.int32).copy()), dev)
        d_rect = _to_device(torch.tensor(p_rects, dtype=torch.int32).reshape(-1, 2), dev)
        final = torch.empty(n * W, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        d_sel2 = d_col = None
        if col.any():
            # sel2 of the colour entries asked for, at their slots; the rest is not read
            cidx = np.cumsum(np.asarray(pbs.colour, dtype=bool)) - 1
            s2 = np.zeros(n, dtype=np.uint32)
            s2[col] = np.asarray(pbs.sel2, dtype=np.uint32)[
                cidx[[entries[k] for k, c in zip(p_ent, col) if c]]]
            d_sel2 = _to_device(torch.from_numpy(s2.view(np.int32)), dev)
            d_col = _to_device(torch.from_numpy(col.astype(np.uint8)), dev)
        if W > 1:      # the file's own N: plain and colour entries in one launch
            device_predict_decode_ways(n, W, C, th, tw, words, d64[0], d64[1], d_states, d_sel,
                                       d_sel2, d_col, int(col.sum()), d_rect, d64[2], out, final,
                                       status)
        elif col.any():
            device_predict_decode2(n, C, th, tw, words, d64[0], d64[1], d_states, d_sel, d_sel2,
                                   d_col, int(col.sum()), d_rect, d64[2], out, final, status)
        else:
            device_predict_decode(n, C, th, tw, words, d64[0], d64[1], d_states, d_sel, d_rect,
                                  d64[2], out, final, status)
        device_scatter_raw(self._device_table([rows[k] for k in p_ent], dev), n, C, th, tw, out,
                           d64[2], d_rect)
        if seal is not None:
            seal.packed_runs(d_runs)
        info["packed_final_states"], info["packed_status"] = final, status
        if verify:
            info["ok"] = (bool(info["ok"]) and bool((final == RANS_L).all().item())
                          and not bool(status.any().item()))
        return info


__all__ = ["MAGIC", "MAGIC_COLOUR", "NAME", "ENTRY_BYTES", "ENTRY_BYTES_COLOUR", "CHOICE_FLOW",
           "CHOICE_PREDICT", "CHOICE_RAW", "COST_ONE", "COST_WORD", "REASON_SMALLER",
           "device_predict_cost", "estimate_bytes", "final_choice", "log2_q8", "predictor_codes",
           "PredictiveTiledBitstream", "PredictiveTileCodec", "choose_streams",
           "device_predict_decode",
           "device_predict_decode2", "device_predict_decode_ways", "device_predict_encode",
           "device_predict_encode2", "device_predict_prep", "device_predict_prep2", "entry_bytes",
           "entry_overhead", "file_size_bound_packed", "is_colour", "is_packed", "order",
           "pack_tables", "packed_index", "passes", "read_count", "read_section_words",
           "read_tables", "tables", "ways_supported", "PREDICT_WAYS", "check_predict_ways"]
