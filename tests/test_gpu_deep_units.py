"""csrc/deep_kernels.hip unit by unit: idf_deep_prep_u16, idf_deep_decode_u16 and the two strided
raw copies called directly over tests/deep_cases.py's units -- the 306 small ones and the
mechanics set, whose coverage tests/test_deep_cases_host.py asserts -- against tests/deep_ref.py
(numpy and the C oracle).  Everything is integer-exact or exact in f32, so every comparison is
equality.  Each test is one or two launches over all its units.

The direct decode gives every unit the packed class, whatever a file would choose: that is what
decodes the units a file stores raw, where the scale nibbles 14 and 15 fill every bucket."""
import ctypes

import numpy as np
import pytest
import torch

import deep_ref as R
from deep_cases import (SHIFT_MAX, damage_units, damaged, low_slot, mechanics_units, small_units)

pytestmark = pytest.mark.gpu

GUARD = 0xA5C3          # uint16, around and between the runs a kernel writes
GUARD_RUN = 64          # samples of it between two runs
SENTINEL = 0x5EA1BEEF   # uint32, in the words prep must leave alone


def device():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint16)
    return torch.from_numpy(a.view(np.int16)).to(device()).view(torch.uint16)


def to_np(t):
    return t.view(torch.int16).contiguous().cpu().numpy().view(np.uint16)


def dev_of(a, dtype):
    """a numpy array of any integer type as a device tensor of the signed type of its width"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype)).to(device())


@pytest.fixture(scope="module")
def cases(oracle):
    """[(name, unit, class, model, state, words)]: the small set and the mechanics set, every unit
    coded by deep_ref whatever its class."""
    units = [(f"small {i}", u) for i, u in enumerate(small_units())] + mechanics_units()
    out = []
    for name, u in units:
        m, state, words = R.encode(u)
        k = R.CONSTANT if m["min"] == m["max"] else \
            R.PACKED if R.packed_bytes(u.size, m["shift"], len(words), len(m["esc"])) < 2 * u.size \
            else R.RAW
        out.append((name, u, k, m, state, words))
    return out


# ------------------------------------------------------------------ memory layouts
def lay_out(shapes, fill):
    """Unit i of shape shapes[i] in device memory, a third each: a dense tensor of its own; a
    window of a larger canvas with a row pitch of w + 5 samples behind an odd sample offset (its
    address is 2-aligned and not 4-aligned); plane 1 of an interleaved buffer with a pixel stride
    of 3 samples.  fill(i) is the unit's samples, or None: the window then holds GUARD like the
    rest of its buffer.  -> (views: uint16 [1, h, w] each, buffers, windows: windows[i](host
    copy of buffer i) is unit i's window in it)."""
    views, bufs, windows = [], [], []
    for i, (h, w) in enumerate(shapes):
        if i % 3 == 0:
            host = np.full((h, w), GUARD, dtype=np.uint16)
            window = lambda a: a                                          # noqa: E731
        elif i % 3 == 1:
            pitch, off = w + 5, 3
            host = np.full(off + h * pitch + 2, GUARD, dtype=np.uint16)
            window = lambda a, h=h, w=w, pitch=pitch, off=off: \
                a[off:off + h * pitch].reshape(h, pitch)[:, :w]           # noqa: E731
        else:
            host = np.full((h, w, 3), GUARD, dtype=np.uint16)
            window = lambda a: a[:, :, 1]                                 # noqa: E731
        u = fill(i)
        if u is not None:
            window(host)[...] = u
        buf = to_dev(host)
        if i % 3 == 1:
            view = buf[off:off + h * pitch].view(h, pitch)[:, :w][None]
            assert view.data_ptr() % 4 == 2
        else:
            view = window(buf)[None]
        assert tuple(view.shape) == (1, h, w)
        views.append(view)
        bufs.append(buf)
        windows.append(window)
    return views, bufs, windows


def rows_of(views, origins=None):
    """deep.unit_rows of one unit a view, the tile's origin at (0, 0) or at origins[i]"""
    from idfcodec import deep
    origins = origins or [(0, 0)] * len(views)
    rows = [(i, v.shape[1], v.shape[2], y, x) for i, (v, (y, x)) in enumerate(zip(views, origins))]
    return deep.unit_rows(rows, views, 1)


# ------------------------------------------------------------------ prep, direct
def prep_direct(rows, counts, th, tw):
    """deep.device_deep_prep with its allocation restated so that low and esc start as SENTINEL
    -> its tables and results as numpy: off, low_h, x, mean, scale (uint32 bit patterns), low, esc
    (uint32), minmax, shift, sel, nesc."""
    from idfcodec import _lib, deep
    dev = device()
    n = len(rows)
    counts = np.asarray(counts, dtype=np.int64)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    low_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deep.low_words(counts, SHIFT_MAX), out=low_h[1:])
    nsym = int(off_h[-1])
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    table, off, low_off = (dev_of(a, np.int64) for a in (rows.reshape(-1), off_h, low_h[:n]))
    x, mean, scale = (torch.zeros(nsym, dtype=torch.float32, device=dev) for _ in range(3))
    low = dev_of(np.full(int(low_h[-1]), SENTINEL, dtype=np.uint32), np.int32)
    esc = dev_of(np.full(nsym, SENTINEL, dtype=np.uint32), np.int32)
    minmax = torch.zeros((n, 2), dtype=torch.int16, device=dev)
    shift = torch.zeros(n, dtype=torch.uint8, device=dev)
    sel = torch.zeros(n, dtype=torch.int32, device=dev)
    nesc = torch.zeros(n, dtype=torch.int64, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().idf_deep_prep_u16(
        _lib.stream_ptr(dev), n, th, tw, p(table), rows.ctypes.data_as(ctypes.c_void_p), p(off),
        p(low_off), p(off), p(x), p(mean), p(scale), p(low), p(esc), p(minmax), p(shift), p(sel),
        p(nesc)), "deep prep")
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)                       # noqa: E731
    return {"off": off_h, "low_h": low_h, "x": u32(x), "mean": u32(mean), "scale": u32(scale),
            "low": u32(low), "esc": u32(esc), "minmax": minmax.cpu().numpy().view(np.uint16),
            "shift": shift.cpu().numpy(), "sel": u32(sel), "nesc": nesc.cpu().numpy()}


def test_prep_equals_the_reference_field_for_field_and_writes_nothing_else(cases):
    units = [c[1] for c in cases]
    views, _, _ = lay_out([u.shape for u in units], lambda i: units[i])
    th, tw = max(u.shape[0] for u in units), max(u.shape[1] for u in units)
    p = prep_direct(rows_of(views), [u.size for u in units], th, tw)
    for t, (name, u, _, m, _, _) in enumerate(cases):
        n, s = u.size, m["shift"]
        assert int(p["shift"][t]) == s, name
        assert int(p["sel"][t]) == m["sel"], name
        assert tuple(p["minmax"][t]) == (m["min"], m["max"]), name
        ne, nl = len(m["esc"]), (n * s + 31) // 32
        assert int(p["nesc"][t]) == ne, name
        o = int(p["off"][t])
        esc = p["esc"][o:o + n]
        assert np.array_equal(esc[:ne], m["esc"]), name              # raster order
        assert (esc[ne:] == SENTINEL).all(), name
        low = p["low"][p["low_h"][t]:p["low_h"][t + 1]]
        assert len(low) == (n * SHIFT_MAX + 31) // 32 and len(m["low"]) == nl
        assert np.array_equal(low[:nl], m["low"]), name
        assert (low[nl:] == SENTINEL).all(), name
        for k in ("x", "mean", "scale"):                              # bit-equal, stream order
            assert np.array_equal(p[k][o:o + n], m[k].view(np.uint32)), (name, k)
    for u, view in zip(units, views):                                 # the sources are read only
        assert np.array_equal(to_np(view[0]), u)


# ------------------------------------------------------------------ decode, direct
def decode_direct(entries, th, tw, zero_runs=False):
    """One idf_deep_decode_u16 over entries, each a dict of h, w and -- a packed one -- shift, sel,
    state, words, low (a low_slot), esc; "cls" names another class (default packed) and "value" a
    constant's.  The tables as DeepTiledCodec._decode_units builds them: every pointer names a
    buffer, rect = (h, w), the escapes are u32, every unit has a low run sized for SHIFT_MAX, and
    GUARD_RUN samples of GUARD lie before, between and behind the out runs, which start as GUARD
    (zero_runs: as zeros, deep_ref.decode's start).
    -> (the runs as uint16 [h, w], final states, statuses, the whole out buffer, out offsets)."""
    from idfcodec import _lib
    dev = device()
    n = len(entries)
    zero = np.zeros(0, dtype=np.uint32)
    words = [np.asarray(e.get("words", zero), dtype=np.uint32) for e in entries]
    lows = [np.asarray(e["low"], dtype=np.uint32) if "low" in e
            else low_slot(zero, e["h"] * e["w"]) for e in entries]
    escs = [np.asarray(e.get("esc", zero)).astype(np.uint32) for e in entries]
    for e, lo in zip(entries, lows):
        assert len(lo) == (e["h"] * e["w"] * SHIFT_MAX + 31) // 32

    def run(parts):
        o = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=o[1:])
        return o[:-1].copy(), np.concatenate(parts + [np.zeros(1, np.uint32)])  # never empty

    word_off, d_words = run(words)
    low_off, d_low = run(lows)
    esc_off, d_esc = run(escs)
    ns = np.array([e["h"] * e["w"] for e in entries], dtype=np.int64)
    out_off = GUARD_RUN + np.concatenate([[0], np.cumsum(ns + GUARD_RUN)[:-1]])
    out_h = np.full(int(out_off[-1] + ns[-1]) + GUARD_RUN, GUARD, dtype=np.uint16)
    if zero_runs:
        for o, k in zip(out_off, ns):
            out_h[o:o + k] = 0
    t64 = np.array([word_off, [len(w) for w in words], low_off, esc_off, [len(x) for x in escs],
                    out_off, [e.get("state", R.L) for e in entries]], dtype=np.uint64)
    d64 = dev_of(t64.reshape(-1), np.int64).view(7, n)
    cls = dev_of(np.array([e.get("cls", R.PACKED) for e in entries], dtype=np.uint8), np.uint8)
    value = dev_of(np.array([e.get("value", 0) for e in entries], dtype=np.uint16), np.int16)
    shift = dev_of(np.array([e.get("shift", 0) for e in entries], dtype=np.uint8), np.uint8)
    sel = dev_of(np.array([e.get("sel", 0) for e in entries], dtype=np.uint32), np.int32)
    rect = dev_of(np.array([(e["h"], e["w"]) for e in entries], dtype=np.int32), np.int32)
    d_words, d_low, d_esc = (dev_of(a, np.int32) for a in (d_words, d_low, d_esc))
    out = dev_of(out_h, np.int16)
    final = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().idf_deep_decode_u16(
        _lib.stream_ptr(dev), n, th, tw, p(cls), p(value), p(shift), p(sel), p(d64[6]),
        p(d_words), p(d64[0]), p(d64[1]), p(d_low), p(d64[2]), p(d_esc), p(d64[3]), p(d64[4]),
        p(rect), p(d64[5]), p(out), p(final), p(status)), "deep decode")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    runs = [got[o:o + k].reshape(e["h"], e["w"]) for o, k, e in zip(out_off, ns, entries)]
    return runs, final.cpu().numpy().view(np.uint64), status.cpu().numpy(), got, out_off


def guards_intact(got, out_off, ns):
    """every sample of the out buffer outside the runs is still GUARD"""
    outside = np.ones(len(got), dtype=bool)
    for o, k in zip(out_off, ns):
        outside[o:o + k] = False
    return bool((got[outside] == GUARD).all())


def packed_entry(u, m, state, words):
    return {"h": u.shape[0], "w": u.shape[1], "shift": m["shift"], "sel": m["sel"],
            "state": int(state), "words": words, "low": low_slot(m["low"], u.size),
            "esc": m["esc"]}


def test_decode_returns_every_unit_whatever_a_file_would_choose(cases):
    entries = [packed_entry(u, m, state, words) for _, u, _, m, state, words in cases]
    # and, in the same launch, a constant unit and one of the raw class
    entries.insert(5, {"h": 7, "w": 19, "cls": R.CONSTANT, "value": 0xBEEF})
    entries.insert(9, {"h": 9, "w": 15, "cls": R.RAW})
    want = [c[1] for c in cases]
    want.insert(5, np.full((7, 19), 0xBEEF, dtype=np.uint16))
    want.insert(9, np.full((9, 15), GUARD, dtype=np.uint16))    # left to the caller's copy
    th, tw = max(e["h"] for e in entries), max(e["w"] for e in entries)
    runs, final, status, got, out_off = decode_direct(entries, th, tw)
    names = [c[0] for c in cases]
    names.insert(5, "constant")
    names.insert(9, "raw")
    for name, run, u, f, st in zip(names, runs, want, final, status):
        assert (int(f), int(st)) == (R.L, 0), name
        assert np.array_equal(run, u), name
    assert guards_intact(got, out_off, [u.size for u in want])
    # the classes a file never decodes were among them
    assert sum(c[2] == R.RAW for c in cases) > 3 and sum(c[2] == R.CONSTANT for c in cases) > 1


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("group", ["widest", "mechanics", "small"])
def test_files_equal_the_reference_and_round_trip(cases, group):
    """One image a unit, at a tile that covers the largest unit of the group: the class decision,
    the gathers, the compaction and the scatter on top of what the direct calls showed."""
    from idfcodec import DeepTiledBitstream, DeepTiledCodec, deep
    wide = deep.tw_max()
    if group == "widest":
        units, tile = [c[1] for c in cases if c[1].shape[1] == wide], (2, wide)
    elif group == "mechanics":
        units = [c[1] for c in cases if not c[0].startswith("small") and c[1].shape[1] != wide]
        tile = (max(u.shape[0] for u in units), max(u.shape[1] for u in units))
    else:
        units, tile = [c[1] for c in cases if c[0].startswith("small")], (16, 16)
    assert len(units) >= 2 and all(u.shape[0] <= tile[0] and u.shape[1] <= tile[1] for u in units)
    images = [u[None] for u in units]
    want = R.write_file(images, *tile)
    codec = DeepTiledCodec(1, tile=tile)
    buf = codec.encode([to_dev(i) for i in images]).to_bytes()
    assert buf == want
    outs, info = codec.decode(DeepTiledBitstream.from_bytes(buf, "cuda"))
    assert info["ok"] and info["damaged_planes"] == []
    for o, i in zip(outs, images):
        assert np.array_equal(to_np(o), i)


# ------------------------------------------------------------------ damage parity
def test_damaged_units_decode_as_the_reference_does(oracle):
    """Every change of deep_cases.damaged to every unit of damage_units, one launch: the whole
    run (it starts as zeros, as deep_ref.decode's does), the final state and the status equal
    deep_ref.decode's, unit for unit -- the clamps included (a high part past the window, a slot
    below the window, a sample outside 0..65535, a shift of 9) -- and no guard is touched."""
    entries, wants, names = [], [], []
    for i, u in enumerate(damage_units()):
        for change, d in damaged(u, *R.encode(u), R.buckets):
            entries.append({"h": u.shape[0], "w": u.shape[1], **d})
            wants.append(R.decode(d["shift"], d["sel"], d["state"], d["words"], d["low"],
                                  d["esc"], *u.shape))
            names.append((i, u.shape, change))
    assert len({n[2] for n in names}) == 9
    seen = 0
    runs, final, status, got, out_off = decode_direct(entries, 16, 16, zero_runs=True)
    for name, run, f, st, want in zip(names, runs, final, status, wants):
        assert (int(f), int(st)) == (want[1], want[2]), name
        assert np.array_equal(run, want[0]), name
        seen |= want[2]
    assert seen & R.UNDERFLOW and seen & R.OUT_OF_WINDOW and seen & R.WORDS_LEFT
    assert guards_intact(got, out_off, [e["h"] * e["w"] for e in entries])


# ------------------------------------------------------------------ the raw copies
def test_raw_gather_reads_every_layout(cases):
    from idfcodec import deep
    units = [c[1] for c in cases]
    views, _, _ = lay_out([u.shape for u in units], lambda i: units[i])
    th, tw = max(u.shape[0] for u in units), max(u.shape[1] for u in units)
    dev = device()
    got = to_np(deep.device_gather_raw16(rows_of(views), [u.size for u in units], th, tw, dev)
                .view(torch.uint16))
    assert np.array_equal(got, np.concatenate([u.reshape(-1) for u in units]))


def test_raw_scatter_writes_the_cropped_rectangle_and_nothing_else(cases):
    """Unit i goes into an output of its own in one of the three layouts, the output a crop whose
    origin lies (dy, dx) inside the unit -- the table row's origin is (-dy, -dx) -- and smaller
    than what is left of it on a third of the units."""
    from idfcodec import _lib
    units = [c[1] for c in cases]
    origins, shapes = [], []
    for i, u in enumerate(units):
        h, w = u.shape
        dy, dx = (i % 4) % h, (i % 5) % w
        H, W = h - dy, w - dx
        if i % 3 == 0:
            H, W = max(1, H - 2), max(1, W - 3)
        origins.append((-dy, -dx))
        shapes.append((H, W))
    assert any(y < 0 and x < 0 for y, x in origins)
    views, bufs, windows = lay_out(shapes, lambda i: None)
    rows = rows_of(views, origins)
    ns = np.array([u.size for u in units], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ns)[:-1]])
    src = to_dev(np.concatenate([u.reshape(-1) for u in units]))
    d_off, d_table = dev_of(off, np.int64), dev_of(rows.reshape(-1), np.int64)
    rect = dev_of(np.array([u.shape for u in units], dtype=np.int32), np.int32)
    th, tw = max(u.shape[0] for u in units), max(u.shape[1] for u in units)
    p = _lib.ptr
    _lib.check(_lib.lib().idf_tile_scatter_raw_strided_u16(
        _lib.stream_ptr(src.device), len(units), th, tw, p(src), p(d_off), p(rect), p(d_table),
        rows.ctypes.data_as(ctypes.c_void_p)), "deep raw scatter")
    torch.cuda.synchronize()
    for i, (u, buf, window, (y, x), (H, W)) in enumerate(zip(units, bufs, windows, origins,
                                                             shapes)):
        got = buf.view(torch.int16).cpu().numpy().view(np.uint16).copy()
        assert np.array_equal(window(got), u[-y:-y + H, -x:-x + W]), i
        window(got)[...] = GUARD
        assert (got == GUARD).all(), i
