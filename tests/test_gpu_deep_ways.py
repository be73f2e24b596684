"""The 16-bit coder's interleaved states on the device: idf_deep_prep_ways_u16 and
idf_deep_decode_ways_u16 called directly over tests/deep_ways_ref.py's units and damaged streams,
and DeepTiledCodec(ways=N) against the reference's files.  Everything is integer-exact or exact
in f32: every comparison is equality.  Each test is one or two launches over all its units."""
import ctypes

import numpy as np
import pytest
import torch

import deep_ref as R
import deep_ways_ref as W
from deep_cases import SHIFT_MAX, low_slot
from test_gpu_deep_units import (GUARD, GUARD_RUN, SENTINEL, dev_of, device, guards_intact, lay_out,
                                 rows_of, to_dev, to_np)

pytestmark = pytest.mark.gpu

TH, TW = 64, 70         # covers every unit of W.SHAPES


def units():
    """[(name, unit)]: every shape with the diagonals and the noisy ramp, two with the mixed one"""
    out = []
    for h, w in W.SHAPES:
        out += [(f"{h}x{w} diagonals", W.ramp_unit(h, w, 3, True)),
                (f"{h}x{w} noisy", W.noisy_unit(h, w))]
        if (h, w) in ((24, 70), (9, 40)):
            out.append((f"{h}x{w} mixed", W.mixed_unit(h, w)))
    return out


@pytest.fixture(scope="module")
def coded(oracle):
    """{N: [(name, unit, model, states, words)]}, coded once whatever a file would choose"""
    return {N: [(name, u, *W.encode(u, N)) for name, u in units()] for N in W.WAYS}


# ------------------------------------------------------------------ prep, direct
def prep_direct(rows, counts, th, tw, N):
    """deep.device_deep_prep at N ways with its allocation restated so that low starts as
    SENTINEL -> its tables and results as numpy."""
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
    _lib.check(_lib.lib().idf_deep_prep_ways_u16(
        _lib.stream_ptr(dev), n, th, tw, p(table), rows.ctypes.data_as(ctypes.c_void_p), p(off),
        p(low_off), p(off), p(x), p(mean), p(scale), p(low), p(esc), p(minmax), p(shift), p(sel),
        p(nesc), N), "deep prep")
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)                       # noqa: E731
    return {"off": off_h, "low_h": low_h, "x": u32(x), "mean": u32(mean), "scale": u32(scale),
            "low": u32(low), "esc": u32(esc), "minmax": minmax.cpu().numpy().view(np.uint16),
            "shift": shift.cpu().numpy(), "sel": u32(sel), "nesc": nesc.cpu().numpy()}


@pytest.mark.parametrize("N", W.WAYS)
def test_prep_writes_the_reference_symbols_and_escapes_in_wavefront_order(coded, N):
    cases = coded[N]
    us = [c[1] for c in cases]
    views, _, _ = lay_out([u.shape for u in us], lambda i: us[i])
    p = prep_direct(rows_of(views), [u.size for u in us], TH, TW, N)
    reordered = 0
    for t, (name, u, m, _, _) in enumerate(cases):
        n, s = u.size, m["shift"]
        assert int(p["shift"][t]) == s and int(p["sel"][t]) == m["sel"], name
        assert tuple(p["minmax"][t]) == (m["min"], m["max"]), name
        ne, nl = len(m["esc"]), (n * s + 31) // 32
        assert int(p["nesc"][t]) == ne, name
        o = int(p["off"][t])
        assert np.array_equal(p["esc"][o:o + ne], m["esc"]), name     # wavefront order
        reordered += not np.array_equal(m["esc"], m["esc_raster"])
        low = p["low"][p["low_h"][t]:p["low_h"][t + 1]]
        assert np.array_equal(low[:nl], m["low"]), name               # where they always were
        assert (low[nl:] == SENTINEL).all(), name
        for k in ("x", "mean", "scale"):                              # bit-equal, at n - 1 - q
            assert np.array_equal(p[k][o:o + n], m[k].view(np.uint32)), (name, k)
    assert reordered >= 3
    for u, view in zip(us, views):                                    # the sources are read only
        assert np.array_equal(to_np(view[0]), u)


# ------------------------------------------------------------------ decode, direct
def decode_direct(entries, th, tw, N):
    """One idf_deep_decode_ways_u16 over entries, each a dict of h, w and -- a packed one --
    shift, sel, states, words, low (a low_slot), esc; "cls" names another class and "value" a
    constant's.  GUARD_RUN samples of GUARD lie before, between and behind the out runs, which
    start as GUARD.  -> (the runs, final states [n, N], statuses, the out buffer, out offsets)."""
    from idfcodec import _lib
    dev = device()
    n = len(entries)
    zero = np.zeros(0, dtype=np.uint32)
    words = [np.asarray(e.get("words", zero), dtype=np.uint32) for e in entries]
    lows = [np.asarray(e["low"], dtype=np.uint32) if "low" in e
            else low_slot(zero, e["h"] * e["w"]) for e in entries]
    escs = [np.asarray(e.get("esc", zero)).astype(np.uint32) for e in entries]

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
    t64 = np.array([word_off, [len(w) for w in words], low_off, esc_off, [len(x) for x in escs],
                    out_off], dtype=np.int64)
    d64 = dev_of(t64.reshape(-1), np.int64).view(6, n)
    states = dev_of(np.array([e.get("states", [R.L] * N) for e in entries], dtype=np.uint64)
                    .reshape(-1), np.int64)
    cls = dev_of(np.array([e.get("cls", R.PACKED) for e in entries], dtype=np.uint8), np.uint8)
    value = dev_of(np.array([e.get("value", 0) for e in entries], dtype=np.uint16), np.int16)
    shift = dev_of(np.array([e.get("shift", 0) for e in entries], dtype=np.uint8), np.uint8)
    sel = dev_of(np.array([e.get("sel", 0) for e in entries], dtype=np.uint32), np.int32)
    rect = dev_of(np.array([(e["h"], e["w"]) for e in entries], dtype=np.int32), np.int32)
    d_words, d_low, d_esc = (dev_of(a, np.int32) for a in (d_words, d_low, d_esc))
    out = dev_of(out_h, np.int16)
    final = torch.zeros(n * N, dtype=torch.int64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().idf_deep_decode_ways_u16(
        _lib.stream_ptr(dev), n, N, th, tw, p(cls), p(value), p(shift), p(sel), p(states),
        p(d_words), p(d64[0]), p(d64[1]), p(d_low), p(d64[2]), p(d_esc), p(d64[3]), p(d64[4]),
        p(rect), p(d64[5]), p(out), p(final), p(status)), "deep decode")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    runs = [got[o:o + k].reshape(e["h"], e["w"]) for o, k, e in zip(out_off, ns, entries)]
    return (runs, final.cpu().numpy().view(np.uint64).reshape(n, N), status.cpu().numpy(), got,
            out_off)


def packed_entry(u, d):
    return {"h": u.shape[0], "w": u.shape[1], "shift": d["shift"], "sel": d["sel"],
            "states": [int(s) for s in d["states"]], "words": d["words"],
            "low": low_slot(d["low"], u.size), "esc": d["esc"]}


@pytest.mark.parametrize("N", W.WAYS)
def test_decode_returns_the_reference_for_sound_and_damaged_units(coded, N):
    """Every unit as it was coded, the damaged streams of five of them, a constant unit and one of
    the raw class, one launch: samples, the N final states and the status are the reference's --
    a damaged unit's by the step rule -- and no guard sample is touched."""
    entries, wants, names = [], [], []
    for name, u, m, S, words in coded[N]:
        d = {"shift": m["shift"], "sel": m["sel"], "states": S, "words": words, "low": m["low"],
             "esc": m["esc"]}
        entries.append(packed_entry(u, d))
        wants.append((u, [R.L] * N, 0))
        names.append(name)
        if name in ("40x40 diagonals", "24x70 mixed", "9x40 noisy", "19x9 noisy", "33x5 noisy"):
            for change, d in W.damaged(m, S, words):
                entries.append(packed_entry(u, d))
                wants.append(W.decode(d["shift"], d["sel"], d["states"], d["words"], d["low"],
                                      d["esc"], *u.shape, N))
                names.append(f"{name}, {change}")
    entries.insert(3, {"h": 7, "w": 19, "cls": R.CONSTANT, "value": 0xBEEF})
    wants.insert(3, (np.full((7, 19), 0xBEEF, dtype=np.uint16), [R.L] * N, 0))
    names.insert(3, "constant")
    entries.insert(8, {"h": 9, "w": 15, "cls": R.RAW})
    wants.insert(8, (np.full((9, 15), GUARD, dtype=np.uint16), [R.L] * N, 0))   # the caller's copy
    names.insert(8, "raw")
    runs, final, status, got, out_off = decode_direct(entries, TH, TW, N)
    seen = 0
    for name, run, f, st, want in zip(names, runs, final, status, wants):
        assert int(st) == want[2] and f.tolist() == want[1], name
        assert np.array_equal(run, want[0]), name
        seen |= want[2]
    assert seen == R.UNDERFLOW | R.OUT_OF_WINDOW | R.WORDS_LEFT
    assert guards_intact(got, out_off, [e["h"] * e["w"] for e in entries])


# ------------------------------------------------------------------ files
@pytest.fixture(scope="module")
def unit_files(oracle):
    """{N: (images, the reference's file)}: one grey image a unit at tile 64 x 128"""
    images = [u[None] for _, u in units()]
    return {N: (images, W.write_file(images, 64, 128, N)) for N in W.WAYS}


@pytest.mark.parametrize("N", W.WAYS)
def test_files_equal_the_reference_and_round_trip(unit_files, N):
    from idfcodec import DeepTiledBitstream, DeepTiledCodec
    images, want = unit_files[N]
    codec = DeepTiledCodec(1, tile=(64, 128), ways=N)
    buf = codec.encode([to_dev(i) for i in images]).to_bytes()
    assert buf == want
    bs = DeepTiledBitstream.from_bytes(buf, "cuda")
    assert bs.ways == N and bs.packed.any() and bs.stored_raw.any()
    outs, info = DeepTiledCodec(1, tile=(64, 128)).decode(bs)       # N is the file's
    assert info["ok"] and info["damaged_planes"] == []
    assert tuple(info["final_states"].shape) == (len(images), N)
    for o, i in zip(outs, images):
        assert np.array_equal(to_np(o), i)
    pick = [len(images) - 1, 4]
    outs, info = codec.decode(bs, images=pick)
    assert info["ok"] and info["tiles"] == 2
    for o, j in zip(outs, pick):
        assert np.array_equal(to_np(o), images[j])


def test_a_file_of_constant_packed_and_raw_units_decodes_in_one_launch(oracle):
    from test_deep_ways_host import ways_images
    from idfcodec import DeepTiledBitstream, DeepTiledCodec
    images = ways_images()
    codec = DeepTiledCodec(1, tile=(16, 16), ways=8)
    bs = codec.encode([to_dev(i) for i in images])
    assert bs.to_bytes() == W.write_file(images, 16, 16, 8)
    outs, info = codec.decode(DeepTiledBitstream.from_bytes(bs.to_bytes(), "cuda"))
    assert info["ok"]
    assert min(info["constant_planes"], info["packed_planes"], info["raw_planes"]) >= 1
    assert info["escapes"] >= 1
    for o, i in zip(outs, images):
        assert np.array_equal(to_np(o), i)
    # the same images at one way: other bytes, the same samples
    one = DeepTiledCodec(1, tile=(16, 16))
    bs1 = one.encode([to_dev(i) for i in images])
    assert bs1.ways == 1 and bs1.to_bytes() == R.write_file(images, 16, 16)
    outs1, info1 = codec.decode(bs1)                                # any codec decodes any file
    assert info1["ok"] and info1["final_states"].ndim == 1
    for a, b in zip(outs, outs1):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("N", (8, 64))
def test_strided_sources_outputs_and_regions(oracle, N):
    """A 3-channel image of 70 x 150 at tile 32 x 64: interleaved and pitched sources, outputs
    through their own strides, a region and a damaged unit among sound ones."""
    from idfcodec import DeepTiledCodec
    C, H, Wd = 3, 70, 150
    b = np.stack([W.ramp_unit(H, Wd, 3, True), W.noisy_unit(H, Wd), W.mixed_unit(H, Wd)])
    want = W.write_file([b], 32, 64, N)
    codec = DeepTiledCodec(C, tile=(32, 64), ways=N)
    assert codec.encode([to_dev(b)]).to_bytes() == want
    hwc = to_dev(np.ascontiguousarray(b.transpose(1, 2, 0)))
    assert codec.encode([hwc], layout="hwc").to_bytes() == want
    big = np.full((C, H + 4, Wd + 6), 31337, dtype=np.uint16)
    big[:, 2:2 + H, 3:3 + Wd] = b
    bs = codec.encode([to_dev(big)[:, 2:2 + H, 3:3 + Wd]], layout="chw")
    assert bs.to_bytes() == want and bs.packed.any()
    dst = to_dev(np.full((C, H + 4, Wd + 6), GUARD, dtype=np.uint16))
    outs, info = codec.decode(bs, out=[dst[:, 2:2 + H, 3:3 + Wd]])
    got = to_np(dst)
    assert info["ok"] and np.array_equal(got[:, 2:2 + H, 3:3 + Wd], b)
    got[:, 2:2 + H, 3:3 + Wd] = GUARD
    assert (got == GUARD).all()                             # nothing else was written
    dst = to_dev(np.full((H, Wd, 4), GUARD, dtype=np.uint16))
    outs, info = codec.decode(bs, layout="hwc", out=[dst[:, :, :C]])
    got = to_np(dst)
    assert info["ok"] and np.array_equal(got[:, :, :C].transpose(2, 0, 1), b)
    assert (got[:, :, C] == GUARD).all()
    out, info = codec.decode_region(bs, 0, 30, 60, 10, 9)   # four tiles of nine
    assert info["ok"] and info["tiles"] == 4 and np.array_equal(to_np(out), b[:, 30:40, 60:69])
    out, info = codec.decode_region(bs, 0, 65, 130, 5, 20, layout="hwc")    # the corner tile
    assert info["ok"] and info["tiles"] == 1
    assert np.array_equal(to_np(out), b[:, 65:70, 130:150].transpose(1, 2, 0))
    # one flipped word: its unit is damaged, every other unit exact
    bad = codec.encode([to_dev(b)])
    bad.words = bad.words.clone()
    bad.words[0] ^= 0x10000
    outs, info = codec.decode(bad)
    first = int(np.flatnonzero(bad.packed)[0])
    assert not info["ok"] and info["damaged_planes"] == [first]
    got = to_np(outs[0])
    e, p = divmod(first, C)
    ty, tx = divmod(e, 3)
    sound = np.ones_like(b, dtype=bool)
    sound[p, 32 * ty:32 * ty + 32, 64 * tx:64 * tx + 64] = False
    assert np.array_equal(got[sound], b[sound])
