"""N-way interleaved rANS streams on the device: the kernels against the format's serial
restatement (tests/rans_ways_ref.py, itself pinned to the C oracle in tests/test_ways_host.py),
word for word and state for state; the slow search paths and the stop conditions; the codec,
the container and the tiled codec with ways."""
import numpy as np
import pytest
import torch

import rans_ways_ref as R

pytestmark = pytest.mark.gpu

WAYS = (8, 16, 32, 64)
L = 1 << 32
GUARD = 0x5A5A5A5A
SLOW_SEED = 1  # slow_case(SLOW_SEED) meets test_slow_paths' conditions with the restatement alone


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt)


def _enc_ways(off, x, mean, scale, ways, tail=0):
    """idf_rans_encode_streams_ways -> (states u64 [ns * ways], the word buffer u32 (prefilled
    with GUARD, `tail` more words past the last stream), counts, status)."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    ns, nsym = off.size - 1, int(off[-1])
    fs = torch.zeros(max(ns * ways, 1), dtype=torch.int64, device="cuda")
    nw = torch.zeros(max(ns, 1), dtype=torch.int64, device="cuda")
    st = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    words = _dev(np.full(max(nsym, 1) + tail, GUARD, np.uint32).view(np.int32), torch.int32)
    wb = lib().idf_rans_encode_workspace_bytes(nsym)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    bufs = [_dev(off, torch.int64), _dev(x, torch.float32), _dev(mean, torch.float32),
            _dev(scale, torch.float32)]
    check(lib().idf_rans_encode_streams_ways(_lib.stream_ptr(), ways, ns, nsym,
                                             *[ptr(b) for b in bufs], ptr(fs), ptr(words),
                                             ptr(nw), ptr(st), ptr(ws), wb), "enc ways")
    torch.cuda.synchronize()
    return (fs.cpu().numpy().view(np.uint64)[:ns * ways], words.cpu().numpy().view(np.uint32),
            nw.cpu().numpy()[:ns], st.cpu().numpy()[:ns])


def _dec_ways(off, woff, nw, words, mean, scale, states, ways, tail=0):
    """idf_rans_decode_streams_ways -> (final states, the symbol buffer (prefilled with NaN,
    `tail` more past the last stream), status)."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    ns, nsym = off.size - 1, int(off[-1])
    fs = torch.zeros(max(ns * ways, 1), dtype=torch.int64, device="cuda")
    out = torch.full((max(nsym, 1) + tail,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    w = np.asarray(words, np.uint32)
    bufs = [_dev(off, torch.int64), _dev(woff, torch.int64), _dev(nw, torch.int64),
            _dev((w if w.size else np.zeros(1, np.uint32)).view(np.int32), torch.int32),
            _dev(mean, torch.float32), _dev(scale, torch.float32),
            _dev(np.asarray(states, np.uint64).view(np.int64), torch.int64)]
    check(lib().idf_rans_decode_streams_ways(_lib.stream_ptr(), ways, ns, nsym,
                                             *[ptr(b) for b in bufs], ptr(fs), ptr(out), ptr(st)),
          "dec ways")
    torch.cuda.synchronize()
    return fs.cpu().numpy().view(np.uint64)[:ns * ways], out.cpu().numpy(), st.cpu().numpy()[:ns]


# ------------------------------------------------------------------ the kernels
@pytest.fixture(scope="module")
def ragged():
    """37 streams (no multiple of 8, 4 or 2): every length around a step of 8 .. 64 ways, then
    random ones; test_many_ragged_streams_match_oracle's inputs.  The restatement's encode per
    ways, computed once."""
    g = np.random.default_rng(21)
    lens = np.array([0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129] + g.integers(200, 701, 26).tolist())
    assert lens.size == 37
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x, mean, scale = R.inputs(g, int(off[-1]))
    ref = {w: R.encode_streams(off, x, mean, scale, w) for w in WAYS}
    return off, x, mean, scale, ref


@pytest.mark.parametrize("ways", WAYS)
def test_encode_equals_the_restatement(ragged, ways):
    off, x, mean, scale, ref = ragged
    rfs, rwords, rnw = ref[ways]
    fs, words, nw, st = _enc_ways(off, x, mean, scale, ways, tail=64)
    assert np.array_equal(nw, rnw)
    assert np.array_equal(fs, rfs)
    assert (st == 0).all()
    for k in range(off.size - 1):
        a, e = off[k], off[k + 1]
        assert np.array_equal(words[a:a + nw[k]], rwords[a:a + nw[k]]), k
        assert (words[a + nw[k]:e] == GUARD).all(), k  # nothing written past the stream's words
    assert (words[off[-1]:] == GUARD).all()


@pytest.mark.parametrize("ways", WAYS)
def test_decode_of_the_ragged_streams(ragged, ways):
    off, x, mean, scale, ref = ragged
    rfs, rwords, rnw = ref[ways]
    # the restatement's words and states, laid out at the symbol offsets ...
    dfs, out, dst = _dec_ways(off, off[:-1], rnw, rwords, mean, scale, rfs, ways, tail=64)
    assert (dfs == L).all() and (dst == 0).all()
    assert np.array_equal(out[:off[-1]], x)
    assert np.isnan(out[off[-1]:]).all()
    # ... and the device's own, compacted
    fs, words, nw, _ = _enc_ways(off, x, mean, scale, ways)
    woff = np.concatenate([[0], np.cumsum(nw)[:-1]]).astype(np.int64)
    packed = np.concatenate([words[off[k]:off[k] + nw[k]] for k in range(nw.size)])
    dfs, out, dst = _dec_ways(off, woff, nw, packed, mean, scale, fs, ways)
    assert (dfs == L).all() and (dst == 0).all()
    assert np.array_equal(out[:off[-1]], x)


def test_one_way_through_the_ways_calls_matches_the_oracle(oracle, ragged):
    """ways = 1 in the same entry points is the one-state format."""
    off, x, mean, scale, _ = ragged
    fs, words, nw, st = _enc_ways(off, x, mean, scale, 1)
    rfs, rwords, rnw, _ = oracle.encode_streams(off, x, mean, scale)
    assert np.array_equal(fs, rfs) and np.array_equal(nw, rnw) and (st == 0).all()
    for k in range(nw.size):
        assert np.array_equal(words[off[k]:off[k] + nw[k]], rwords[off[k]:off[k] + nw[k]]), k
    dfs, out, dst = _dec_ways(off, off[:-1], nw, words[:max(int(off[-1]), 1)], mean, scale, fs, 1)
    assert (dfs == L).all() and (dst == 0).all() and np.array_equal(out[:off[-1]], x)


def test_unsupported_ways_are_argument_errors():
    from idfcodec._lib import lib
    for ways in (0, 2, 4, 12, 128, -8):
        assert lib().idf_rans_encode_streams_ways(None, ways, 0, 0, *[None] * 9, 0) == 1
        assert lib().idf_rans_decode_streams_ways(None, ways, 0, 0, *[None] * 10) == 1
    for ways in (1,) + WAYS:  # no streams: IDF_OK without a launch
        assert lib().idf_rans_encode_streams_ways(None, ways, 0, 0, *[None] * 9, 0) == 0
        assert lib().idf_rans_decode_streams_ways(None, ways, 0, 0, *[None] * 10) == 0


def slow_case(seed, n_streams=24):
    """test_decode_slow_paths_match_oracle's mix: ordinary scales with 2^-62, 2^62 and negative
    ones, random words (one per symbol) and, per ways, random states in [2^32, 2^62)."""
    g = np.random.default_rng(seed)
    lens = g.integers(1, 201, n_streams)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    mean = (g.integers(-512, 513, n) / 256).astype(np.float32)
    scale = (np.exp(6 * g.random(n) - 5)).astype(np.float32)
    kind = g.integers(0, 4, n)
    scale[kind == 1] = np.float32(2.0 ** -62)
    scale[kind == 2] = np.float32(2.0 ** 62)
    scale[kind == 3] = -np.float32(2.0 ** 40) * (1 + g.random((kind == 3).sum())).astype(np.float32)
    words = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    states = {w: g.integers(1 << 32, 1 << 62, n_streams * w, dtype=np.uint64) for w in (8, 64)}
    return off, lens.astype(np.int64), mean, scale, kind, words, states


@pytest.mark.parametrize("ways", [8, 64])
def test_slow_paths(ways):
    """Decode is a function of (states, words, mean, scale) whether or not an encoder made them:
    symbols, final states and flags equal the serial decoder's on every stream it finishes
    without a reference error."""
    off, lens, mean, scale, kind, words, states = slow_case(SLOW_SEED)
    rfs, rout, rst, ok = R.decode_streams(off, off[:-1], lens, words, mean, scale, states[ways],
                                          ways)
    assert ok.sum() >= lens.size // 2
    hit = np.zeros(mean.size, bool)
    for k in np.flatnonzero(ok):
        hit[off[k]:off[k + 1]] = True
    for kd in (1, 2, 3):  # every slow path inside a checked stream
        assert (hit & (kind == kd)).sum() > 100, kd
    dfs, out, dst = _dec_ways(off, off[:-1], lens, words, mean, scale, states[ways], ways)
    for k in np.flatnonzero(ok):
        a, e = off[k], off[k + 1]
        assert np.array_equal(dfs[k * ways:(k + 1) * ways], rfs[k * ways:(k + 1) * ways]), k
        assert np.array_equal(out[a:e], rout[a:e]), k
        assert dst[k] == rst[k], (k, dst[k], rst[k])


def test_stops_leave_the_wave_mates_exact():
    """ways 8: the 8 streams of one wave.  Decode: stream 2 meets a scale 0 in mid-stream,
    stream 5 is given too few words.  Encode: stream 3 meets a scale 0.  The flagged streams
    carry their flags, the others are exact, and nothing past a stream's ranges is written."""
    from idfcodec import _lib
    ways = 8
    g = np.random.default_rng(33)
    lens = np.array([300, 129, 260, 64, 7, 410, 65, 200], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x, mean, scale = R.inputs(g, int(off[-1]))
    rfs, rwords, rnw = R.encode_streams(off, x, mean, scale, ways)
    assert rnw[5] >= 3
    # ---- decode
    scale_d = scale.copy()
    zero_at = off[2] + 131  # symbol 131 of stream 2: step 16, way 3
    scale_d[zero_at] = 0.0
    woff, nw = off[:-1].copy(), rnw.copy()
    woff[5] += 3  # stream 5 without its first 3 words: its last 3 reads find none
    nw[5] -= 3
    dfs, out, dst = _dec_ways(off, woff, nw, rwords, mean, scale_d, rfs, ways, tail=64)
    for k in range(lens.size):
        a, e = off[k], off[k + 1]
        if k == 2:
            assert dst[k] & _lib.STREAM_SCALE_ZERO, dst[k]
            first = a + (131 // ways + 1) * ways  # the steps before the stop (decoded last first)
            assert np.array_equal(out[first:e], x[first:e])
        elif k == 5:
            assert dst[k] & _lib.STREAM_UNDERFLOW, dst[k]
        else:
            assert dst[k] == 0 and (dfs[k * ways:(k + 1) * ways] == L).all(), k
            assert np.array_equal(out[a:e], x[a:e]), k
    assert np.isnan(out[off[-1]:]).all()
    # ---- encode
    scale_e = scale.copy()
    scale_e[off[3] + 20] = 0.0
    fs, words, enw, est = _enc_ways(off, x, mean, scale_e, ways, tail=64)
    for k in range(lens.size):
        a, e = off[k], off[k + 1]
        assert 0 <= enw[k] <= e - a
        assert (words[a + enw[k]:e] == GUARD).all(), k
        if k == 3:
            assert est[k] & _lib.STREAM_SCALE_ZERO, est[k]
        else:
            assert est[k] == 0 and enw[k] == rnw[k], k
            assert np.array_equal(fs[k * ways:(k + 1) * ways], rfs[k * ways:(k + 1) * ways]), k
            assert np.array_equal(words[a:a + enw[k]], rwords[a:a + enw[k]]), k
    assert (words[off[-1]:] == GUARD).all()


# ------------------------------------------------------------------ the codec
@pytest.fixture(scope="module")
def model():
    from idfcodec import configs, synthetic
    return synthetic.build_model(configs.get("imagenet64")).cuda()


@pytest.mark.parametrize("B,ways", [(3, 8), (3, 64), (16, 8)])
def test_codec_streams_equal_the_restatement_and_round_trip(model, B, ways):
    from idfcodec import synthetic
    from idfcodec.codec import Bitstream
    codec = model.codec()
    eng = model.engine()
    img = synthetic.images(B, seed=70 + B).cuda()
    raw = codec.encode(img, compact=False, ways=ways)
    assert raw.ways == ways and raw.n_streams == eng.nsplit * B
    assert raw.states.numel() == raw.n_streams * ways
    ws = eng.workspace(B)
    lat, mean, scale = (ws[k].cpu().numpy() for k in ("lat", "mean", "scale"))
    off = codec.coder.sym_off(B).cpu().numpy()
    rfs, rwords, rnw = R.encode_streams(off, lat, mean, scale, ways)
    assert np.array_equal(raw.states.cpu().numpy().view(np.uint64), rfs)
    assert np.array_equal(raw.nwords.cpu().numpy(), rnw)
    got = raw.words.cpu().numpy().view(np.uint32)
    for k in range(rnw.size):
        assert np.array_equal(got[off[k]:off[k] + rnw[k]], rwords[off[k]:off[k] + rnw[k]]), k
    out, info = codec.decode(raw)  # the scratch-offset bitstream
    assert info["ok"] and torch.equal(out, img)
    assert info["final_states"].numel() == raw.n_streams * ways
    # the container
    bs = codec.encode(img, ways=ways)
    assert bs.bits() == 64 * rfs.size + 32 * int(rnw.sum())
    back = Bitstream.from_bytes(bs.to_bytes(), device="cuda")
    assert back.ways == ways
    out, info = codec.decode(back)
    assert info["ok"] and torch.equal(out, img)
    # an image coded alone: the same states and words as inside the batch
    alone = codec.encode(img[1:2], ways=ways)
    sel = bs.select([1])
    assert torch.equal(alone.states, sel.states) and torch.equal(alone.nwords, sel.nwords)
    assert torch.equal(alone.words, sel.words)
    out, info = codec.decode(sel)
    assert info["ok"] and torch.equal(out, img[1:2])


def test_codec_group_and_ways_combine(model):
    from idfcodec import synthetic
    codec = model.codec()
    img = synthetic.images(16, seed=86).cuda()
    bs = codec.encode(img, group=4, ways=8)
    assert bs.group == 4 and bs.ways == 8 and bs.n_streams == model.engine().nsplit * 4
    assert bs.states.numel() == bs.n_streams * 8
    out, info = codec.decode(bs)
    assert info["ok"] and torch.equal(out, img)


def test_ways_one_is_todays_bitstream(model):
    from idfcodec import synthetic
    img = synthetic.images(3, seed=73).cuda()
    a, b = model.encode(img), model.encode(img, ways=1)
    assert b.ways == 1
    assert torch.equal(a.states, b.states) and torch.equal(a.nwords, b.nwords)
    assert torch.equal(a.words, b.words) and a.to_bytes() == b.to_bytes()
    with pytest.raises(ValueError, match="ways"):
        model.encode(img, ways=4)


# ------------------------------------------------------------------ tiles
def test_tiled_with_ways():
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    from idfcodec.tiled import TiledBitstream
    model = synthetic.build_model(_flows("IDFlows", 2, 2, 16, 16, 3, _dense(24, 3), _dense(16, 2),
                                         2)).cuda()
    imgs = [synthetic.images(1, 3, 70, 33, seed=91)[0].cuda(),
            synthetic.images(1, 3, 64, 64, seed=92)[0].cuda()]
    tc = model.tiled(ways=8)
    assert tc.ways == 8
    tbs = tc.encode(imgs)
    assert tbs.stream.ways == 8 and tbs.stream.n_images == 15 + 16
    assert tbs.stream.states.numel() == tbs.stream.n_streams * 8
    raw = tbs.to_bytes()
    merged = model.tiled(max_batch=2, ways=8).encode(imgs)  # 16 chunks through _merge
    assert merged.to_bytes() == raw
    for codec in (model.tiled(max_batch=2, ways=8), model.tiled(ways=8), model.tiled()):
        back = TiledBitstream.from_bytes(raw, device="cuda")
        outs, info = codec.decode(back)
        assert info["ok"] and all(torch.equal(o, i) for o, i in zip(outs, imgs))
        crop, info = codec.decode_region(back, 0, 10, 5, 45, 25)  # rows 10..54, columns 5..29
        assert info["ok"] and info["tiles"] == 4 * 2
        assert torch.equal(crop, imgs[0][:, 10:55, 5:30])
    one = model.tiled().encode(imgs)
    assert one.stream.ways == 1
    assert tbs.state_bits_per_subpixel() == 8 * one.state_bits_per_subpixel()
