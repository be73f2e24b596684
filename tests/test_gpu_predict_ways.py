"""The predictive coder's interleaved streams on the device (predict_ways = N): the ways-taking
prep bit for bit against the numpy reference (tests/predict_ways_ref.py) inside guard values, prep
plus idf_rans_encode_streams_ways word for word against the pure-Python N-way coder,
idf_predict_decode_ways_u8 on the reference's words inside guard bytes, one damaged and one
shortened stream among intact ones, and tiled_safe(predict=..., predict_ways=N) end to end: exact
round trips, the file sizes the reference's costs predict, crops over packed, raw and kept tiles.

The rectangles are test_gpu_predict's: tiles (16,16), (12,8), (40,33) with images 1x1, a full tile,
a tile plus a 1-wide / 1-high strip, 5x5 and 2 x 2 tiles with 5-wide edges -- the smallest shapes
that reach win < N (P = N), win = 1, hin = 1, R < N, R no multiple of N, a plane border inside a
band (hin 12, N 8), lane 0 of a band reading lane N - 1 of the band before at win >= N ((40,33) at
N 8, 16, 32) and more than 64 words an entry (noise at (40,33)).  Tiny models only."""
import functools

import numpy as np
import pytest
import torch

import colour_ref as cref
import predict_ref as ref
import predict_ways_ref as wref
import rans_ways_ref
from test_gpu_predict import (FGUARD, SIZES, TILES, L, _case, _others_exact, _planes_of, _smooth,
                              _table, _victim)
from test_gpu_safe import GUARD, _dev, _guarded, _guards_intact, _noise, _tiny_model
from test_predict_host import contents

pytestmark = pytest.mark.gpu

# C in {1, 3, 4} at N in {8, 64} on all three tiles; N in {16, 32} at C = 3, (40, 33)
CASES = [(C, th, tw, N) for C in (1, 3, 4) for th, tw in TILES for N in (8, 64)] + \
        [(3, 40, 33, 16), (3, 40, 33, 32)]
IDS = [f"C{C}-{th}x{tw}-N{N}" for C, th, tw, N in CASES]


@functools.lru_cache(maxsize=None)
def _wcase(C, th, tw, N):
    """test_gpu_predict._case's images and rectangles with the reference's N-way coding of each
    entry: symbols in wavefront order, N states and the words of rans_ways_ref.  Computed once
    per (C, th, tw, N) and shared, never modified."""
    base = _case(C, th, tw)
    arrs = [wref.arrays(p, N, int(s)) for p, s in zip(base["planes"], base["sel"])]
    x, mean, scale = (np.concatenate([a[i] for a in arrs]) for i in range(3))
    fs, words, nw = rans_ways_ref.encode_streams(base["off"], x, mean, scale, N)
    w_off = np.zeros(len(nw) + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    compact = np.concatenate([words[a:a + n] for a, n in zip(base["off"][:-1], nw)])
    return dict(base, x=x, mean=mean, scale=scale, states=fs.reshape(-1, N), nw=nw,
                words=compact.astype(np.uint32), w_off=w_off)


def test_the_cases_reach_every_branch():
    rects = {(C, h, w) for C, th, tw, _ in CASES for h, w in _case(C, th, tw)["rects"]}
    assert {(3, 1, 1), (3, 16, 1), (3, 1, 16), (3, 5, 5), (3, 12, 8), (3, 40, 33)} <= rects
    assert any(w < 8 for _, _, w in rects) and any(C * h < 8 for C, h, _ in rects)
    assert any((C * h) % 8 and C * h > 8 for C, h, _ in rects)
    assert any(h % 8 and C > 1 for C, h, _ in rects)           # a plane border inside a band
    assert int(_wcase(3, 40, 33, 8)["nw"].max()) > 64          # the word-window switch


# ------------------------------------------------------------------ 1. prep and encode
@pytest.mark.parametrize("C,th,tw,N", CASES, ids=IDS)
def test_prep_equals_reference_inside_guards(C, th, tw, N):
    from idfcodec.predict import device_predict_prep
    case = _wcase(C, th, tw, N)
    src, table = _table(case, th, tw)
    n, nsym = len(case["planes"]), int(case["off"][-1])
    gap = 64
    bufs = [torch.full((nsym + 2 * gap,), FGUARD, dtype=torch.float32, device="cuda")
            for _ in range(3)]
    x, mean, scale = (b[gap:gap + nsym] for b in bufs)
    selbuf = torch.full((n + 2 * gap,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sel = selbuf[gap:gap + n]
    device_predict_prep(table, n, C, th, tw, _dev(case["off"], torch.int64), sel, x, mean, scale,
                        ways=N)
    torch.cuda.synchronize()
    assert np.array_equal(sel.cpu().numpy().view(np.uint32), case["sel"])
    for got, want in zip((x, mean, scale), (case["x"], case["mean"], case["scale"])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for b in bufs:
        assert bool((b[:gap] == FGUARD).all()) and bool((b[gap + nsym:] == FGUARD).all())
    assert bool((selbuf[:gap] == 0x5A5A5A5A).all()) and bool((selbuf[gap + n:] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("C,th,tw,N", CASES, ids=IDS)
def test_streams_equal_the_reference_word_for_word(C, th, tw, N):
    from idfcodec.predict import device_predict_encode
    case = _wcase(C, th, tw, N)
    src, table = _table(case, th, tw)
    sel, states, nw, status, words = device_predict_encode(table, case["counts"], C, th, tw, N)
    assert not status.any()
    assert np.array_equal(sel, case["sel"])
    assert np.array_equal(nw, case["nw"])
    assert states.shape == case["states"].shape and np.array_equal(states, case["states"])
    assert np.array_equal(words.cpu().numpy().view(np.uint32), case["words"])


def test_both_candidates_in_wavefront_order():
    """idf_predict_prep2_ways_u8: stream 2t the plain candidate, 2t + 1 the colour one, each the
    reference's symbols at the reference's indices; coded, the reference's states and words."""
    from idfcodec.predict import device_predict_encode2
    C, th, tw, N = 3, 12, 8, 8
    case = _wcase(C, th, tw, N)
    src, table = _table(case, th, tw)
    sel, states, nw, status, words = device_predict_encode2(table, case["counts"], C, th, tw,
                                                            ways=N)
    assert not status.any() and states.shape == (2 * len(case["planes"]), N)
    assert np.array_equal(sel[:, 0], case["sel"])
    assert np.array_equal(states[0::2], case["states"]) and np.array_equal(nw[0::2], case["nw"])
    got = words.cpu().numpy().view(np.uint32)
    o = 0
    for e, p in enumerate(case["planes"]):
        assert np.array_equal(got[o:o + nw[2 * e]],
                              case["words"][case["w_off"][e]:case["w_off"][e + 1]]), e
        o += int(nw[2 * e])
        s, s2, S, w = wref.encode(p, N, colour=True)
        assert (int(sel[e, 1]), int(sel[e, 2])) == (s, s2), e
        assert states[2 * e + 1].tolist() == S and np.array_equal(got[o:o + len(w)], w), e
        assert nw[2 * e + 1] == len(w)
        o += len(w)


# ------------------------------------------------------------------ 2. the decoder
def _decode(case, C, th, tw, N, words, w_off, nw, colour=None, sel2=None, states=None, sel=None,
            planes=None):
    """idf_predict_decode_ways_u8 over every entry of the case into guarded bytes, the entries'
    outputs handed out in reverse order with 5 unused bytes between two: -> (big, out, offsets,
    the bytes expected, final states [n, N], status)."""
    from idfcodec.predict import device_predict_decode_ways
    planes = case["planes"] if planes is None else planes
    n = len(planes)
    offs, o = [0] * n, 0
    for e in reversed(range(n)):
        offs[e] = o
        o += int(planes[e].size) + 5
    want = np.full(o, GUARD, dtype=np.uint8)
    for e, p in enumerate(planes):
        want[offs[e]:offs[e] + p.size] = p.reshape(-1)
    big, (out,) = _guarded([(o,)])
    final = torch.zeros(n * N, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st = case["states"] if states is None else states
    sl = case["sel"] if sel is None else sel
    rects = [p.shape[1:] for p in planes]
    nc = 0 if colour is None else int(np.count_nonzero(colour))
    if not words.size:  # streams of no word still name a buffer
        words = np.zeros(1, dtype=np.uint32)
    device_predict_decode_ways(
        n, N, C, th, tw, torch.from_numpy(words.view(np.int32).copy()).cuda(),
        _dev(w_off[:n], torch.int64), _dev(nw, torch.int64),
        torch.from_numpy(np.ascontiguousarray(st).view(np.int64).reshape(-1).copy()).cuda(),
        torch.from_numpy(np.asarray(sl, dtype=np.uint32).view(np.int32).copy()).cuda(),
        None if not nc else torch.from_numpy(np.asarray(sel2, np.uint32).view(np.int32).copy()).cuda(),
        None if not nc else torch.from_numpy(np.asarray(colour, dtype=np.uint8)).cuda(), nc,
        _dev(rects, torch.int32), _dev(offs, torch.int64), out, final, status)
    torch.cuda.synchronize()
    return big, out, offs, want, final.cpu().numpy().reshape(n, N), status.cpu().numpy()


@pytest.mark.parametrize("C,th,tw,N", CASES, ids=IDS)
def test_decode_returns_the_bytes_inside_guards(C, th, tw, N):
    case = _wcase(C, th, tw, N)
    big, out, offs, want, final, status = _decode(case, C, th, tw, N, case["words"],
                                                  case["w_off"], case["nw"])
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])


@pytest.mark.parametrize("N", [8, 32])
def test_plain_and_colour_entries_decode_in_one_launch(N):
    """Every other entry a colour entry, coded by the reference: its sel2 on the second table of
    planes 0 and 2, the inverse transform behind the decoder."""
    C, th, tw = 3, 12, 8
    planes = [cref.correlated(12, 8, 3), contents((3, 12, 8))["ramp"], cref.independent(5, 8, 4),
              cref.noise(12, 1, 5), cref.correlated(1, 8, 6), contents((3, 12, 8))["noise"]]
    colour = np.array([True, False, True, True, True, False])
    coded = [wref.encode(p, N, colour=bool(c)) for p, c in zip(planes, colour)]
    nw = np.array([len(c[3]) for c in coded], dtype=np.int64)
    w_off = np.zeros(len(nw) + 1, dtype=np.int64)
    np.cumsum(nw, out=w_off[1:])
    words = np.concatenate([c[3] for c in coded]).astype(np.uint32)
    states = np.array([c[2] for c in coded], dtype=np.uint64)
    sel = np.array([c[0] for c in coded], dtype=np.uint32)
    sel2 = np.array([c[1] or 0 for c in coded], dtype=np.uint32)
    big, out, offs, want, final, status = _decode(None, C, th, tw, N, words, w_off, nw, colour,
                                                  sel2, states, sel, planes)
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])


# ------------------------------------------------------------------ 3. damage
@pytest.mark.parametrize("N", [8, 64])
def test_a_flipped_word_is_reported_and_stays_in_its_entry(N):
    """A bounds check, run once: the call returns, the entry whose word was flipped is flagged (a
    status flag or a final state other than L), every other entry -- its bytes, its N final
    states, its status -- and every guard byte is exact."""
    C, th, tw = 3, 16, 16
    case = _wcase(C, th, tw, N)
    e = _victim(case)
    assert case["nw"][e] >= 8
    words = case["words"].copy()
    words[case["w_off"][e] + case["nw"][e] // 2] ^= 0x00010000
    big, out, offs, want, final, status = _decode(case, C, th, tw, N, words, case["w_off"],
                                                  case["nw"])
    assert status[e] != 0 or (final[e] != L).any()
    _others_exact(case, e, out, offs, (final == L).all(1) * L, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])   # whatever the entry holds, nothing around it moved


@pytest.mark.parametrize("N", [8, 64])
def test_a_missing_word_is_an_underflow(N):
    """A bounds check, run once.  The first word pushed is the last one read: without it the read
    finds no word -- UNDERFLOW on that entry only, whatever its bytes."""
    C, th, tw = 3, 16, 16
    case = _wcase(C, th, tw, N)
    e = _victim(case)
    nw = case["nw"].copy()
    nw[e] -= 1
    first = case["w_off"].copy()
    first[e] += 1
    big, out, offs, want, final, status = _decode(case, C, th, tw, N, case["words"], first, nw)
    assert status[e] & ref.UNDERFLOW
    _others_exact(case, e, out, offs, (final == L).all(1) * L, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])


# ------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def model_far():
    """test_gpu_predict's: the top level's prior mean moved 8.0 away, so every tile escapes."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    prior = m.blocks[-1]["prior"]
    with torch.no_grad():
        prior.NN.layers[-1].bias[:prior.out_channel] += 8.0
    return m.cuda()


@pytest.fixture(scope="module")
def model_sharp():
    """test_gpu_predict's: every prior's logscale lowered by 3.0, so dark tiles are kept."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            b["prior"].NN.layers[-1].bias[b["prior"].out_channel:] -= 3.0
    return m.cuda()


@pytest.fixture(scope="module")
def mixed():
    """test_gpu_predict's: a 32x48 image of six tiles -- dark, noise, smooth / smooth, dark, noise
    -- and three more images, one of each kind."""
    dark = lambda H, W, s: _noise(H, W, s) % 4  # noqa: E731
    top = torch.cat([dark(16, 16, 80), _noise(16, 16, 81), _smooth(16, 16, 82)], dim=2)
    bottom = torch.cat([_smooth(16, 16, 83), dark(16, 16, 84), _noise(16, 16, 85)], dim=2)
    return [t.contiguous().cuda() for t in (torch.cat([top, bottom], dim=1), dark(17, 16, 86),
                                            _smooth(37, 21, 87), _noise(5, 40, 88))]


def _ragged(i, H, W):
    return (_smooth(H, W, 50 + i) if i % 2 else _noise(H, W, 50 + i)).cuda()


@pytest.mark.parametrize("kind", ["smooth", "noise", "ragged"])
def test_round_trip_and_the_size_the_reference_predicts(model_far, kind):
    from idfcodec.predict import PredictiveTiledBitstream, file_size_bound_packed
    N = 8
    make = {"smooth": lambda i, H, W: _smooth(H, W, 40 + i).cuda(),
            "noise": lambda i, H, W: _noise(H, W, 70 + i).cuda(), "ragged": _ragged}[kind]
    imgs = [make(i, H, W) for i, (H, W) in enumerate(SIZES)]
    pc = model_far.tiled_safe(predict=True, predict_ways=N)
    assert pc.predict_ways == N and pc.ways == 1
    pbs = pc.encode(imgs)
    assert pbs.predict_ways == N and pbs.escaped.all()
    buf = pbs.to_bytes()
    got = PredictiveTiledBitstream.from_bytes(buf, device="cuda")
    assert got.predict_ways == N
    # decode follows the file's own N, whatever the codec was built with
    for codec in (pc, model_far.tiled_safe(predict=True)):
        outs, info = codec.decode(got)
        assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))
        assert info["packed_tiles"] == pbs.n_packed and info["raw_tiles"] == 13 - pbs.n_packed
    if pbs.n_packed:
        assert info["packed_final_states"].numel() == N * pbs.n_packed
    # the split and the length from the reference: an entry costs its bytes raw, or 8 + 8 N + 4 nw
    planes = _planes_of(imgs, pbs.layout)
    choice = [wref.choice(p, N) for p in planes]
    assert pbs.packed.tolist() == [k != "raw" for k, _ in choice]
    assert (pbs.n_packed > 0) == (kind != "noise")
    head = len(pbs.layout.pack(b"IDFP")) + 2          # 13 tiles: a bitmap of 2 bytes
    assert len(buf) == head + 2 + 8 + 8 + 4 + sum(c for _, c in choice) + 8
    assert len(buf) <= file_size_bound_packed(SIZES, 3, 16, 16, 2, kept=False)
    assert np.array_equal(pbs.nwords, [(c - 8 - 8 * N) // 4 for k, c in choice if k != "raw"])


def test_region_over_packed_raw_and_kept_tiles(model_sharp, mixed):
    pc = model_sharp.tiled_safe(predict=True, predict_ways=8)
    pbs = pc.encode(mixed)
    kinds = [("kept" if not e else "packed" if p else "raw")
             for e, p in zip(pbs.escaped[:6], pbs.packed[:6])]
    assert set(kinds) == {"kept", "packed", "raw"}, kinds
    outs, info = pc.decode(pbs)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, mixed))
    outs, info = pc.decode(pbs, images=[2, 0])
    assert info["ok"] and torch.equal(outs[0], mixed[2]) and torch.equal(outs[1], mixed[0])
    y0, x0, h, w = 10, 9, 15, 30            # all six tiles of image 0, each clipped
    crop, info = pc.decode_region(pbs, 0, y0, x0, h, w)
    assert info["ok"] and info["tiles"] == 6
    assert info["packed_tiles"] == kinds.count("packed") and info["raw_tiles"] == kinds.count("raw")
    assert torch.equal(crop, mixed[0][:, y0:y0 + h, x0:x0 + w])
    # a crop inside one packed tile: that tile alone is decoded, no flow runs
    e = kinds.index("packed")
    ty, tx = divmod(e, 3)
    crop, info = pc.decode_region(pbs, 0, ty * 16 + 3, tx * 16 + 2, 9, 11)
    assert info["ok"] and info["tiles"] == 1 and info["packed_tiles"] == 1
    assert info["final_states"].numel() == 0 and info["packed_final_states"].numel() == 8
    assert torch.equal(crop, mixed[0][:, ty * 16 + 3:ty * 16 + 12, tx * 16 + 2:tx * 16 + 13])


def test_bytes_depend_on_neither_max_batch_nor_the_default(model_sharp, mixed):
    from idfcodec.predict import PredictiveTileCodec
    a = PredictiveTileCodec(model_sharp, max_batch=2, predict_ways=8).encode(mixed)
    b = PredictiveTileCodec(model_sharp, max_batch=256, predict_ways=8).encode(mixed)
    assert a.to_bytes() == b.to_bytes() and a.n_packed > 0
    # the flow's ways and the predictor's are independent
    c = PredictiveTileCodec(model_sharp, ways=8, predict_ways=8).encode(mixed)
    assert c.stream.ways == 8 and c.predict_ways == 8
    # predict_ways = 1 is the default, byte for byte
    one = PredictiveTileCodec(model_sharp, predict_ways=1).encode(mixed).to_bytes()
    assert one == PredictiveTileCodec(model_sharp).encode(mixed).to_bytes()
    assert one == model_sharp.tiled_safe(predict=True).encode(mixed).to_bytes()
    assert one != b.to_bytes()


def test_colour_mode_round_trips_and_flags_what_the_reference_flags(model_far):
    from idfcodec.predict import PredictiveTiledBitstream
    N = 16
    sizes = [(16, 16), (32, 48), (21, 37)]
    imgs = [torch.from_numpy(p).cuda() for p in cref.end_to_end_input(sizes)]
    pc = model_far.tiled_safe(predict="colour", predict_ways=N)
    assert pc is model_far.tiled_safe(predict="colour", predict_ways=N)
    assert pc is not model_far.tiled_safe(predict="colour")      # the cache is keyed on N too
    pbs = pc.encode(imgs)
    buf = pbs.to_bytes()
    assert buf[:4] == b"IDFQ" and pbs.predict_ways == N
    got = PredictiveTiledBitstream.from_bytes(buf, device="cuda")
    outs, info = pc.decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))
    kinds = [wref.choice(p, N, colour=True)[0] for p in _planes_of(imgs, pbs.layout)]
    assert pbs.packed.tolist() == [k != "raw" for k in kinds]
    assert pbs.colour.tolist() == [k == "colour" for k in kinds]
    assert "colour" in kinds and info["colour_tiles"] == kinds.count("colour")


def test_verify_catches_a_damaged_packed_entry(model_far):
    imgs = [_smooth(16, 16, 60).cuda(), _smooth(37, 21, 61).cuda()]
    pc = model_far.tiled_safe(predict=True, predict_ways=8)
    pbs = pc.encode(imgs)
    assert pbs.n_packed >= 2 and int(pbs.nwords[0]) >= 4
    pbs.words = pbs.words.clone()
    pbs.words[2] ^= 0x00010000
    outs, info = pc.decode(pbs)
    assert not info["ok"]
    assert torch.equal(outs[1][:, 16:, :], imgs[1][:, 16:, :])     # other entries stay exact


# ------------------------------------------------------------------ 5. errors
def test_other_ways_are_refused(model_far):
    from idfcodec._lib import lib
    one = 8  # any non-NULL address: the calls return before it is read
    for ways in (4, 128):
        assert lib().idf_predict_prep_ways_u8(None, 1, 3, 16, 16, *[one] * 6, ways) == 1
        assert lib().idf_predict_decode_ways_u8(None, 1, 0, ways, 3, 16, 16, *[one] * 12) == 1
        with pytest.raises(ValueError, match="predict_ways"):
            model_far.tiled_safe(predict=True, predict_ways=ways)
        with pytest.raises(ValueError, match="predict_ways"):
            model_far.tiled_safe(predict="colour", predict_ways=ways)
    with pytest.raises(ValueError, match="predict_ways"):
        model_far.tiled_safe(predict_ways=8)                       # needs predict
    with pytest.raises(TypeError):
        model_far.tiled_sealed(predict_ways=8)
