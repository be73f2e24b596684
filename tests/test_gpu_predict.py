"""The predictive coder of escaped tiles on the device: idf_predict_prep_u8 bit for bit against the
numpy reference (tests/predict_ref.py) inside guard values, the streams word for word against the
C oracle, idf_predict_decode_u8 on the device's and on the reference's words inside guard bytes,
one damaged and one shortened stream among intact ones, and tiled_safe(predict=True) end to end:
exact round trips, the file sizes the reference predicts, the inner stream of tiled_safe(),
crops over packed, raw and kept tiles, and bytes that depend on neither chunking nor company.
Tiny models only."""
import functools

import numpy as np
import pytest
import torch

import predict_ref as ref
from test_gpu_safe import GUARD, _dev, _guarded, _guards_intact, _noise, _rows, _tiny_model
from test_predict_host import contents

pytestmark = pytest.mark.gpu

TILES = [(16, 16), (12, 8), (40, 33)]
L = 1 << 32
FGUARD = -7.25      # no x, mean or scale of the model


def _sizes(th, tw):
    """1x1, a full tile, a full tile over a 1 x tw strip, a full tile beside a th x 1 strip, 5x5,
    and 2 x 2 tiles with a 5-wide and 5-high edge (a 5x5 corner)."""
    return [(1, 1), (th, tw), (th + 1, tw), (th, tw + 1), (5, 5), (th + 5, tw + 5)]


@functools.lru_cache(maxsize=None)
def _case(C, th, tw):
    """Every content of test_predict_host.contents at every size of _sizes: the images, their
    rectangles' bytes in entry order and the reference's coding of each.  Computed once per
    (C, th, tw) and shared, never modified."""
    from idfcodec.safe import entry_rects
    from idfcodec.tiled import tile_table
    sizes, imgs = [], []
    for i, (H, W) in enumerate(_sizes(th, tw)):
        for name, p in contents((C, H, W), seed=17 * i).items():
            sizes.append((H, W))
            imgs.append(p)
    rects = entry_rects(sizes, th, tw)
    _, entries = tile_table(sizes, th, tw)
    planes = [np.ascontiguousarray(imgs[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w])
              for (i, ty, tx), (h, w) in zip(entries, rects)]
    counts = np.array([p.size for p in planes], dtype=np.int64)
    off = np.zeros(len(planes) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    sel = np.array([ref.choose_sel(p) for p in planes], dtype=np.uint32)
    arrs = [ref.arrays(p, int(s)) for p, s in zip(planes, sel)]
    x, mean, scale = (np.concatenate([a[i] for a in arrs]) for i in range(3))
    import rans_oracle
    fs, words, nw, status = rans_oracle.encode_streams(off, x, mean, scale)
    assert not status.any()
    return {"sizes": sizes, "imgs": imgs, "rects": rects, "planes": planes, "counts": counts,
            "off": off, "sel": sel, "x": x, "mean": mean, "scale": scale, "states": fs,
            "words": words, "nw": nw}


def _table(case, th, tw):
    src = [torch.from_numpy(i).cuda() for i in case["imgs"]]
    rows, _ = _rows(src, th, tw)
    return src, _dev(rows, torch.int64)


def _compact(case):
    """The reference's words, entry order and push order, and their offsets."""
    w_off = np.zeros(len(case["nw"]) + 1, dtype=np.int64)
    np.cumsum(case["nw"], out=w_off[1:])
    words = np.concatenate([case["words"][a:a + n] for a, n in zip(case["off"][:-1], case["nw"])])
    return words.astype(np.uint32), w_off


def _shapes_covered(case):
    return {(h, w) for h, w in case["rects"]}


# ------------------------------------------------------------------ 1. prep and encode
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_prep_equals_reference_inside_guards(C, th, tw):
    from idfcodec.predict import device_predict_prep
    case = _case(C, th, tw)
    assert {(1, 1), (1, tw), (th, 1), (5, 5), (th, tw)} <= _shapes_covered(case)
    src, table = _table(case, th, tw)
    n, nsym = len(case["planes"]), int(case["off"][-1])
    gap = 64
    bufs = [torch.full((nsym + 2 * gap,), FGUARD, dtype=torch.float32, device="cuda")
            for _ in range(3)]
    x, mean, scale = (b[gap:gap + nsym] for b in bufs)
    selbuf = torch.full((n + 2 * gap,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sel = selbuf[gap:gap + n]
    device_predict_prep(table, n, C, th, tw, _dev(case["off"], torch.int64), sel, x, mean, scale)
    torch.cuda.synchronize()
    assert np.array_equal(sel.cpu().numpy().view(np.uint32), case["sel"])
    for got, want in zip((x, mean, scale), (case["x"], case["mean"], case["scale"])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for b in bufs:
        assert bool((b[:gap] == FGUARD).all()) and bool((b[gap + nsym:] == FGUARD).all())
    assert bool((selbuf[:gap] == 0x5A5A5A5A).all()) and bool((selbuf[gap + n:] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_streams_equal_the_oracle_word_for_word(C, th, tw):
    from idfcodec.predict import device_predict_encode
    case = _case(C, th, tw)
    src, table = _table(case, th, tw)
    sel, states, nw, status, words = device_predict_encode(table, case["counts"], C, th, tw)
    assert not status.any()                   # every byte inside the window, every freq >= 1
    assert np.array_equal(sel, case["sel"])
    assert np.array_equal(nw, case["nw"])
    assert np.array_equal(states, case["states"])
    want, _ = _compact(case)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)


def test_a_tile_outside_the_image_has_no_symbols():
    """A negative origin: the raw gather stores nothing for such a tile, the prep codes nothing."""
    from idfcodec.predict import device_predict_prep
    img = torch.from_numpy(contents((3, 16, 16))["noise"]).cuda()
    rows = [[img.data_ptr(), 16, 16, -4, 0], [img.data_ptr(), 16, 16, 0, 0]]
    off = _dev([0, 0, 768], torch.int64)
    x, mean, scale = (torch.full((768,), FGUARD, dtype=torch.float32, device="cuda")
                      for _ in range(3))
    sel = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    device_predict_prep(_dev(rows, torch.int64), 2, 3, 16, 16, off, sel, x, mean, scale)
    want = ref.arrays(img.cpu().numpy())
    assert int(sel[0]) == 0 and int(sel[1]) & 0xFFFFFFFF == ref.choose_sel(img.cpu().numpy())
    assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(scale.cpu().numpy(), want[2])


# ------------------------------------------------------------------ 2. the decoder
def _decode(case, C, th, tw, words, w_off, nw, states=None, sel=None):
    """idf_predict_decode_u8 over every entry of the case into guarded bytes, the entries'
    outputs handed out in reverse order with 5 unused bytes between two: -> (big, out, offsets,
    the bytes expected, final states, status)."""
    from idfcodec.predict import device_predict_decode
    n = len(case["planes"])
    offs, o = [0] * n, 0
    for e in reversed(range(n)):
        offs[e] = o
        o += int(case["counts"][e]) + 5
    want = np.full(o, GUARD, dtype=np.uint8)
    for e, p in enumerate(case["planes"]):
        want[offs[e]:offs[e] + p.size] = p.reshape(-1)
    big, (out,) = _guarded([(o,)])
    final = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st = case["states"] if states is None else states
    sl = case["sel"] if sel is None else sel
    device_predict_decode(
        n, C, th, tw, torch.from_numpy(words.view(np.int32).copy()).cuda(),
        _dev(w_off[:n], torch.int64), _dev(nw, torch.int64),
        torch.from_numpy(st.view(np.int64).copy()).cuda(),
        torch.from_numpy(sl.view(np.int32).copy()).cuda(),
        _dev(case["rects"], torch.int32), _dev(offs, torch.int64), out, final, status)
    torch.cuda.synchronize()
    return big, out, offs, want, final.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_decode_returns_the_bytes_inside_guards(C, th, tw):
    from idfcodec.predict import device_predict_encode
    case = _case(C, th, tw)
    # the reference's own words
    words, w_off = _compact(case)
    big, out, offs, want, final, status = _decode(case, C, th, tw, words, w_off, case["nw"])
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])
    # the device encoder's words
    src, table = _table(case, th, tw)
    sel, states, nw, _, dwords = device_predict_encode(table, case["counts"], C, th, tw)
    d_off = np.zeros(len(nw) + 1, dtype=np.int64)
    np.cumsum(nw, out=d_off[1:])
    big, out, offs, want, final, status = _decode(
        case, C, th, tw, dwords.cpu().numpy().view(np.uint32), d_off, nw, states, sel)
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])


@pytest.mark.parametrize("shape", ["1", "2"])
def test_the_other_search_shapes_decode_the_same_bytes(monkeypatch, shape):
    """IDF_PREDICT_SEARCH (timing variants of the decoder's search: 1, five probes a lane in one
    round; 2, the two exact rounds without the guess) changes no byte, state or flag -- on intact
    words and on a damaged stream alike."""
    case = _case(3, 40, 33)
    words, w_off = _compact(case)
    bad = words.copy()
    e = _victim(case)
    bad[w_off[e] + case["nw"][e] // 2] ^= 0x00010000
    ref_run = _decode(case, 3, 40, 33, bad, w_off, case["nw"])
    monkeypatch.setenv("IDF_PREDICT_SEARCH", shape)
    big, out, offs, want, final, status = _decode(case, 3, 40, 33, words, w_off, case["nw"])
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])
    got = _decode(case, 3, 40, 33, bad, w_off, case["nw"])
    assert torch.equal(got[0], ref_run[0])
    assert np.array_equal(got[4], ref_run[4]) and np.array_equal(got[5], ref_run[5])


def test_decoded_bytes_scatter_into_a_crop_with_negative_origins():
    """The decoder's output has the raw bytes' layout: idf_tile_scatter_raw_u8 places it, here
    into a crop across four tiles, each clipped on two sides."""
    from idfcodec.predict import device_predict_decode, device_predict_encode
    from idfcodec.safe import device_scatter_raw, entry_rects, raw_offsets
    img = contents((3, 37, 21))["ramp"] ^ (_noise(37, 21, 90).numpy() & 3)
    src = torch.from_numpy(img).cuda()
    rows, _ = _rows([src], 16, 16)
    rects = entry_rects([(37, 21)], 16, 16)
    counts = [3 * h * w for h, w in rects]
    sel, states, nw, status, words = device_predict_encode(_dev(rows, torch.int64), counts, 3, 16,
                                                           16)
    offs, total = raw_offsets([True] * 6, rects, 3)
    w_off = np.concatenate([[0], np.cumsum(nw)[:-1]])
    raw = torch.empty(total, dtype=torch.uint8, device="cuda")
    final = torch.empty(6, dtype=torch.int64, device="cuda")
    st = torch.empty(6, dtype=torch.int32, device="cuda")
    device_predict_decode(6, 3, 16, 16, words, _dev(w_off, torch.int64), _dev(nw, torch.int64),
                          torch.from_numpy(states.view(np.int64).copy()).cuda(),
                          torch.from_numpy(sel.view(np.int32).copy()).cuda(),
                          _dev(rects, torch.int32), _dev(offs, torch.int64), raw, final, st)
    assert bool((final == L).all()) and not bool(st.any())
    y0, x0, h, w = 14, 13, 5, 6
    big, (crop,) = _guarded([(3, h, w)])
    crows = [[crop.data_ptr(), h, w, ty * 16 - y0, tx * 16 - x0] for ty in (0, 1) for tx in (0, 1)]
    device_scatter_raw(_dev(crows, torch.int64), 4, 3, 16, 16, raw, _dev(offs[:4], torch.int64),
                       _dev(rects[:4], torch.int32))
    assert _guards_intact(big, [crop], [img[:, y0:y0 + h, x0:x0 + w]])


# ------------------------------------------------------------------ 3. damage
def _victim(case):
    """An entry of several words among the others: a full noise tile."""
    return int(np.argmax(case["nw"]))


def _others_exact(case, e_bad, out, offs, final, status):
    got = out.cpu().numpy()
    for e, p in enumerate(case["planes"]):
        if e == e_bad:
            continue
        assert np.array_equal(got[offs[e]:offs[e] + p.size], p.reshape(-1)), e
        assert final[e] == L and status[e] == 0, e


def test_a_flipped_word_is_reported_and_stays_in_its_entry():
    """A bounds check, run once: the call returns, the entry whose word was flipped is flagged (a
    status flag or a final state other than L), every other entry and every guard byte is
    exact."""
    C, th, tw = 3, 16, 16
    case = _case(C, th, tw)
    words, w_off = _compact(case)
    e = _victim(case)
    assert case["nw"][e] >= 8
    words = words.copy()
    words[w_off[e] + case["nw"][e] // 2] ^= 0x00010000
    big, out, offs, want, final, status = _decode(case, C, th, tw, words, w_off, case["nw"])
    assert status[e] != 0 or final[e] != L
    _others_exact(case, e, out, offs, final, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])   # whatever the entry holds, nothing around it moved


def test_a_missing_word_is_an_underflow():
    """A bounds check, run once.  The first word pushed is the last one read: without it every
    symbol up to that read decodes as before and the read finds no word -- UNDERFLOW, whatever
    the bytes.  With the last word pushed dropped instead (the same offsets, nwords - 1) the
    decoder starts on the wrong word; the entry is flagged one way or another."""
    C, th, tw = 3, 16, 16
    case = _case(C, th, tw)
    words, w_off = _compact(case)
    e = _victim(case)
    nw = case["nw"].copy()
    nw[e] -= 1
    first = w_off.copy()
    first[e] += 1
    big, out, offs, want, final, status = _decode(case, C, th, tw, words, first, nw)
    assert status[e] & ref.UNDERFLOW
    _others_exact(case, e, out, offs, final, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])
    big, out, offs, want, final, status = _decode(case, C, th, tw, words, w_off, nw)
    assert status[e] != 0 or final[e] != L
    _others_exact(case, e, out, offs, final, status)


# ------------------------------------------------------------------ 4. end to end
SIZES = ((1, 1), (16, 16), (17, 16), (5, 40), (37, 21))


def _smooth(H, W, seed, C=3):
    """A ramp plus noise 0..3, uint8 [C, H, W]"""
    return torch.from_numpy(contents((C, H, W))["ramp"]) + (_noise(H, W, seed, C) & 3)


@pytest.fixture(scope="module")
def model_far():
    """test_gpu_safe's: the top level's prior mean moved 8.0 away, so every tile escapes."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    prior = m.blocks[-1]["prior"]
    with torch.no_grad():
        prior.NN.layers[-1].bias[:prior.out_channel] += 8.0
    return m.cuda()


@pytest.fixture(scope="module")
def model_sharp():
    """test_gpu_safe's: every prior's logscale lowered by 3.0, so dark tiles are kept."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            b["prior"].NN.layers[-1].bias[b["prior"].out_channel:] -= 3.0
    return m.cuda()


def _planes_of(imgs, lay):
    th, tw = lay.tile_hw
    return [imgs[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w].cpu().numpy()
            for (i, ty, tx), (h, w) in zip(lay.entries, lay.rects)]


def test_smooth_images_round_trip_and_shrink_by_what_the_reference_predicts(model_far):
    from idfcodec.predict import PredictiveTiledBitstream, file_size_bound_packed
    imgs = [_smooth(H, W, 40 + i).cuda() for i, (H, W) in enumerate(SIZES)]
    pc = model_far.tiled_safe(predict=True)
    pbs = pc.encode(imgs)
    buf = pbs.to_bytes()
    outs, info = pc.decode(PredictiveTiledBitstream.from_bytes(buf, device="cuda"))
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))
    assert pbs.escaped.all() and pbs.n_packed > 0
    assert info["packed_tiles"] == pbs.n_packed and info["raw_tiles"] == 13 - pbs.n_packed
    # both sizes from the reference: an entry costs its bytes raw, or 16 + 4 * nwords packed
    planes = _planes_of(imgs, pbs.layout)
    cost = [ref.packed_cost(p) for p in planes]
    assert pbs.packed.tolist() == [c < p.size for c, p in zip(cost, planes)]
    head = len(pbs.layout.pack(b"IDFP")) + 2          # 13 tiles: a bitmap of 2 bytes
    n_src = sum(p.size for p in planes)
    safe_size = head + 8 + n_src + 8
    assert len(model_far.tiled_safe().encode(imgs).to_bytes()) == safe_size
    assert len(buf) == head + 2 + 8 + 8 + 4 + sum(cost) + 8
    assert len(buf) < safe_size
    assert len(buf) <= file_size_bound_packed(SIZES, 3, 16, 16, 2, kept=False)


def test_noise_packs_nothing_and_costs_the_fixed_overhead(model_far):
    from idfcodec.predict import file_size_bound_packed
    imgs = [_noise(H, W, 70 + i).cuda() for i, (H, W) in enumerate(SIZES)]
    pc = model_far.tiled_safe(predict=True)
    pbs = pc.encode(imgs)
    assert pbs.n_packed == 0 and pbs.escaped.all() and pbs.words.numel() == 0
    buf = pbs.to_bytes()
    safe = model_far.tiled_safe().encode(imgs).to_bytes()
    # the packed bitmap over 13 escaped tiles, the section's u64 length and its u32 count
    assert len(buf) == len(safe) + 2 + 8 + 4
    assert len(buf) <= file_size_bound_packed(SIZES, 3, 16, 16, 2, kept=False)
    outs, info = pc.decode(pbs)
    assert info["ok"] and info["raw_tiles"] == 13 and info["packed_tiles"] == 0
    assert all(torch.equal(a, b) for a, b in zip(outs, imgs))


@pytest.fixture(scope="module")
def mixed():
    """A 32x48 image of six tiles -- dark (bytes 0..3), noise, smooth / smooth, dark, noise -- and
    three more images, one of each kind."""
    dark = lambda H, W, s: _noise(H, W, s) % 4  # noqa: E731
    top = torch.cat([dark(16, 16, 80), _noise(16, 16, 81), _smooth(16, 16, 82)], dim=2)
    bottom = torch.cat([_smooth(16, 16, 83), dark(16, 16, 84), _noise(16, 16, 85)], dim=2)
    return [t.contiguous().cuda() for t in (torch.cat([top, bottom], dim=1), dark(17, 16, 86),
                                            _smooth(37, 21, 87), _noise(5, 40, 88))]


def test_mixed_set_keeps_the_inner_stream_of_tiled_safe(model_sharp, mixed):
    from idfcodec.predict import PredictiveTiledBitstream
    pc = model_sharp.tiled_safe(predict=True)
    pbs = pc.encode(mixed)
    sbs = model_sharp.tiled_safe().encode(mixed)
    assert pbs.n_kept > 0 and pbs.n_packed > 0 and pbs.stored_raw.any()
    assert pbs.escaped.tolist() == sbs.escaped.tolist()
    assert pbs.stream.to_bytes() == sbs.stream.to_bytes()
    assert np.array_equal(pbs.reasons, sbs.reasons)
    got = PredictiveTiledBitstream.from_bytes(pbs.to_bytes(), device="cuda")
    outs, info = pc.decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, mixed))
    assert info["tiles"] == 6 + 2 + 6 + 3
    assert info["packed_tiles"] == pbs.n_packed and info["raw_tiles"] == int(pbs.stored_raw.sum())
    # one image alone, out of order
    outs, info = pc.decode(got, images=[2, 0])
    assert info["ok"] and torch.equal(outs[0], mixed[2]) and torch.equal(outs[1], mixed[0])


def test_region_over_packed_raw_and_kept_tiles(model_sharp, mixed):
    pc = model_sharp.tiled_safe(predict=True)
    pbs = pc.encode(mixed)
    kinds = [("kept" if not e else "packed" if p else "raw")
             for e, p in zip(pbs.escaped[:6], pbs.packed[:6])]
    assert set(kinds) == {"kept", "packed", "raw"}, kinds
    y0, x0, h, w = 10, 9, 15, 30            # all six tiles of image 0, each clipped
    crop, info = pc.decode_region(pbs, 0, y0, x0, h, w)
    assert info["ok"] and info["tiles"] == 6
    assert info["packed_tiles"] == kinds.count("packed") and info["raw_tiles"] == kinds.count("raw")
    assert torch.equal(crop, mixed[0][:, y0:y0 + h, x0:x0 + w])
    # a crop inside one packed tile: no flow runs
    e = kinds.index("packed")
    ty, tx = divmod(e, 3)
    crop, info = pc.decode_region(pbs, 0, ty * 16 + 3, tx * 16 + 2, 9, 11)
    assert info["ok"] and info["tiles"] == 1 and info["packed_tiles"] == 1
    assert info["final_states"].numel() == 0
    assert torch.equal(crop, mixed[0][:, ty * 16 + 3:ty * 16 + 12, tx * 16 + 2:tx * 16 + 13])


def test_bytes_depend_on_neither_max_batch_nor_company(model_sharp, mixed):
    from idfcodec.predict import PredictiveTileCodec
    a = PredictiveTileCodec(model_sharp, max_batch=2).encode(mixed)
    b = PredictiveTileCodec(model_sharp, max_batch=256).encode(mixed)
    assert a.to_bytes() == b.to_bytes()
    alone = PredictiveTileCodec(model_sharp).encode([mixed[0]])
    n, P = alone.n_entries, alone.n_packed
    assert alone.escaped.tolist() == b.escaped[:n].tolist()
    assert alone.packed.tolist() == b.packed[:n].tolist() and P > 0
    assert np.array_equal(alone.sel, b.sel[:P]) and np.array_equal(alone.states, b.states[:P])
    assert np.array_equal(alone.nwords, b.nwords[:P])
    assert torch.equal(alone.words.cpu(), b.words[:int(alone.nwords.sum())].cpu())
    assert torch.equal(alone.raw.cpu(), b.raw[:alone.raw.numel()].cpu())


def test_verify_catches_a_damaged_packed_entry(model_far):
    imgs = [_smooth(16, 16, 60).cuda(), _smooth(37, 21, 61).cuda()]
    pc = model_far.tiled_safe(predict=True)
    pbs = pc.encode(imgs)
    assert pbs.n_packed >= 2 and int(pbs.nwords[0]) >= 4
    pbs.words = pbs.words.clone()
    pbs.words[2] ^= 0x00010000
    outs, info = pc.decode(pbs)
    assert not info["ok"]
    assert torch.equal(outs[1][:, 16:, :], imgs[1][:, 16:, :])     # other entries stay exact


def test_default_tiled_safe_is_unchanged(model_far):
    from idfcodec.predict import PredictiveTileCodec
    from idfcodec.safe import SafeTiledCodec
    imgs = [_smooth(H, W, 40 + i).cuda() for i, (H, W) in enumerate(SIZES)]
    sc = model_far.tiled_safe()
    assert type(sc) is SafeTiledCodec and model_far.tiled_safe() is sc
    assert model_far.tiled_safe(predict=False) is sc
    pc = model_far.tiled_safe(predict=True)
    assert type(pc) is PredictiveTileCodec and model_far.tiled_safe(predict=True) is pc
    assert model_far.tiled_safe() is sc                # the two caches do not evict each other
    assert sc.encode(imgs).to_bytes() == SafeTiledCodec(model_far).encode(imgs).to_bytes()
    with pytest.raises(TypeError):
        model_far.tiled_sealed(predict=True)
