"""The colour mode of the predictive coder on the device: idf_predict_prep2_u8 bit for bit against
the numpy reference (tests/colour_ref.py) inside guard values, both candidates' streams word for
word against the C oracle, idf_predict_decode2_u8 on a mix of plain and colour entries inside
guard bytes (the plain ones as idf_predict_decode_u8 decodes them), its refusal of C < 3, one
damaged and one shortened colour stream among intact ones, and tiled_safe(predict="colour") end
to end: exact round trips, the choices and file sizes the reference predicts, the inner stream of
tiled_safe(), a crop over kept, raw, plain and colour tiles, bytes that depend on neither chunking
nor company, and the IDFP bytes of the default predictive path, frozen.  Tiny models only."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

import colour_ref as cref
import predict_ref as ref
from conftest import GOLDEN
from test_gpu_predict import (FGUARD, SIZES, TILES, _compact, _planes_of, _sizes, _table,
                              model_far, model_sharp)  # noqa: F401 (fixtures)
from test_gpu_safe import GUARD, _dev, _guarded, _guards_intact, _noise
from test_predict_host import contents

pytestmark = pytest.mark.gpu

L = 1 << 32
SELGUARD = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _case(C, th, tw):
    """Every content of test_predict_host.contents and the two generators at every size of
    test_gpu_predict._sizes: the images, their rectangles' bytes in entry order and the
    reference's coding of both candidates of each (stream 2e plain, 2e + 1 colour).  Computed
    once per (C, th, tw) and shared, never modified."""
    import rans_oracle
    from idfcodec.safe import entry_rects
    from idfcodec.tiled import tile_table
    sizes, imgs = [], []
    for i, (H, W) in enumerate(_sizes(th, tw)):
        both = dict(contents((C, H, W), seed=17 * i))
        both["correlated"] = cref.correlated(H, W, i, C)
        both["independent"] = cref.independent(H, W, i, C)
        for name, p in both.items():
            sizes.append((H, W))
            imgs.append(p)
    rects = entry_rects(sizes, th, tw)
    _, entries = tile_table(sizes, th, tw)
    planes = [np.ascontiguousarray(imgs[i][:, ty * th:ty * th + h, tx * tw:tx * tw + w])
              for (i, ty, tx), (h, w) in zip(entries, rects)]
    counts = np.array([p.size for p in planes], dtype=np.int64)
    off = np.zeros(2 * len(planes) + 1, dtype=np.int64)
    np.cumsum(np.repeat(counts, 2), out=off[1:])
    sel = np.array([(ref.choose_sel(p),) + cref.choose_sels(p) for p in planes], dtype=np.uint32)
    arrs = []
    for p, s in zip(planes, sel):
        arrs += [ref.arrays(p, int(s[0])), cref.arrays(p, int(s[1]), int(s[2]))]
    x, mean, scale = (np.concatenate([a[i] for a in arrs]) for i in range(3))
    fs, words, nw, status = rans_oracle.encode_streams(off, x, mean, scale)
    assert not status.any()
    return {"sizes": sizes, "imgs": imgs, "rects": rects, "planes": planes, "counts": counts,
            "off": off, "sel": sel, "x": x, "mean": mean, "scale": scale, "states": fs,
            "words": words, "nw": nw}


# ------------------------------------------------------------------ 1. prep and encode
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_prep_of_both_candidates_equals_reference_inside_guards(C, th, tw):
    from idfcodec.predict import device_predict_prep2
    case = _case(C, th, tw)
    assert {(1, 1), (1, tw), (th, 1), (5, 5), (th, tw)} <= {(h, w) for h, w in case["rects"]}
    src, table = _table(case, th, tw)
    n, nsym = len(case["planes"]), int(case["off"][-1])
    gap = 64
    bufs = [torch.full((nsym + 2 * gap,), FGUARD, dtype=torch.float32, device="cuda")
            for _ in range(3)]
    x, mean, scale = (b[gap:gap + nsym] for b in bufs)
    selbuf = torch.full((3 * n + 2 * gap,), SELGUARD, dtype=torch.int32, device="cuda")
    sel = selbuf[gap:gap + 3 * n]
    device_predict_prep2(table, n, C, th, tw, _dev(case["off"], torch.int64), sel, x, mean, scale)
    torch.cuda.synchronize()
    assert np.array_equal(sel.cpu().numpy().view(np.uint32).reshape(n, 3), case["sel"])
    for got, want in zip((x, mean, scale), (case["x"], case["mean"], case["scale"])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for b in bufs:
        assert bool((b[:gap] == FGUARD).all()) and bool((b[gap + nsym:] == FGUARD).all())
    assert bool((selbuf[:gap] == SELGUARD).all()) and bool((selbuf[gap + 3 * n:] == SELGUARD).all())


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_both_candidates_streams_equal_the_oracle_word_for_word(C, th, tw):
    from idfcodec.predict import device_predict_encode, device_predict_encode2
    case = _case(C, th, tw)
    src, table = _table(case, th, tw)
    sel, states, nw, status, words = device_predict_encode2(table, case["counts"], C, th, tw)
    assert not status.any()
    assert np.array_equal(sel, case["sel"])
    assert np.array_equal(nw, case["nw"]) and np.array_equal(states, case["states"])
    want, w_off = _compact(case)
    got = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    # the plain candidate is idf_predict_prep_u8's stream
    sel1, states1, nw1, _, words1 = device_predict_encode(table, case["counts"], C, th, tw)
    assert np.array_equal(sel1, sel[:, 0]) and np.array_equal(states1, states[0::2])
    assert np.array_equal(nw1, nw[0::2])
    plain = np.concatenate([got[w_off[2 * e]:w_off[2 * e + 1]] for e in range(len(nw1))])
    assert np.array_equal(words1.cpu().numpy().view(np.uint32), plain)


@pytest.mark.parametrize("th,tw", TILES)
def test_best_gathers_the_chosen_packed_streams_alone(th, tw):
    """device_predict_encode2(best=True): the same sels, states, counts and status, and the words
    of the streams choose_streams picks and packs, in entry order."""
    from idfcodec.predict import choose_streams, device_predict_encode2
    case = _case(3, th, tw)
    src, table = _table(case, th, tw)
    sel, states, nw, status, words = device_predict_encode2(table, case["counts"], 3, th, tw,
                                                            best=True)
    assert np.array_equal(sel, case["sel"]) and np.array_equal(nw, case["nw"])
    assert np.array_equal(states, case["states"]) and not status.any()
    col, pick, hit = choose_streams(case["nw"], status, case["counts"])
    assert col.any() and (~col).any() and hit.any() and (~hit).any()
    all_words, w_off = _compact(case)
    want = np.concatenate([all_words[w_off[k]:w_off[k + 1]] for k in pick[hit]])
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want)


def test_offsets_that_do_not_fit_write_nothing():
    from idfcodec.predict import device_predict_prep2
    img = torch.from_numpy(cref.correlated(16, 16, 3)).cuda()
    rows = [[img.data_ptr(), 16, 16, -4, 0], [img.data_ptr(), 16, 16, 0, 0],
            [img.data_ptr(), 16, 16, 0, 0]]
    off = _dev([0, 0, 0, 768, 1536, 1536 + 700, 1536 + 1400], torch.int64)   # entry 2: 700 each
    x, mean, scale = (torch.full((3000,), FGUARD, dtype=torch.float32, device="cuda")
                      for _ in range(3))
    sel = torch.full((9,), -1, dtype=torch.int32, device="cuda")
    device_predict_prep2(_dev(rows, torch.int64), 3, 3, 16, 16, off, sel, x, mean, scale)
    p = img.cpu().numpy()
    want = (ref.choose_sel(p),) + cref.choose_sels(p)
    assert sel.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, *want, 0, 0, 0]
    assert np.array_equal(x[:768].cpu().numpy(), ref.arrays(p)[0])
    assert np.array_equal(x[768:1536].cpu().numpy(), cref.arrays(p)[0])
    assert np.array_equal(scale[768:1536].cpu().numpy(), cref.arrays(p)[2])
    assert bool((x[1536:] == FGUARD).all()) and bool((scale[1536:] == FGUARD).all())


# ------------------------------------------------------------------ 2. the decoder
def _mix(case, words, w_off, nw, states, sel):
    """Entries alternate: even ones are decoded from their colour stream, odd ones from their
    plain stream.  -> the decoder's per-entry arguments (words stay where they are)."""
    n = len(case["planes"])
    col = np.arange(n) % 2 == 0
    pick = 2 * np.arange(n) + col
    return {"col": col, "w_off": w_off[pick], "nw": np.asarray(nw)[pick],
            "states": np.asarray(states)[pick], "words": words,
            "sel": np.where(col, sel[:, 1], sel[:, 0]).astype(np.uint32),
            "sel2": sel[:, 2].astype(np.uint32)}


def _layout(case):
    """Output offsets handed out in reverse entry order with 5 unused bytes between two, and the
    bytes expected around them."""
    n = len(case["planes"])
    offs, o = [0] * n, 0
    for e in reversed(range(n)):
        offs[e] = o
        o += int(case["counts"][e]) + 5
    want = np.full(o, GUARD, dtype=np.uint8)
    for e, p in enumerate(case["planes"]):
        want[offs[e]:offs[e] + p.size] = p.reshape(-1)
    return offs, want


def _decode2(case, C, th, tw, m, plain_call=False):
    """idf_predict_decode2_u8 (plain_call: idf_predict_decode_u8 on the same arguments) over
    every entry into guarded bytes -> (big, out, offsets, the bytes expected, final, status)."""
    from idfcodec.predict import device_predict_decode, device_predict_decode2
    n = len(case["planes"])
    offs, want = _layout(case)
    big, (out,) = _guarded([(len(want),)])
    final = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    words = torch.from_numpy(m["words"].view(np.int32).copy()).cuda()
    a = (_dev(m["w_off"], torch.int64), _dev(m["nw"], torch.int64),
         torch.from_numpy(m["states"].view(np.int64).copy()).cuda(),
         torch.from_numpy(m["sel"].view(np.int32).copy()).cuda())
    tail = (_dev(case["rects"], torch.int32), _dev(offs, torch.int64), out, final, status)
    if plain_call:
        device_predict_decode(n, C, th, tw, words, *a, *tail)
    else:
        device_predict_decode2(n, C, th, tw, words, *a,
                               torch.from_numpy(m["sel2"].view(np.int32).copy()).cuda(),
                               torch.from_numpy(m["col"].astype(np.uint8)).cuda(),
                               int(m["col"].sum()), *tail)
    torch.cuda.synchronize()
    return big, out, offs, want, final.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("th,tw", TILES)
def test_decode_of_mixed_entries_returns_the_bytes_inside_guards(C, th, tw):
    from idfcodec.predict import device_predict_encode2
    case = _case(C, th, tw)
    assert th * tw % 64 or (th, tw) == (16, 16)     # 12x8 and 40x33: planes end inside a batch
    # the reference's own words
    words, w_off = _compact(case)
    m = _mix(case, words, w_off, case["nw"], case["states"], case["sel"])
    big, out, offs, want, final, status = _decode2(case, C, th, tw, m)
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])
    # the plain entries: what idf_predict_decode_u8 makes of the same arguments
    big1, out1, _, _, final1, status1 = _decode2(case, C, th, tw, m, plain_call=True)
    g2, g1 = out.cpu().numpy(), out1.cpu().numpy()
    for e in np.flatnonzero(~m["col"]):
        a, b = offs[e], offs[e] + int(case["counts"][e])
        assert np.array_equal(g2[a:b], g1[a:b]), e
    assert np.array_equal(final[~m["col"]], final1[~m["col"]])
    assert np.array_equal(status[~m["col"]], status1[~m["col"]])
    # the device encoder's words
    src, table = _table(case, th, tw)
    sel, states, nw, _, dwords = device_predict_encode2(table, case["counts"], C, th, tw)
    d_off = np.zeros(len(nw) + 1, dtype=np.int64)
    np.cumsum(nw, out=d_off[1:])
    m = _mix(case, dwords.cpu().numpy().view(np.uint32), d_off, nw, states, sel)
    big, out, offs, want, final, status = _decode2(case, C, th, tw, m)
    assert (final == L).all() and not status.any()
    assert _guards_intact(big, [out], [want])


def test_no_colour_entry_is_the_plain_call():
    """n_colour == 0: neither the flags nor sel2 is read (both NULL here)."""
    from idfcodec._lib import lib, ptr, stream_ptr
    C, th, tw = 3, 12, 8
    case = _case(C, th, tw)
    words, w_off = _compact(case)
    n = len(case["planes"])
    pick = 2 * np.arange(n)
    offs, want = _layout(case)
    big, (out,) = _guarded([(len(want),)])
    final = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    keep = [torch.from_numpy(words.view(np.int32).copy()).cuda(), _dev(w_off[pick], torch.int64),
            _dev(case["nw"][pick], torch.int64),
            torch.from_numpy(case["states"][pick].view(np.int64).copy()).cuda(),
            torch.from_numpy(case["sel"][:, 0].copy().view(np.int32)).cuda()]
    tail = [_dev(case["rects"], torch.int32), _dev(offs, torch.int64), out, final, status]
    rc = lib().idf_predict_decode2_u8(stream_ptr(out.device), n, 0, C, th, tw,
                                      *[ptr(t) for t in keep], None, None,
                                      *[ptr(t) for t in tail])
    torch.cuda.synchronize()
    assert rc == 0 and bool((final == L).all()) and not bool(status.any())
    assert _guards_intact(big, [out], [want])


def test_one_plane_with_a_colour_flag_is_refused_and_writes_nothing():
    from idfcodec._lib import lib, ptr, stream_ptr
    p = contents((1, 12, 8))["ramp"]
    sel, state, words = ref.encode(p)
    big, (out,) = _guarded([(96,)])
    final = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    args = [torch.from_numpy(words.view(np.int32).copy()).cuda(), _dev([0], torch.int64),
            _dev([len(words)], torch.int64),
            torch.from_numpy(np.array([state], dtype=np.uint64).view(np.int64)).cuda(),
            torch.from_numpy(np.array([sel], dtype=np.uint32).view(np.int32)).cuda(),
            _dev([0], torch.int32),
            torch.ones(1, dtype=torch.uint8, device="cuda"), _dev([[12, 8]], torch.int32),
            _dev([0], torch.int64), out, final, status]
    for C in (1, 2):
        rc = lib().idf_predict_decode2_u8(stream_ptr(out.device), 1, 1, C, 12, 8,
                                          *[ptr(t) for t in args])
        torch.cuda.synchronize()
        assert rc == 1                                    # IDF_ERR_ARG
    assert bool((big == GUARD).all()) and int(final[0]) == 77 and int(status[0]) == -1
    # without the flag the same arguments decode
    rc = lib().idf_predict_decode2_u8(stream_ptr(out.device), 1, 0, 1, 12, 8,
                                      *[ptr(t) for t in args])
    torch.cuda.synchronize()
    assert rc == 0 and int(final[0]) == L and int(status[0]) == 0
    assert _guards_intact(big, [out], [p.reshape(-1)])


# ------------------------------------------------------------------ 3. damage
def _victim(case, m):
    """A colour entry of several words among the others: the largest of them."""
    nw = np.where(m["col"], m["nw"], -1)
    return int(np.argmax(nw))


def _others_exact(case, e_bad, out, offs, final, status):
    got = out.cpu().numpy()
    for e, p in enumerate(case["planes"]):
        if e == e_bad:
            continue
        assert np.array_equal(got[offs[e]:offs[e] + p.size], p.reshape(-1)), e
        assert final[e] == L and status[e] == 0, e


def test_a_flipped_word_in_a_colour_entry_is_reported_and_stays_in_its_entry():
    """A bounds check, run once: the call returns, the colour entry whose word was flipped is
    flagged (a status flag or a final state other than L), every other entry and every guard byte
    is exact -- the inverse transform included, which rewrites only the entry's own bytes."""
    C, th, tw = 3, 16, 16
    case = _case(C, th, tw)
    words, w_off = _compact(case)
    m = _mix(case, words.copy(), w_off, case["nw"], case["states"], case["sel"])
    e = _victim(case, m)
    assert m["col"][e] and m["nw"][e] >= 8
    m["words"][m["w_off"][e] + m["nw"][e] // 2] ^= 0x00010000
    big, out, offs, want, final, status = _decode2(case, C, th, tw, m)
    assert status[e] != 0 or final[e] != L
    _others_exact(case, e, out, offs, final, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])   # whatever the entry holds, nothing around it moved


def test_a_missing_word_in_a_colour_entry_is_an_underflow():
    """A bounds check, run once.  The first word pushed is the last one read: without it the
    read finds no word -- UNDERFLOW -- and the entry stops there."""
    C, th, tw = 3, 16, 16
    case = _case(C, th, tw)
    words, w_off = _compact(case)
    m = _mix(case, words, w_off, case["nw"], case["states"], case["sel"])
    e = _victim(case, m)
    m["nw"] = m["nw"].copy()
    m["w_off"] = m["w_off"].copy()
    m["nw"][e] -= 1
    m["w_off"][e] += 1
    big, out, offs, want, final, status = _decode2(case, C, th, tw, m)
    assert status[e] & ref.UNDERFLOW
    _others_exact(case, e, out, offs, final, status)
    got = out.cpu().numpy()
    want[offs[e]:offs[e] + case["counts"][e]] = got[offs[e]:offs[e] + case["counts"][e]]
    assert _guards_intact(big, [out], [want])


# ------------------------------------------------------------------ 4. end to end
def _reference(imgs, lay):
    """-> (the entries' bytes, the reference's (kind, cost) of each)"""
    planes = _planes_of(imgs, lay)
    return planes, [cref.choice(p) for p in planes]


def _e2e(model_far):
    imgs = [torch.from_numpy(i).cuda() for i in cref.end_to_end_input(SIZES)]
    return imgs, model_far.tiled_safe(predict="colour")


def test_patchwork_round_trips_and_matches_the_reference(model_far):
    from idfcodec.predict import PredictiveTiledBitstream, file_size_bound_packed
    imgs, qc = _e2e(model_far)
    qbs = qc.encode(imgs)
    buf = qbs.to_bytes()
    assert buf[:4] == b"IDFQ" and qbs.escaped.all()
    got = PredictiveTiledBitstream.from_bytes(buf, device="cuda")
    outs, info = qc.decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))
    planes, choice = _reference(imgs, qbs.layout)
    kinds = [k for k, _ in choice]
    assert {"raw", "plain", "colour"} <= set(kinds), kinds
    assert qbs.packed.tolist() == [k != "raw" for k in kinds]
    assert qbs.colour.tolist() == [k == "colour" for k in kinds]
    assert info["packed_tiles"] == qbs.n_packed and info["colour_tiles"] == qbs.n_colour
    assert info["raw_tiles"] == kinds.count("raw")
    want_sel, want_sel2 = [], []
    for p, k in zip(planes, kinds):
        if k == "plain":
            want_sel.append(ref.choose_sel(p))
        elif k == "colour":
            s, s2 = cref.choose_sels(p)
            want_sel.append(s)
            want_sel2.append(s2)
    assert qbs.sel.tolist() == want_sel and qbs.sel2.tolist() == want_sel2
    # the file: header, escape + packed bitmaps (13 tiles: 2 bytes each), the colour bitmap, the
    # three u64 lengths, P and Q, and every entry at the reference's cost
    P = qbs.n_packed
    head = len(qbs.layout.pack(b"IDFQ")) + 2 + 2 + -(-P // 8)
    assert len(buf) == head + 8 + 8 + 4 + 4 + sum(c for _, c in choice) + 8
    assert len(buf) <= file_size_bound_packed(SIZES, 3, 16, 16, 2, kept=False, colour=True)
    # against the IDFP file of the same call: every entry costs at most its plain cost
    pbuf = model_far.tiled_safe(predict=True).encode(imgs).to_bytes()
    assert len(buf) <= len(pbuf) + -(-P // 8) + 4
    # the predict=True codec reads the IDFQ stream too
    outs, info = model_far.tiled_safe(predict=True).decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))


def test_correlated_images_are_smaller_than_their_idfp_file(model_far):
    imgs = [torch.from_numpy(cref.correlated(H, W, 50 + i)).cuda()
            for i, (H, W) in enumerate(SIZES)]
    qc = model_far.tiled_safe(predict="colour")
    qbs = qc.encode(imgs)
    buf = qbs.to_bytes()
    pbuf = model_far.tiled_safe(predict=True).encode(imgs).to_bytes()
    assert qbs.n_colour > 0 and len(buf) < len(pbuf)
    assert len(buf) <= len(pbuf) + -(-qbs.n_packed // 8) + 4
    planes, choice = _reference(imgs, qbs.layout)
    assert qbs.colour.tolist() == [k == "colour" for k, _ in choice]
    assert all(k == "colour" for (k, _), p in zip(choice, planes) if p.shape[1:] == (16, 16))
    outs, info = qc.decode(qbs)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))


def test_default_predictive_path_writes_the_parent_bytes(model_far):
    """tiled_safe(predict=True) on the patchwork set: every tile escapes under model_far, so the
    bytes depend on the predictor alone.  The digest was recorded before the colour mode
    existed."""
    imgs, _ = _e2e(model_far)
    buf = model_far.tiled_safe(predict=True).encode(imgs).to_bytes()
    with open(os.path.join(GOLDEN, "idfp_patchwork.sha256")) as f:
        want = f.read().split()
    assert buf[:4] == b"IDFP" and [str(len(buf)), hashlib.sha256(buf).hexdigest()] == want


def test_the_three_codecs_are_cached_apart(model_far):
    from idfcodec.predict import PredictiveTileCodec
    qc = model_far.tiled_safe(predict="colour")
    pc = model_far.tiled_safe(predict=True)
    assert type(qc) is PredictiveTileCodec and qc.colour and not pc.colour
    assert model_far.tiled_safe(predict="colour") is qc and model_far.tiled_safe(predict=True) is pc
    assert model_far.tiled_safe() is not pc and model_far.tiled_safe(predict="colour") is qc
    with pytest.raises(ValueError):
        model_far.tiled_safe(predict="color")


@pytest.fixture(scope="module")
def mixed():
    """A 32x48 image of six tiles -- dark (bytes 0..3), noise, correlated / independent, dark,
    correlated -- and three more images, one of each coded kind."""
    dark = lambda H, W, s: _noise(H, W, s) % 4  # noqa: E731
    cor = lambda H, W, s: torch.from_numpy(cref.correlated(H, W, s))  # noqa: E731
    ind = lambda H, W, s: torch.from_numpy(cref.independent(H, W, s))  # noqa: E731
    top = torch.cat([dark(16, 16, 80), _noise(16, 16, 81), cor(16, 16, 82)], dim=2)
    bottom = torch.cat([ind(16, 16, 83), dark(16, 16, 84), cor(16, 16, 85)], dim=2)
    return [t.contiguous().cuda() for t in (torch.cat([top, bottom], dim=1), dark(17, 16, 86),
                                            cor(37, 21, 87), ind(5, 40, 88))]


def _kinds(qbs, n=None):
    return [("kept" if not e else "raw" if not p else "colour" if c else "plain")
            for e, p, c in zip(qbs.escaped[:n], qbs.packed[:n], qbs.colour[:n])]


def test_mixed_set_keeps_the_inner_stream_and_crops_over_every_kind(model_sharp, mixed):
    from idfcodec.predict import PredictiveTiledBitstream
    qc = model_sharp.tiled_safe(predict="colour")
    qbs = qc.encode(mixed)
    sbs = model_sharp.tiled_safe().encode(mixed)
    assert qbs.escaped.tolist() == sbs.escaped.tolist()
    assert qbs.stream.to_bytes() == sbs.stream.to_bytes()
    assert np.array_equal(qbs.reasons, sbs.reasons)
    kinds = _kinds(qbs, 6)
    assert set(kinds) == {"kept", "raw", "plain", "colour"}, kinds
    got = PredictiveTiledBitstream.from_bytes(qbs.to_bytes(), device="cuda")
    outs, info = qc.decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, mixed))
    assert info["tiles"] == 6 + 2 + 6 + 3 and info["colour_tiles"] == qbs.n_colour
    outs, info = qc.decode(got, images=[2, 0])
    assert info["ok"] and torch.equal(outs[0], mixed[2]) and torch.equal(outs[1], mixed[0])
    y0, x0, h, w = 10, 9, 15, 30            # all six tiles of image 0, each clipped
    crop, info = qc.decode_region(got, 0, y0, x0, h, w)
    assert info["ok"] and info["tiles"] == 6
    assert info["colour_tiles"] == kinds.count("colour")
    assert info["packed_tiles"] == kinds.count("colour") + kinds.count("plain")
    assert info["raw_tiles"] == kinds.count("raw")
    assert torch.equal(crop, mixed[0][:, y0:y0 + h, x0:x0 + w])
    # a crop inside one colour tile: no flow runs
    ty, tx = divmod(kinds.index("colour"), 3)
    crop, info = qc.decode_region(got, 0, ty * 16 + 3, tx * 16 + 2, 9, 11)
    assert info["ok"] and info["tiles"] == 1 and info["colour_tiles"] == 1
    assert info["final_states"].numel() == 0
    assert torch.equal(crop, mixed[0][:, ty * 16 + 3:ty * 16 + 12, tx * 16 + 2:tx * 16 + 13])


def test_bytes_depend_on_neither_max_batch_nor_company(model_sharp, mixed):
    from idfcodec.predict import PredictiveTileCodec
    a = PredictiveTileCodec(model_sharp, max_batch=2, colour=True).encode(mixed)
    b = PredictiveTileCodec(model_sharp, max_batch=256, colour=True).encode(mixed)
    assert a.to_bytes() == b.to_bytes()
    alone = PredictiveTileCodec(model_sharp, colour=True).encode([mixed[0]])
    n, P, Q = alone.n_entries, alone.n_packed, alone.n_colour
    assert alone.escaped.tolist() == b.escaped[:n].tolist()
    assert alone.packed.tolist() == b.packed[:n].tolist() and P > 0
    assert alone.colour.tolist() == b.colour[:n].tolist() and Q > 0
    assert np.array_equal(alone.sel, b.sel[:P]) and np.array_equal(alone.sel2, b.sel2[:Q])
    assert np.array_equal(alone.states, b.states[:P])
    assert np.array_equal(alone.nwords, b.nwords[:P])
    assert torch.equal(alone.words.cpu(), b.words[:int(alone.nwords.sum())].cpu())
    assert torch.equal(alone.raw.cpu(), b.raw[:alone.raw.numel()].cpu())


def test_a_pass_limit_splits_the_entries_without_changing_a_byte(model_far, monkeypatch):
    """SYMBOLS_PER_PASS counts both candidates: with room for one 16x16 entry's two streams a pass
    the 13 entries go through several passes and the file is the same."""
    from idfcodec import predict
    imgs, qc = _e2e(model_far)
    want = qc.encode(imgs).to_bytes()
    monkeypatch.setattr(predict, "SYMBOLS_PER_PASS", 2 * 768)
    assert qc.encode(imgs).to_bytes() == want
