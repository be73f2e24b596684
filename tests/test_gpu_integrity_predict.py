"""Sealed predictive tiled files on the device: IDFC around IDFP and IDFQ.  Round trips whose
inner bytes are the unsealed codec's and whose CRCs are zlib's (tests/crc_ref.py); a file whose
tiles lie in all three codings -- flow, predictor, raw -- with one tile of each kind damaged in
its contents and named by its entry, alone and together; parts of a file; strided sources and
destinations; the model check, the pairing of codec and inner file, and the caches of
tiled_safe(seal=True).  Damage touches contents only (stored bytes, words, a state, a recorded
CRC), never a length, a count or an offset.  Tiny models only."""
import numpy as np
import pytest
import torch

import colour_ref as cref
import crc_ref
from test_gpu_predict import model_far  # noqa: F401 (fixture)
from test_gpu_predict_smallest import every_outcome, model_flat, model_sharp  # noqa: F401
from test_gpu_strided import _guards_intact, _views

pytestmark = pytest.mark.gpu

N = 18              # every_outcome: 6 + 2 + 6 + 3 + 1 tiles of 16x16
FLOW, PREDICT, RAW = 0, 1, 2


def _u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


@pytest.fixture(scope="module")
def crcs(every_outcome):  # noqa: F811
    """zlib's CRC-32 of every tile's source bytes: computed once, shared, never changed"""
    return crc_ref.tile_crcs([t.cpu().numpy() for t in every_outcome], 16, 16)


def _differing(outs, imgs):
    """The entries whose returned bytes are not the source's, compared on the host."""
    from idfcodec.tiled import tiles_host
    same = []
    for o, i in zip(outs, imgs):
        same += [np.array_equal(a, b) for a, b in zip(tiles_host(o.cpu().numpy(), 16, 16),
                                                      tiles_host(i.cpu().numpy(), 16, 16))]
    return [e for e, s in enumerate(same) if not s]


# ------------------------------------------------------------------ 1. round trips
CASES = [(p, w, c, None) for p in (True, "colour") for w in (1, 8)
         for c in ("escaped", "smallest")] + [(True, 1, "smallest", 2)]


def _sealed_codec(model, predict, ways, mb):
    """tiled_safe(seal=True); mb: a SealedCodec built by hand around a codec of that max_batch"""
    from idfcodec.integrity import SealedCodec
    from idfcodec.predict import PredictiveTileCodec
    if mb is None:
        return model.tiled_safe(predict=predict, predict_ways=ways, seal=True)
    return SealedCodec(PredictiveTileCodec(model, max_batch=mb, colour=predict == "colour",
                                           predict_ways=ways))


@pytest.mark.parametrize("predict,ways,choose,mb", CASES)
def test_sealed_predictive_round_trip(model_flat, every_outcome, crcs, predict, ways,  # noqa: F811
                                      choose, mb):
    from idfcodec.integrity import SealedBitstream, SealedCodec
    from idfcodec.predict import PredictiveTiledBitstream
    zc = _sealed_codec(model_flat, predict, ways, mb)
    pc = zc.codec
    assert type(zc) is SealedCodec and pc.predict_ways == ways
    if mb is None:
        assert pc is model_flat.tiled_safe(predict=predict, predict_ways=ways)
    zbs = zc.encode(every_outcome, choose=choose)
    plain = pc.encode(every_outcome, choose=choose)
    want = plain.to_bytes()
    assert type(zbs.inner) is PredictiveTiledBitstream and zbs.inner.to_bytes() == want
    assert want[:4] == (b"IDFQ" if predict == "colour" else b"IDFP")
    assert zbs.crc.dtype == np.uint32 and zbs.crc.tolist() == crcs
    buf = zbs.to_bytes()
    assert len(buf) == len(want) + 28 + 4 * N
    back = SealedBitstream.from_bytes(buf, device="cuda")
    assert back.to_bytes() == buf
    if (predict, ways, choose) == (True, 1, "smallest"):
        # image 0's six tiles lie in all three codings: the three check paths all run
        assert back.inner.choice[:6].tolist() == [FLOW, PREDICT, RAW, PREDICT, FLOW, PREDICT]
    if mb == 2:
        assert back.inner.n_kept > 2        # the kept tiles span several chunks
    outs, info = zc.decode(back)
    assert info["crc_bad"] == [] and info["ok"] is True
    assert all(torch.equal(a, b) for a, b in zip(outs, every_outcome))
    _, pinfo = pc.decode(plain)
    assert pinfo["ok"] is True
    for k in ("tiles", "raw_tiles", "packed_tiles", "colour_tiles"):
        assert info[k] == pinfo[k], k
    assert info["tiles"] == N and info["packed_tiles"] == back.inner.n_packed > 0
    assert set(pinfo) | {"crc_bad"} == set(info)
    assert torch.equal(info["packed_final_states"], pinfo["packed_final_states"])
    assert info["packed_final_states"].numel() == back.inner.n_packed * ways
    assert torch.equal(info["packed_status"], pinfo["packed_status"])


# ------------------------------------------------------------------ 2. damage
_FILES = {}


def _file(model, imgs, predict=True, ways=1, choose="smallest"):
    """(the sealed codec, the file's bytes): encoded once per kind and shared; every test reads
    its own bitstream from the bytes and damages that."""
    key = (id(model), predict, ways, choose)
    if key not in _FILES:
        zc = model.tiled_safe(predict=predict, predict_ways=ways, seal=True)
        _FILES[key] = zc.encode(imgs, choose=choose).to_bytes()
    return model.tiled_safe(predict=predict, predict_ways=ways, seal=True), _FILES[key]


def _read(buf):
    from idfcodec.integrity import SealedBitstream
    return SealedBitstream.from_bytes(buf, device="cuda")


def _damage_raw(zbs, e):
    """one flipped bit of a stored byte of raw entry e"""
    from idfcodec.safe import raw_offsets
    inner = zbs.inner
    assert inner.stored_raw[e]
    offs, _ = raw_offsets(inner.stored_raw, inner.rects(), inner.C)
    h, w = inner.rects()[e]
    inner.raw[offs[e] + (inner.C * h * w) // 2] ^= 0x20


def _damage_packed(zbs, e):
    """One flipped bit in the words of packed entry e's stream, found through nwords and
    packed_index.  The word is the middle one of the stream: the decoder reads the words from
    the last to the first, so hundreds of symbols follow it and the decoded bytes change (a flip
    in one of the first words pushed is met by the last few symbols only, which may decode to the
    same bytes and leave just a final state that is not L)."""
    from idfcodec.predict import packed_index
    inner = zbs.inner
    p = packed_index(inner.escaped, inner.packed)[e]
    assert p >= 0
    nw = np.asarray(inner.nwords, dtype=np.int64)
    assert nw[p] >= 8
    at = int(nw[:p].sum() + nw[p] // 2)
    inner.words[at] ^= 0x00010000


def _damage_kept(zbs, e):
    """The contents of kept entry e's flow stream, level 0.  test_gpu_integrity flips a word of a
    coded tile; the tiles this file keeps are constant ones whose streams hold no word at all
    (their 24 bytes are two states and two zero counts: test_gpu_predict_smallest), so the bit
    flipped is one of the state, the stream's whole content.  Bit 40 lies above the 24 bits that
    choose the first symbol and scrambles every later one; the state stays above 2^32."""
    from idfcodec.safe import inner_index
    inner = zbs.inner
    k = inner_index(inner.escaped)[e]
    assert k >= 0
    s = inner.stream
    if int(s.nwords_host()[k]) > 4:      # a stream with words: test_gpu_integrity's damage
        at = int(s.word_offsets()[k].item()) + 2
        s.words[at] = s.words[at] ^ 0x00010000
    else:
        s.states[k * s.ways] ^= 1 << 40


def _decode_damaged(zc, zbs, imgs, bad):
    outs, info = zc.decode(zbs)
    print("damaged", bad, "crc_bad", info["crc_bad"], "differing", _differing(outs, imgs),
          "ok", info["ok"])
    assert info["crc_bad"] == bad and info["ok"] is False
    # every other tile's bytes are the source's, and exactly the named ones differ
    assert _differing(outs, imgs) == bad
    return info


def test_each_kind_of_damaged_tile_is_named(model_flat, every_outcome):  # noqa: F811
    zc, buf = _file(model_flat, every_outcome)
    assert _read(buf).inner.choice[:3].tolist() == [FLOW, PREDICT, RAW]
    for e, damage in ((2, _damage_raw), (1, _damage_packed), (0, _damage_kept)):
        zbs = _read(buf)
        damage(zbs, e)
        info = _decode_damaged(zc, zbs, every_outcome, [e])
        assert info["tiles"] == N
    zbs = _read(buf)
    _damage_raw(zbs, 2)
    _damage_packed(zbs, 1)
    _damage_kept(zbs, 0)
    _decode_damaged(zc, zbs, every_outcome, [0, 1, 2])


def test_a_flipped_recorded_crc_names_its_entry(model_flat, every_outcome):  # noqa: F811
    zc, buf = _file(model_flat, every_outcome)
    zbs = _read(buf)
    zbs.crc[5] ^= 1
    outs, info = zc.decode(zbs)
    assert info["crc_bad"] == [5] and info["ok"] is False
    assert all(torch.equal(a, b) for a, b in zip(outs, every_outcome))     # its bytes are right


def test_a_damaged_colour_entry_at_eight_ways_is_named(model_far):  # noqa: F811
    """The packed case on a colour entry of interleaved streams: correlated planes, which the
    colour mode codes smaller, under a model that keeps nothing."""
    imgs = [torch.from_numpy(cref.correlated(H, W, 50 + i)).cuda()
            for i, (H, W) in enumerate(((32, 48), (17, 16), (37, 21)))]
    zc, buf = _file(model_far, imgs, predict="colour", ways=8)
    zbs = _read(buf)
    inner = zbs.inner
    assert buf[28 + 4 * inner.n_entries:][:4] == b"IDFQ" and inner.predict_ways == 8
    assert zbs.crc.tolist() == crc_ref.tile_crcs([t.cpu().numpy() for t in imgs], 16, 16)
    outs, info = zc.decode(zbs)
    assert info["crc_bad"] == [] and info["ok"] is True and info["colour_tiles"] > 0
    assert all(torch.equal(a, b) for a, b in zip(outs, imgs))
    e = int(np.flatnonzero(inner.colour)[0])
    _damage_packed(zbs, e)
    _decode_damaged(zc, zbs, imgs, [e])


# ------------------------------------------------------------------ 3. parts of a file
def test_parts_of_a_file_report_the_files_entries(model_flat, every_outcome, crcs):  # noqa: F811
    zc, buf = _file(model_flat, every_outcome)
    zbs = _read(buf)
    assert zbs.inner.packed[5]
    _damage_packed(zbs, 5)
    outs, info = zc.decode(zbs, images=[2, 0])
    assert info["crc_bad"] == [5] and info["ok"] is False and info["tiles"] == 12
    assert torch.equal(outs[0], every_outcome[2])
    assert _differing([outs[1]], [every_outcome[0]]) == [5]
    # tiles (0, 0) and (0, 1) of image 0: entries 0 and 1, a kept and a packed one
    crop, info = zc.decode_region(zbs, 0, 0, 0, 16, 32)
    assert info["crc_bad"] == [] and info["ok"] is True and info["tiles"] == 2
    assert info["packed_tiles"] == 1 and info["raw_tiles"] == 0
    assert torch.equal(crop, every_outcome[0][:, :16, :32])
    # all six tiles of image 0, each clipped
    y0, x0, h, w = 10, 9, 15, 30
    crop, info = zc.decode_region(zbs, 0, y0, x0, h, w)
    assert info["crc_bad"] == [5] and info["ok"] is False and info["tiles"] == 6
    want = every_outcome[0][:, y0:y0 + h, x0:x0 + w]
    assert torch.equal(crop[:, :, :32 - x0], want[:, :, :32 - x0])         # left of entry 5
    assert torch.equal(crop[:, :16 - y0], want[:, :16 - y0])               # above it
    # verify=False on the sound file: the sums stay on the device, in the call's order
    zbs = _read(buf)
    outs, info = zc.decode(zbs, images=[2, 0], verify=False)
    assert "ok" not in info and "crc_bad" not in info
    assert info["crc"].is_cuda and info["crc"].dtype == torch.int32
    assert info["crc_entries"] == [*range(8, 14), *range(6)]
    assert _u32(info["crc"]) == zbs.crc[info["crc_entries"]].tolist()
    assert _u32(info["crc"]) == [crcs[e] for e in info["crc_entries"]]
    assert torch.equal(outs[0], every_outcome[2]) and torch.equal(outs[1], every_outcome[0])
    crop, info = zc.decode_region(zbs, 0, y0, x0, h, w, verify=False)
    assert info["crc_entries"] == list(range(6))
    assert _u32(info["crc"]) == crcs[:6] and torch.equal(crop, want)


# ------------------------------------------------------------------ 4. layouts
def test_strided_sources_write_the_same_sealed_bytes(model_flat, every_outcome):  # noqa: F811
    zc, want = _file(model_flat, every_outcome)
    host = [t.cpu() for t in every_outcome]
    for kind in ("hwc", "hwc_pitch", "window"):
        big, tensors, layout, views = _views(kind, host)
        assert zc.encode(tensors, layout=layout, choose="smallest").to_bytes() == want, kind
        assert _guards_intact(big, views, host), kind       # a source is only read
    zbs = _read(want)
    outs, info = zc.decode(zbs, layout="hwc")
    assert info["crc_bad"] == [] and info["ok"] is True
    assert all(torch.equal(o.cpu(), t.permute(1, 2, 0)) for o, t in zip(outs, host))
    # into the caller's rows of W * C + 5 bytes
    big, tensors, layout, views = _views("hwc_pitch", host, fill=False)
    assert layout == "hwc"
    outs, info = zc.decode(zbs, layout="hwc", out=tensors)
    assert info["crc_bad"] == [] and info["ok"] is True
    assert all(a is b for a, b in zip(outs, tensors)) and _guards_intact(big, views, host)


# ------------------------------------------------------------------ 5. model and pairing
def test_another_model_is_refused_and_a_file_that_keeps_nothing_needs_no_weight(
        model_flat, model_far, every_outcome, monkeypatch):  # noqa: F811
    from idfcodec.integrity import model_fingerprint
    zc, buf = _file(model_flat, every_outcome)
    zbs = _read(buf)
    fp, fp_far = model_fingerprint(model_flat), model_fingerprint(model_far)
    assert zbs.fingerprint == fp != fp_far
    zfar = model_far.tiled_safe(predict=True, seal=True)
    with pytest.raises(ValueError) as err:
        zfar.decode(zbs)
    assert f"{fp:#010x}" in str(err.value) and f"{fp_far:#010x}" in str(err.value)
    # model_far keeps nothing: every tile is the predictor's or raw
    _, far_buf = _file(model_far, every_outcome, choose="escaped")
    far = _read(far_buf)
    assert far.inner.n_kept == 0 and far.inner.n_packed > 0 and far.inner.stored_raw.any()
    assert far.fingerprint == fp_far

    def no_decode(*a, **k):
        raise AssertionError("decoded a file of another model")
    monkeypatch.setattr(zc.codec, "_decode_entries", no_decode)
    with pytest.raises(ValueError, match="fingerprint"):    # refused before anything decodes
        zc.decode(far)
    with pytest.raises(ValueError, match="fingerprint"):
        zc.decode_region(far, 0, 0, 0, 4, 4)
    monkeypatch.undo()
    outs, info = zc.decode(far, check_model=False)
    assert info["crc_bad"] == [] and info["ok"] is True
    assert info["final_states"].numel() == 0                # no flow ran
    assert all(torch.equal(a, b) for a, b in zip(outs, every_outcome))


def test_codec_and_inner_file_pair_by_exact_kind(model_flat, every_outcome):  # noqa: F811
    from idfcodec.integrity import SealedBitstream
    zp, buf = _file(model_flat, every_outcome)
    zs = model_flat.tiled_sealed()
    idfs = SealedBitstream.from_bytes(zs.encode(every_outcome).to_bytes(), device="cuda")
    with pytest.raises(ValueError, match="SafeTiledBitstream.*PredictiveTileCodec"):
        zp.decode(idfs)
    with pytest.raises(ValueError, match="PredictiveTiledBitstream.*SafeTiledCodec"):
        zs.decode(_read(buf))
    with pytest.raises(ValueError, match="PredictiveTiledBitstream.*TiledCodec"):
        model_flat.tiled_sealed(safe=False).decode(_read(buf))
    # an IDFQ file goes through the IDFP codec's seal, as the unsealed codec reads both
    _, qbuf = _file(model_flat, every_outcome, predict="colour", ways=8)
    assert qbuf[28 + 4 * N:][:4] == b"IDFQ"
    outs, info = zp.decode(_read(qbuf))
    assert info["crc_bad"] == [] and info["ok"] is True
    assert all(torch.equal(a, b) for a, b in zip(outs, every_outcome))


def test_tiled_safe_seal_is_cached_beside_the_other_codecs(model_sharp):  # noqa: F811
    from idfcodec.integrity import SealedCodec
    m = model_sharp
    before = (m.tiled_sealed(), m.tiled(), m.tiled_safe(), m.tiled_safe(predict=True),
              m.tiled_safe(predict="colour"))
    z = m.tiled_safe(predict=True, seal=True)
    assert type(z) is SealedCodec and m.tiled_safe(predict=True, seal=True) is z
    assert z.codec is m.tiled_safe(predict=True)
    zq = m.tiled_safe(predict="colour", seal=True)
    assert zq is not z and zq.codec is m.tiled_safe(predict="colour")
    assert m.tiled_safe(predict=True, seal=True) is z       # the two kinds do not evict each other
    assert m.tiled_safe(seal=True) is m.tiled_sealed() is before[0]
    after = (m.tiled_sealed(), m.tiled(), m.tiled_safe(), m.tiled_safe(predict=True),
             m.tiled_safe(predict="colour"))
    assert all(a is b for a, b in zip(before, after))
    # another predict_ways is another codec, and its seal wraps that one
    z8 = m.tiled_safe(predict=True, predict_ways=8, seal=True)
    assert z8 is not z and z8.codec.predict_ways == 8
    assert z8.codec is m.tiled_safe(predict=True, predict_ways=8)
    with pytest.raises(ValueError, match="predict_ways"):
        m.tiled_safe(predict_ways=8, seal=True)
