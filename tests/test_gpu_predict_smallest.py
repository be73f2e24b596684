"""choose="smallest" on the device: idf_predict_cost_u8 against the numpy reference, integer for
integer and inside guard values; choose="escaped" byte for byte the default call; and
choose="smallest" on sets where every outcome occurs -- kept because the flow is smaller, moved to
the predictor although the keep rule keeps it (REASON_SMALLER), packed because the flow fails the
rule, raw -- with exact round trips, the size bound at every max_ratio, the shortlist on and off,
chunk sizes and company, the colour mode with interleaved streams, strided sources, and the count
of streams the predictor is handed.  Tiny models only."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

import predict_cost_ref as cref
from test_gpu_predict import SIZES, _planes_of, _smooth
from test_gpu_safe import _dev, _noise, _rows, _tiny_model

pytestmark = pytest.mark.gpu

KINDS = ("noise", "smooth", "dark")
GUARD64 = -0x5A5A5A5A5A5A5A5B
MEAN = 77           # the byte the flat model's priors sit on


def _content(kind, H, W, seed, C=3):
    if kind == "noise":
        return _noise(H, W, seed, C)
    if kind == "smooth":
        return _smooth(H, W, seed, C)
    return _noise(H, W, seed, C) % 4


# ------------------------------------------------------------------ 1. the cost kernel
@functools.lru_cache(maxsize=None)
def _cost_case(C, th, tw, kind):
    """The five images of SIZES in one content, their tiles' bytes in entry order and the
    reference's costs [n, 2] (the colour candidate where C >= 3).  Computed once and shared."""
    from idfcodec.tiled import TileLayout
    imgs = [_content(kind, H, W, 7 * i + len(kind), C) for i, (H, W) in enumerate(SIZES)]
    lay = TileLayout(SIZES, C, (th, tw))
    planes = _planes_of(imgs, lay)
    want = np.array([cref.costs(p, C >= 3) for p in planes], dtype=np.int64)
    return imgs, lay, want


@pytest.mark.parametrize("th,tw", [(16, 16), (12, 8)])
@pytest.mark.parametrize("C,colour", [(1, False), (3, False), (3, True), (4, False), (4, True)])
def test_cost_kernel_equals_the_reference_inside_guards(C, colour, th, tw):
    from idfcodec._lib import lib, ptr, stream_ptr
    for kind in KINDS:
        imgs, lay, want = _cost_case(C, th, tw, kind)
        if (th, tw) == (16, 16):
            # 13 tiles, with 1x1, 1x16, 5x5, 5x8 and 16x5 parts at origins that are not 0
            assert lay.n_tiles == 13
            assert {(1, 1), (1, 16), (5, 5), (5, 8), (16, 5), (16, 16)} <= set(lay.rects)
        src = [i.cuda() for i in imgs]
        rows, _ = _rows(src, th, tw)
        n, gap = len(rows), 16
        buf = torch.full((2 * n + 2 * gap,), GUARD64, dtype=torch.int64, device="cuda")
        out = buf[gap:gap + 2 * n]
        rc = lib().idf_predict_cost_u8(stream_ptr(out.device), n, C, th, tw,
                                       ptr(_dev(rows, torch.int64)), int(colour), ptr(out))
        assert rc == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n, 2)
        assert np.array_equal(got[:, 0], want[:, 0]), kind
        assert np.array_equal(got[:, 1], want[:, 1] if colour else np.zeros(n, np.int64)), kind
        assert bool((buf[:gap] == GUARD64).all()) and bool((buf[gap + 2 * n:] == GUARD64).all())


def test_cost_of_a_tile_outside_the_image_is_zero_and_colour_needs_three_planes():
    from idfcodec._lib import IdfError
    from idfcodec.predict import device_predict_cost
    img = _noise(16, 16, 3).cuda()
    rows = [[img.data_ptr(), 16, 16, -4, 0], [img.data_ptr(), 16, 16, 0, 0]]
    got = device_predict_cost(_dev(rows, torch.int64), 2, 3, 16, 16, True).cpu().numpy()
    assert got[0].tolist() == [0, 0]
    assert got[1].tolist() == cref.costs(img.cpu().numpy(), True)
    one = _noise(16, 16, 3, 1).cuda()
    table = _dev([[one.data_ptr(), 16, 16, 0, 0]], torch.int64)
    assert device_predict_cost(table, 1, 1, 16, 16).cpu().numpy()[0, 0] == \
        cref.cost_q8(one.cpu().numpy())
    for C in (1, 2):
        with pytest.raises(IdfError, match="IDF_ERR_ARG"):
            device_predict_cost(table, 1, C, 16, 16, True)
    with pytest.raises(ValueError, match="five fields"):
        device_predict_cost(torch.zeros((1, 8), dtype=torch.int64, device="cuda"), 1, 3, 16, 16)


# ------------------------------------------------------------------ 2. models and sets
@pytest.fixture(scope="module")
def model_sharp():
    """test_gpu_safe's: every prior's logscale lowered by 3.0, so dark tiles are kept."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            b["prior"].NN.layers[-1].bias[b["prior"].out_channel:] -= 3.0
    return m.cuda()


@pytest.fixture(scope="module")
def model_flat():
    """A 16x16 model whose flow wins on its own ground: every coupling's last layer zeroed (the
    latents are the dequantised pixels, moved about) and every prior's last layer a constant --
    mean MEAN / 256, scale 1/8 bin.  A byte at the mean then has frequency 0.964 * 2^24 (0.053
    bit), one a bin away 5.8 bits, one 3 or more bins away the window's floor, 24 bits."""
    m = _tiny_model(2, 2, 16, 16, 3, 2)
    with torch.no_grad():
        for b in m.blocks:
            for f in b["flows"]:
                if hasattr(f, "dense"):
                    f.dense.layers[-1].weight.zero_()
                    f.dense.layers[-1].bias.zero_()
            last, oc = b["prior"].NN.layers[-1], b["prior"].out_channel
            last.weight.zero_()
            last.bias[:oc] = MEAN / 256
            last.bias[oc:] = math.log(1 / 2048)
    return m.cuda()


def _const(H, W):
    return torch.full((3, H, W), MEAN, dtype=torch.uint8)


def _near(H, W, seed):
    """bytes MEAN - 1 .. MEAN + 1"""
    return (MEAN - 1 + _noise(H, W, seed) % 3).to(torch.uint8)


@pytest.fixture(scope="module")
def every_outcome():
    """A 32x48 image of six tiles -- constant, near, noise / dark, constant, near -- and four more
    images: constant 17x16, near 37x21, noise 5x40, constant 1x1.  6 + 2 + 6 + 3 + 1 tiles.

    What they cost on model_flat (bytes; flow = entry_bits / 8 at one way and predictor = 16 + 4 *
    nwords, both measured on an MI355X; the full tiles' figures were computed beforehand on the
    CPU with the oracle and tests/predict_ref.py and agree):
      constant 16x16x3: flow 24 (0.031 of 768), estimate 140 (0.182)       -> the flow, not coded
      near     16x16x3: flow 388-412 (0.51-0.54), predictor 248-252 (0.33) -> moved, REASON_SMALLER
      dark     16x16x3: flow 2328 (3.03: not eligible), predictor 308      -> packed
      noise    16x16x3: flow 2300 (2.99: not eligible), predictor 856      -> raw
      near 16x5, 5x16, 5x5: flow 356-432 of 240 / 75 bytes: not eligible, predictor 96-100 / 48
      constant 1x16x3:  flow 24 of 48 bytes, estimate 40                   -> the flow
      constant 1x1x3:   flow 24 of 3 bytes: not eligible, predictor 16     -> raw
    At ways = 8, predict_ways = 8 and colour: constant flow 136, estimate 188; near flow 484-496,
    predictor 288-300; the 1x16 constant strip (flow 136 of 48) and the 5x5 tile go raw."""
    top = torch.cat([_const(16, 16), _near(16, 16, 91), _noise(16, 16, 92)], dim=2)
    bottom = torch.cat([_noise(16, 16, 93) % 4, _const(16, 16), _near(16, 16, 94)], dim=2)
    return [t.contiguous().cuda() for t in (torch.cat([top, bottom], dim=1), _const(17, 16),
                                            _near(37, 21, 95), _noise(5, 40, 96), _const(1, 1))]


ALL_SIZES = [(32, 48), (17, 16), (37, 21), (5, 40), (1, 1)]


def _report(pbs, title):
    from idfcodec.predict import entry_bytes
    raw = entry_bytes(pbs.rects(), pbs.C)
    print(f"\n{title}: entry, rect, raw, flow bytes, est bytes, pred bytes, choice, reasons")
    for e, (r, n) in enumerate(zip(pbs.rects(), raw)):
        print(f"  {e:2d} {str(r):9s} {n:4d} {pbs.flow_bits[e] // 8:5d} {pbs.est_bytes[e]:5d} "
              f"{pbs.pred_bytes[e]:5d}  {'flow pred raw'.split()[pbs.choice[e]]:4s} "
              f"{pbs.reasons[e]}")


def _round_trip(pc, buf, imgs):
    from idfcodec.predict import PredictiveTiledBitstream
    got = PredictiveTiledBitstream.from_bytes(buf, device="cuda")
    assert got.to_bytes() == buf        # before the decode, which may hand got.stream a buffer
    outs, info = pc.decode(got)
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, imgs))
    return got, info


# ------------------------------------------------------------------ 3. choose="escaped"
def test_choose_escaped_is_the_default_call_byte_for_byte(model_sharp, every_outcome):
    for predict in (True, "colour"):
        pc = model_sharp.tiled_safe(predict=predict)
        a, b = pc.encode(every_outcome), pc.encode(every_outcome, choose="escaped")
        c = pc.encode(every_outcome, choose="escaped", shortlist=False)
        assert a.to_bytes() == b.to_bytes() == c.to_bytes()
        assert np.array_equal(a.reasons, b.reasons) and not (a.reasons & 8).any()
        assert (a.est_bytes == -1).all() and (a.pred_bytes[~a.escaped] == -1).all()
        assert (a.pred_bytes[a.escaped] > 0).all()
        # the safe codec's decision and inner stream, as before
        sbs = model_sharp.tiled_safe().encode(every_outcome)
        assert a.escaped.tolist() == sbs.escaped.tolist()
        assert np.array_equal(a.reasons, sbs.reasons)
        assert a.stream.to_bytes() == sbs.stream.to_bytes()
    with pytest.raises(ValueError, match="choose"):
        pc.encode(every_outcome, choose="smaller")


# ------------------------------------------------------------------ 4. choose="smallest"
def _flow_bytes_of_a_constant_tile(oracle):
    """entry_bits / 8 of a full constant tile on model_flat, from the CPU oracle: two levels of 384
    latents, all at the mean, scale 1/8 bin."""
    x = np.full(384, MEAN / 256, dtype=np.float32)
    s = np.full(384, np.float32(1 / 2048), dtype=np.float32)
    return 2 * (8 + 4 + 4 * len(oracle.encode(1 << 32, x, x, s)[1]))


def test_smallest_with_every_outcome(model_flat, every_outcome, oracle):
    from idfcodec.predict import (CHOICE_FLOW, CHOICE_PREDICT, CHOICE_RAW, entry_bytes,
                                  file_size_bound_packed)
    from idfcodec.safe import REASON_SIZE, REASON_SMALLER
    pc = model_flat.tiled_safe(predict=True)
    esc = pc.encode(every_outcome)
    pbs = pc.encode(every_outcome, choose="smallest")
    _report(esc, "choose='escaped'")
    _report(pbs, "choose='smallest'")
    raw = entry_bytes(pbs.rects(), 3)
    # image 0's six tiles: constant, near, noise / dark, constant, near
    assert pbs.choice[:6].tolist() == [CHOICE_FLOW, CHOICE_PREDICT, CHOICE_RAW,
                                       CHOICE_PREDICT, CHOICE_FLOW, CHOICE_PREDICT]
    assert pbs.reasons[:6].tolist() == [0, REASON_SMALLER, REASON_SIZE, REASON_SIZE, 0,
                                        REASON_SMALLER]
    assert esc.choice[:6].tolist() == [CHOICE_FLOW, CHOICE_FLOW, CHOICE_RAW, CHOICE_PREDICT,
                                       CHOICE_FLOW, CHOICE_FLOW]
    # the flow's cost of the constant tile is what the oracle says on the CPU
    assert pbs.flow_bits[0] // 8 == _flow_bytes_of_a_constant_tile(oracle) == pbs.flow_bits[4] // 8
    assert 8 * pbs.pred_bytes[1] < pbs.flow_bits[1] <= 8 * raw[1]       # moved although kept
    # every entry sits in its smallest coding, on the numbers the stream reports
    coded = pbs.pred_bytes >= 0
    el = (pbs.reasons & ~np.uint8(REASON_SMALLER)) == 0
    best = np.minimum(np.where(el, pbs.flow_bits // 8, raw),
                      np.where(coded, np.minimum(pbs.pred_bytes, raw), raw))
    cost = np.where(pbs.choice == CHOICE_FLOW, pbs.flow_bits // 8,
                    np.where(pbs.choice == CHOICE_PREDICT, pbs.pred_bytes, raw))
    assert (cost == best).all()
    # the file: an ordinary IDFP file, exact, smaller
    buf = pbs.to_bytes()
    assert buf[:4] == b"IDFP" and struct.unpack_from("<H", buf, 6)[0] == 0
    got, info = _round_trip(pc, buf, every_outcome)
    assert info["packed_tiles"] == pbs.n_packed and info["raw_tiles"] == int(pbs.stored_raw.sum())
    assert len(buf) < len(esc.to_bytes())
    saved = int(((esc.flow_bits // 8 - pbs.pred_bytes)[pbs.reasons == REASON_SMALLER]).sum())
    assert saved > 0 and len(esc.to_bytes()) - len(buf) >= saved - 2   # less a byte a bitmap
    # a crop over all six tiles of image 0 (flow, predictor and raw side by side), each clipped
    y0, x0, h, w = 10, 9, 15, 30
    crop, info = pc.decode_region(got, 0, y0, x0, h, w)
    assert info["ok"] and info["tiles"] == 6
    assert info["packed_tiles"] == 3 and info["raw_tiles"] == 1
    assert torch.equal(crop, every_outcome[0][:, y0:y0 + h, x0:x0 + w])
    # the shortlist changes nothing here: every estimate is more than a word from the flow's cost
    assert (np.abs(8 * pbs.est_bytes - pbs.flow_bits)[el] > 32).all()
    full = pc.encode(every_outcome, choose="smallest", shortlist=False)
    _report(full, "choose='smallest', shortlist=False")
    assert (full.pred_bytes >= 0).all() and not (pbs.pred_bytes >= 0).all()
    assert full.to_bytes() == buf
    assert np.array_equal(full.pred_bytes[coded], pbs.pred_bytes[coded])
    # the estimate is the coder's cost within a word (one way)
    assert set(((full.est_bytes - full.pred_bytes) // 4).tolist()) <= {0, 1}
    # every max_ratio: within the bound, exact; above 1 nothing changes, the flow never costs
    # more than the bytes
    bound = file_size_bound_packed(ALL_SIZES, 3, 16, 16, 2)
    for ratio in (0.5, 1.0, float("inf")):
        for shortlist in (True, False):
            p = pc.encode(every_outcome, max_ratio=ratio, choose="smallest", shortlist=shortlist)
            b = p.to_bytes()
            assert len(b) <= bound and len(b) <= len(pc.encode(every_outcome,
                                                              max_ratio=ratio).to_bytes())
            _round_trip(pc, b, every_outcome)
            if ratio >= 1:
                assert b == buf
            kept = p.choice == CHOICE_FLOW
            assert (p.flow_bits[kept] <= 8 * raw[kept] * min(ratio, 1.0)).all()
    # at inf the dark and noise tiles are eligible and leave the flow all the same
    p = pc.encode(every_outcome, max_ratio=float("inf"), choose="smallest")
    assert p.reasons[2] == p.reasons[3] == REASON_SMALLER
    assert p.choice[2] == CHOICE_RAW and p.choice[3] == CHOICE_PREDICT
    # at 0.5 the near tiles (0.531 through the flow) are not eligible: packed, not "smaller"
    p = pc.encode(every_outcome, max_ratio=0.5, choose="smallest")
    assert p.reasons[1] == REASON_SIZE and p.choice[1] == CHOICE_PREDICT


def test_check_decode_verifies_before_the_choice(model_flat, every_outcome):
    pc = model_flat.tiled_safe(predict=True)
    a = pc.encode(every_outcome, choose="smallest")
    b = pc.encode(every_outcome, choose="smallest", check="decode")
    assert a.to_bytes() == b.to_bytes() and np.array_equal(a.reasons, b.reasons)


def test_same_choices_for_every_max_batch_and_for_an_image_alone(model_flat, every_outcome):
    from idfcodec.predict import PredictiveTileCodec
    a = PredictiveTileCodec(model_flat, max_batch=4).encode(every_outcome, choose="smallest")
    b = PredictiveTileCodec(model_flat, max_batch=256).encode(every_outcome, choose="smallest")
    assert a.to_bytes() == b.to_bytes() and np.array_equal(a.reasons, b.reasons)
    for k in ("flow_bits", "est_bytes", "pred_bytes"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    alone = PredictiveTileCodec(model_flat).encode([every_outcome[0]], choose="smallest")
    n, P = alone.n_entries, alone.n_packed
    assert n == 6 and alone.choice.tolist() == b.choice[:n].tolist() and P == 3
    assert np.array_equal(alone.reasons, b.reasons[:n])
    assert np.array_equal(alone.sel, b.sel[:P]) and np.array_equal(alone.states, b.states[:P])
    assert np.array_equal(alone.nwords, b.nwords[:P])
    assert torch.equal(alone.words.cpu(), b.words[:int(alone.nwords.sum())].cpu())
    assert torch.equal(alone.raw.cpu(), b.raw[:alone.raw.numel()].cpu())
    for k in ("flow_bits", "est_bytes", "pred_bytes"):
        assert np.array_equal(getattr(alone, k), getattr(b, k)[:n]), k


def test_smallest_in_colour_mode_with_interleaved_streams(model_flat, every_outcome):
    """predict="colour", predict_ways=8, ways=8: an IDFQ file whose header names 8 ways; the
    flow's entries cost 2 * (64 + 4 + 4 nw) bytes, a packed entry 72 (76) + 4 nw."""
    from idfcodec.predict import (CHOICE_FLOW, CHOICE_PREDICT, CHOICE_RAW, entry_bytes,
                                  file_size_bound_packed)
    from idfcodec.safe import REASON_SMALLER
    pc = model_flat.tiled_safe(ways=8, predict="colour", predict_ways=8)
    esc = pc.encode(every_outcome)
    pbs = pc.encode(every_outcome, choose="smallest")
    _report(pbs, "colour, predict_ways 8, ways 8: choose='smallest'")
    raw = entry_bytes(pbs.rects(), 3)
    assert set(pbs.choice.tolist()) == {CHOICE_FLOW, CHOICE_PREDICT, CHOICE_RAW}
    assert (pbs.reasons == REASON_SMALLER).any()
    assert pbs.choice[0] == CHOICE_FLOW and pbs.choice[1] == CHOICE_PREDICT
    assert 2 * (64 + 4) <= pbs.flow_bits[0] // 8 < 160 and pbs.pred_bytes[0] == -1
    buf = pbs.to_bytes()
    assert buf[:4] == b"IDFQ" and struct.unpack_from("<H", buf, 6)[0] == 8
    got, info = _round_trip(pc, buf, every_outcome)
    assert info["packed_tiles"] == pbs.n_packed
    assert len(buf) < len(esc.to_bytes())
    for ratio in (0.5, 1.0, float("inf")):
        b = pc.encode(every_outcome, max_ratio=ratio, choose="smallest").to_bytes()
        assert len(b) <= file_size_bound_packed(ALL_SIZES, 3, 16, 16, 2, colour=True)
    full = pc.encode(every_outcome, choose="smallest", shortlist=False)
    _report(full, "colour, predict_ways 8, ways 8: shortlist=False")
    assert len(full.to_bytes()) <= len(buf)
    cost = np.where(full.choice == CHOICE_FLOW, full.flow_bits // 8,
                    np.where(full.choice == CHOICE_PREDICT, full.pred_bytes, raw))
    assert (cost <= raw).all()
    # the estimate's gap to the coder at eight ways: printed, not asserted
    print("  est - pred bytes per entry:", (full.est_bytes - full.pred_bytes).tolist())
    y0, x0, h, w = 10, 9, 15, 30
    crop, info = pc.decode_region(got, 0, y0, x0, h, w)
    assert info["ok"] and torch.equal(crop, every_outcome[0][:, y0:y0 + h, x0:x0 + w])


def test_a_shortlisted_out_tile_is_not_coded(model_flat, monkeypatch):
    """On constant images at the mean every entry is eligible and the flow's 24 bytes are below
    every estimate: the predictor is handed no stream with the shortlist and all N without it."""
    from idfcodec.predict import CHOICE_FLOW, PredictiveTileCodec
    sizes = [(16, 16), (17, 16), (5, 40), (37, 21)]
    imgs = [_const(H, W).cuda() for H, W in sizes]
    pc = model_flat.tiled_safe(predict=True)
    handed = []
    inner = PredictiveTileCodec._predict_coded

    def counting(self, rows, rects, dev):
        handed.append(len(rows))
        return inner(self, rows, rects, dev)

    monkeypatch.setattr(PredictiveTileCodec, "_predict_coded", counting)
    a = pc.encode(imgs, choose="smallest")
    assert sum(handed) == 0 and (a.choice == CHOICE_FLOW).all() and (a.pred_bytes == -1).all()
    assert (a.est_bytes > a.flow_bits // 8).all()
    del handed[:]
    b = pc.encode(imgs, choose="smallest", shortlist=False)
    assert sum(handed) == a.n_entries == 12 and (b.pred_bytes > b.flow_bits // 8).all()
    assert b.to_bytes() == a.to_bytes()
    _round_trip(pc, a.to_bytes(), imgs)


def test_sharp_model_moves_its_dark_tiles_to_the_predictor(model_sharp):
    """test_gpu_safe's model_sharp keeps a full dark tile at 0.797 of its bytes; the predictor
    codes it in 0.38.  choose="smallest" moves every such tile and stores the noise raw."""
    from idfcodec.predict import CHOICE_PREDICT, CHOICE_RAW
    from idfcodec.safe import REASON_SMALLER
    dark = lambda H, W, s: _noise(H, W, s) % 4  # noqa: E731
    imgs = [t.cuda() for t in (dark(32, 32, 80), _noise(16, 16, 81), dark(17, 16, 82),
                               _noise(37, 21, 83), dark(5, 40, 84))]
    pc = model_sharp.tiled_safe(predict=True)
    esc = pc.encode(imgs)
    pbs = pc.encode(imgs, choose="smallest")
    _report(pbs, "model_sharp, dark and noise")
    assert esc.n_kept >= 4 and (esc.reasons[:4] == 0).all()
    assert (pbs.reasons[:4] == REASON_SMALLER).all() and (pbs.choice[:4] == CHOICE_PREDICT).all()
    assert pbs.choice[4] == CHOICE_RAW
    assert 0.75 < pbs.flow_bits[0] / (8 * 768) < 0.85 and 0.36 < pbs.pred_bytes[0] / 768 < 0.40
    assert len(pbs.to_bytes()) < len(esc.to_bytes())
    _round_trip(pc, pbs.to_bytes(), imgs)
    full = pc.encode(imgs, choose="smallest", shortlist=False)
    assert len(full.to_bytes()) <= len(pbs.to_bytes())


def test_strided_sources_are_staged_once_and_code_the_same_bytes(model_flat, every_outcome,
                                                                 monkeypatch):
    """layout="hwc": the entries are copied into the raw layout once, for the cost kernel and for
    the coding, and the file is the planar sources' file."""
    from idfcodec import predict
    pc = model_flat.tiled_safe(predict=True)
    want = pc.encode(every_outcome, choose="smallest").to_bytes()
    hwc = [i.permute(1, 2, 0).contiguous() for i in every_outcome]
    calls = []
    gather = predict.device_gather_raw

    def counting(table, n, *a):
        calls.append((n, table.shape[1]))
        return gather(table, n, *a)

    monkeypatch.setattr(predict, "device_gather_raw", counting)
    got = pc.encode(hwc, layout="hwc", choose="smallest")
    assert got.to_bytes() == want
    assert calls == [(18, 8)]       # every entry once; the raw bytes are gathered by safe.py's
    outs, info = pc.decode(got, layout="hwc")
    assert info["ok"] and all(torch.equal(a, b) for a, b in zip(outs, hwc))
