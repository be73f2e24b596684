"""The 8-bit predictive coder's kernels at the tile the product uses, 64 x 64, and at their
limits; every comparison is bit for bit against predict_ref, colour_ref, predict_ways_ref,
rans_oracle, rans_ways_ref, predict_cost_ref, zlib and numpy (tests/predict_cases.py holds the
cases and tests/test_predict_cases_host.py shows what they reach).

64 x 64, C in {1, 3, 4}, images 64x64, 65x64, 64x65 and 69x69 of zeros, ramp, vstep and noise
(rectangles: a full tile, 1x64, 64x1, 5x5, 64x5, 5x64): the preps inside guard values, the
streams word for word, the decoders on the reference's words and on the device's own inside guard
bytes -- one way and N ways, plain and colour entries mixed; the raw copies, the verify kernel
with a changed byte in each of the four 1024-pixel blocks of a tile, the tile CRCs and the cost
kernel.  Kernel-level tiles that are no model's: (2, 70, 130) with win > N at N = 64, (1, 3, 200),
(4, 120, 126) at the N-way decoder's LDS limit, (1, 1, 32768) at the one-way decoder's LDS row and
(4, 1, 15000); one past each limit is IDF_ERR_UNSUPPORTED before any launch.  End to end without
a flow: grey and grey + alpha sources through tiled_planes of a tiny 3 x 64 x 64 model."""
import zlib

import numpy as np
import pytest
import torch

import crc_ref
import predict_cases as pc
import predict_cost_ref as costref
import predict_ref as ref
import predict_ways_ref as wref
from test_gpu_predict import FGUARD
from test_gpu_safe import GUARD, _dev, _guarded, _guards_intact, _rows, _tiny_model

pytestmark = pytest.mark.gpu

L = ref.L
TH, TW = pc.TILE64
SELGUARD = 0x5A5A5A5A
GUARD64 = -0x0123456789ABCDEF
# (C, N, both candidates): prep_u8 at every C; prep_ways at N = 8, 64 at every C and 16, 32 at
# C = 3; prep2 and prep2_ways at C = 3, 4
CONFIGS = [(C, 1, False) for C in (1, 3, 4)] + \
          [(C, N, False) for C in (1, 3, 4) for N in (8, 64)] + [(3, 16, False), (3, 32, False)] + \
          [(C, N, True) for C in (3, 4) for N in (1, 8, 64)]
IDS = [f"C{C}-N{N}-{'both' if two else 'plain'}" for C, N, two in CONFIGS]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def _decode(planes, C, th, tw, N, words, w_off, nw, states, sel, sel2=None, col=None):
    """Every entry decoded into guarded bytes, the outputs handed out in reverse order with 5
    unused bytes between two: idf_predict_decode_u8 / decode2 at N = 1, decode_ways else.
    -> (the guards and bytes are exact, final uint64 [n, N], status)."""
    from idfcodec.predict import (device_predict_decode, device_predict_decode2,
                                  device_predict_decode_ways)
    n = len(planes)
    offs, total = pc.reverse_layout([p.size for p in planes])
    want = np.full(total, GUARD, dtype=np.uint8)
    for e, p in enumerate(planes):
        want[offs[e]:offs[e] + p.size] = p.reshape(-1)
    big, (out,) = _guarded([(total,)])
    final = torch.zeros(n * N, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    words = np.concatenate([np.asarray(words, dtype=np.uint32), np.zeros(1, np.uint32)])
    head = (_i32(words), _dev(w_off[:n], torch.int64), _dev(nw, torch.int64), _i64(states),
            _i32(np.asarray(sel, dtype=np.uint32)))
    tail = (_dev([p.shape[1:] for p in planes], torch.int32), _dev(offs, torch.int64), out, final,
            status)
    nc = 0 if col is None else int(np.count_nonzero(col))
    colour = (_i32(np.asarray(sel2, dtype=np.uint32)),
              torch.from_numpy(np.asarray(col, dtype=np.uint8)).cuda(), nc) if nc else \
        (None, None, 0)
    if N > 1:
        device_predict_decode_ways(n, N, C, th, tw, *head, *colour, *tail)
    elif nc:
        device_predict_decode2(n, C, th, tw, *head, *colour, *tail)
    else:
        device_predict_decode(n, C, th, tw, *head, *tail)
    torch.cuda.synchronize()
    return (_guards_intact(big, [out], [want]),
            final.cpu().numpy().view(np.uint64).reshape(n, N), status.cpu().numpy())


def _exact(run):
    ok, final, status = run
    return ok and bool((final == L).all()) and not status.any()


# ------------------------------------------------------------------ 1. 64 x 64: prep, code, decode
@pytest.mark.parametrize("C,N,two", CONFIGS, ids=IDS)
def test_64x64_prep_streams_and_decode_equal_the_references(C, N, two):
    from idfcodec.predict import (device_predict_encode, device_predict_encode2,
                                  device_predict_prep, device_predict_prep2)
    case, coded = pc.case64(C), pc.coded64(C, N, two)
    planes, n = case["planes"], len(case["planes"])
    src = [torch.from_numpy(i).cuda() for i in case["imgs"]]
    rows, _ = _rows(src, TH, TW)
    table = _dev(rows, torch.int64)
    # the prep inside guard values
    nsym, gap, k = int(coded["off"][-1]), 64, 3 if two else 1
    bufs = [torch.full((nsym + 2 * gap,), FGUARD, dtype=torch.float32, device="cuda")
            for _ in range(3)]
    x, mean, scale = (b[gap:gap + nsym] for b in bufs)
    selbuf = torch.full((k * n + 2 * gap,), SELGUARD, dtype=torch.int32, device="cuda")
    sel = selbuf[gap:gap + k * n]
    prep = device_predict_prep2 if two else device_predict_prep
    prep(table, n, C, TH, TW, _dev(coded["off"], torch.int64), sel, x, mean, scale, ways=N)
    torch.cuda.synchronize()
    assert np.array_equal(sel.cpu().numpy().view(np.uint32).reshape(coded["sel"].shape),
                          coded["sel"])
    for got, want in zip((x, mean, scale), (coded["x"], coded["mean"], coded["scale"])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for b in bufs:
        assert bool((b[:gap] == FGUARD).all()) and bool((b[gap + nsym:] == FGUARD).all())
    assert bool((selbuf[:gap] == SELGUARD).all()) and bool((selbuf[gap + k * n:] == SELGUARD).all())
    # the streams word for word
    if two:
        dsel, states, nw, status, words = device_predict_encode2(table, case["counts"], C, TH, TW,
                                                                 ways=N)
    else:
        dsel, states, nw, status, words = device_predict_encode(table, case["counts"], C, TH, TW, N)
    assert not status.any() and np.array_equal(dsel, coded["sel"])
    assert np.array_equal(nw, coded["nw"])
    assert np.array_equal(np.asarray(states).reshape(-1, N), coded["states"])
    dwords = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(dwords, coded["words"])
    # decode of the reference's words and of the device's own: every state L, every status 0
    if two:   # even entries from their colour stream, odd ones from their plain stream
        col = np.arange(n) % 2 == 0
        pick = 2 * np.arange(n) + col
        s1 = np.where(col, coded["sel"][:, 1], coded["sel"][:, 0])
        arg = lambda st: (coded["w_off"][pick], coded["nw"][pick], st[pick], s1,  # noqa: E731
                          coded["sel"][:, 2], col)
    else:
        arg = lambda st: (coded["w_off"], coded["nw"], st, coded["sel"])  # noqa: E731
    assert _exact(_decode(planes, C, TH, TW, N, coded["words"], *arg(coded["states"])))
    assert _exact(_decode(planes, C, TH, TW, N, dwords,
                          *arg(np.asarray(states).reshape(-1, N))))


# ------------------------------------------------------------------ 2. tiles that are no model's
BIG = [(kind, C, th, tw, N) for kind, C, th, tw, Ns, _ in pc.big_units() for N in Ns]


@pytest.mark.parametrize("kind,C,th,tw,N", BIG, ids=[f"{C}x{th}x{tw}-N{N}" for _, C, th, tw, N
                                                      in BIG])
def test_kernel_level_tiles_at_the_limits(kind, C, th, tw, N):
    from idfcodec.predict import device_predict_encode
    planes = next(ps for k, c, h, w, _, ps in pc.big_units() if (k, c, h, w) == (kind, C, th, tw))
    coded = [pc.encode(p, N) for p in planes]
    src = [torch.from_numpy(p).cuda() for p in planes]
    rows, _ = _rows(src, th, tw)
    assert len(rows) == len(planes)                        # one entry an image
    counts = [p.size for p in planes]
    sel, states, nw, status, words = device_predict_encode(_dev(rows, torch.int64), counts, C, th,
                                                           tw, N)
    assert not status.any() and sel.tolist() == [c.sel for c in coded]
    assert nw.tolist() == [len(c.words) for c in coded]
    want_states = np.array([c.states for c in coded], dtype=np.uint64)
    assert np.array_equal(np.asarray(states).reshape(-1, N), want_states)
    want_words = np.concatenate([c.words for c in coded])
    dwords = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(dwords, want_words)
    w_off = np.concatenate([[0], np.cumsum(nw)])
    assert _exact(_decode(planes, C, th, tw, N, want_words, w_off, nw, want_states, sel))
    assert _exact(_decode(planes, C, th, tw, N, dwords, w_off, nw,
                          np.asarray(states).reshape(-1, N), sel))


def test_one_past_each_limit_is_unsupported_before_any_launch():
    from idfcodec._lib import lib, ptr, stream_ptr
    big, (out,) = _guarded([(64,)])
    final = torch.full((64,), 77, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    z64, z32 = torch.zeros(64, dtype=torch.int64, device="cuda"), \
        torch.zeros(64, dtype=torch.int32, device="cuda")
    s = stream_ptr(out.device)
    head = [ptr(z32), ptr(z64), ptr(z64), ptr(z64), ptr(z32)]
    tail = [ptr(z32), ptr(z64), ptr(out), ptr(final), ptr(status)]
    for N in wref.WAYS:
        assert lib().idf_predict_decode_ways_u8(s, 1, 0, N, 4, 120, 127, *head, None, None,
                                                *tail) == 4
        assert lib().idf_predict_ways_supported(4, 120, 126, N) == 0
    assert lib().idf_predict_decode_u8(s, 1, 1, 1, 32769, *head, *tail) == 4
    assert lib().idf_predict_decode2_u8(s, 1, 0, 1, 1, 32769, *head, None, None, *tail) == 4
    torch.cuda.synchronize()
    assert bool((big == GUARD).all()) and bool((final == 77).all()) and int(status[0]) == -1


# ------------------------------------------------------------------ 3. the other kernels at 64 x 64
def _raw_case(C):
    """case64's images on the device, their table, rectangles, byte offsets in reverse entry
    order and the raw bytes numpy expects."""
    case = pc.case64(C)
    src = [torch.from_numpy(i).cuda() for i in case["imgs"]]
    rows, entries = _rows(src, TH, TW)
    offs, total = pc.reverse_layout(case["counts"])
    want = np.full(total, GUARD, dtype=np.uint8)
    for e, p in enumerate(case["planes"]):
        want[offs[e]:offs[e] + p.size] = p.reshape(-1)
    return case, src, rows, offs, want


@pytest.mark.parametrize("C", [1, 3, 4])
def test_raw_copies_verify_and_crc_at_64x64(C):
    from idfcodec.integrity import device_tile_crc32, device_tile_crc32_pm
    from idfcodec.safe import device_gather_raw, device_scatter_raw, device_verify
    from idfcodec.tiled import device_gather
    case, src, rows, offs, want = _raw_case(C)
    imgs, rects, n = case["imgs"], case["rects"], len(rows)
    table, d_off = _dev(rows, torch.int64), _dev(offs, torch.int64)
    # gather and scatter: four full 1024-pixel blocks a full tile
    big, (raw,) = _guarded([(len(want),)])
    device_gather_raw(table, n, C, TH, TW, d_off, raw)
    assert _guards_intact(big, [raw], [want])
    obig, outs = _guarded([i.shape for i in imgs])
    orows, _ = _rows(outs, TH, TW)
    device_scatter_raw(_dev(orows, torch.int64), n, C, TH, TW, raw, d_off,
                       _dev(rects, torch.int32))
    assert _guards_intact(obig, outs, imgs)
    # verify: one changed byte in each of the four blocks of a full tile, one at a time
    buf = torch.zeros(n * TH * TW * 4, device="cuda")
    device_gather(table, n, C, TH, TW, buf)
    mism = torch.zeros(n, dtype=torch.int32, device="cuda")

    def count():
        mism.zero_()
        device_verify(table, n, C, TH, TW, buf, mism)
        return mism.tolist()
    assert count() == [0] * n
    full = [e for e, r in enumerate(rects) if r == (TH, TW)]
    for blk, t in zip(range(4), full[1:]):
        pixel = 1024 * blk + (0, 1023, 517, 64)[blk]
        i = (t * TH * TW + pixel) * 4 + (C - 1 if blk % 2 else 0)
        old = float(buf[i])
        buf[i] = old + (2 / 256 if old < 0.5 else -2 / 256)
        assert count() == [int(e == t) for e in range(n)], (blk, t)
        buf[i] = old
    assert count() == [0] * n
    # CRC-32 of the sources and of the pixel-major rows: three or four 4096-byte chunks
    crcs = crc_ref.tile_crcs(imgs, TH, TW)
    assert crcs[full[1]] == zlib.crc32(case["planes"][full[1]].tobytes())
    out = torch.full((n + 16,), SELGUARD, dtype=torch.int32, device="cuda")
    device_tile_crc32(table, n, C, TH, TW, out[8:8 + n])
    got = out.cpu().numpy().view(np.uint32)
    assert got[8:8 + n].tolist() == crcs and (got[:8] == SELGUARD).all() and \
        (got[8 + n:] == SELGUARD).all()
    out.fill_(SELGUARD)
    device_tile_crc32_pm(buf, n, C, TH, TW, _dev(rects, torch.int32), out[8:8 + n])
    got = out.cpu().numpy().view(np.uint32)
    assert got[8:8 + n].tolist() == crcs and (got[:8] == SELGUARD).all() and \
        (got[8 + n:] == SELGUARD).all()


@pytest.mark.parametrize("th,tw", [(64, 64), (40, 33)])
@pytest.mark.parametrize("C,colour", [(1, False), (3, False), (3, True), (4, False), (4, True)])
def test_cost_kernel_equals_the_reference_at_the_larger_tiles(C, colour, th, tw):
    from idfcodec._lib import lib, ptr, stream_ptr
    if (th, tw) == (64, 64):
        case = pc.case64(C)
        imgs, planes = case["imgs"], case["planes"]
    else:
        from test_gpu_predict import _case
        case = _case(C, th, tw)
        imgs, planes = case["imgs"], case["planes"]
    want = np.array([costref.costs(p, colour) for p in planes], dtype=np.int64)
    src = [torch.from_numpy(i).cuda() for i in imgs]
    rows, _ = _rows(src, th, tw)
    n, gap = len(rows), 16
    buf = torch.full((2 * n + 2 * gap,), GUARD64, dtype=torch.int64, device="cuda")
    out = buf[gap:gap + 2 * n]
    assert lib().idf_predict_cost_u8(stream_ptr(out.device), n, C, th, tw,
                                     ptr(_dev(rows, torch.int64)), int(colour), ptr(out)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(n, 2)
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.array_equal(got[:, 1], want[:, 1] if colour else np.zeros(n, np.int64))
    assert bool((buf[:gap] == GUARD64).all()) and bool((buf[gap + 2 * n:] == GUARD64).all())


# ------------------------------------------------------------------ 4. end to end without a flow
@pytest.fixture(scope="module")
def model64():
    return _tiny_model(2, 1, 64, 64, 3, 1).cuda()


def _grey(Cs):
    """Grey (Cs = 1) and grey + alpha (2) sources of ragged sizes: 1, 3 x 2 and 1 x 4 tiles."""
    sizes = [(64, 64), (130, 70), (5, 200)]
    names = ("noise", "ramp", "vstep", "zeros")
    imgs = []
    for i, (H, W) in enumerate(sizes):
        c = pc.contents((1, H, W), seed=3 * i)
        planes = [c[names[(i + p) % 4]][0] for p in range(Cs)]
        imgs.append(torch.from_numpy(np.stack(planes)).cuda())
    return imgs


@pytest.mark.parametrize("N", [1, 64])
@pytest.mark.parametrize("Cs", [1, 2])
def test_grey_sources_through_tiled_planes_of_a_64x64_model(model64, Cs, N):
    from idfcodec import planes
    from test_gpu_planes import _units
    imgs = _grey(Cs)
    codec = model64.tiled_planes(Cs, predict_ways=N)
    assert (codec.Cb, codec.Ce) == (0, Cs) and codec.tile_hw == (64, 64)
    bs = codec.encode(imgs)
    assert bs.base is None and bs.n_units == Cs * (1 + 6 + 4) and bs.predict_ways == N
    got = planes.PlaneSetBitstream.from_bytes(bs.to_bytes(), device="cuda")
    outs, info = codec.decode(got)
    assert info["ok"] and info["flow_tiles"] == 0
    assert len(outs) == len(imgs) and all(torch.equal(a, b) for a, b in zip(outs, imgs))
    # every packed unit is the reference's stream
    units = _units(imgs, 0, bs.layout)
    const = np.array([u.min() == u.max() for u in units])
    coded = [pc.encode(u, N) for u, c in zip(units, const) if not c]
    nw = np.array([len(c.words) for c in coded], dtype=np.int64)
    nb = np.array([u.size for u in units])
    cls = np.full(len(units), planes.CLASS_CONSTANT, dtype=np.uint8)
    cls[~const] = planes.unit_class(np.zeros(len(coded)), np.ones(len(coded)),
                                    np.zeros(len(coded)), nw, nb[~const], N)
    assert np.array_equal(bs.classes, cls) and {0, 1, 2} <= set(cls.tolist())
    pk = [c for c, k in zip(coded, cls[~const]) if k == planes.CLASS_PACKED]
    assert len(pk) >= 2 and bs.sel.tolist() == [c.sel for c in pk]
    assert np.array_equal(np.asarray(bs.states, dtype=np.uint64).reshape(-1, N),
                          np.array([c.states for c in pk], dtype=np.uint64))
    assert np.array_equal(bs.words.cpu().numpy().view(np.uint32),
                          np.concatenate([c.words for c in pk]))
    # a region across a tile corner of the 3 x 2 image
    y0, x0, h, w = 60, 59, 69, 9
    crop, info = codec.decode_region(got, 1, y0, x0, h, w)
    assert info["ok"] and torch.equal(crop, imgs[1][:, y0:y0 + h, x0:x0 + w])
