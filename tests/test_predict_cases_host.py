"""tests/predict_cases.py on the host (no device): the damage set yields, through the references
alone, every outcome the device tests compare (so they cannot pass on a set that has stopped
covering anything), predict_ways_ref's "step" stop rule against its serial one, and the big
geometries reach the regimes they are there for."""
import numpy as np
import pytest

import predict_cases as pc
import predict_ref as ref
import predict_ways_ref as wref
from idfcodec import predict

L = ref.L
U, O, W = ref.UNDERFLOW, ref.OUT_OF_WINDOW, ref.WORDS_LEFT
BIG = (3, 16, 16)


def _damaged(cases):
    return [c for c in cases if c.planes is None and not c.name.startswith("rect")]


def _outcomes(cases):
    return {(c.want[2], all(s == L for s in c.want[1])) for c in _damaged(cases)}


def test_kinds_and_room():
    kinds = pc.damage_kinds()
    assert len(kinds) == len(set(kinds)) == 23 and sum(k.startswith("word ") for k in kinds) == 12
    plain, colour = (pc.encode(pc.units(BIG)[1][1], 1, col) for col in (False, True))
    assert [k for k in kinds if pc.damaged(plain, k) is None] == ["sel2 = 0", "sel2 = 0xFFFFFFFF"]
    assert all(pc.damaged(colour, k) is not None for k in kinds)
    assert pc.damaged(plain, "colour flag flipped", C=2) is None
    empty = plain._replace(words=plain.words[:0])
    left = [k for k in kinds if pc.damaged(empty, k) is not None]
    assert left == ["an extra word in front", "state below L", "state bit 63", "sel = 0",
                    "sel = 0xFFFFFFFF", "colour flag flipped"]
    # values change, counts move by one (or to none), the entry's own arrays are never shared
    for k in kinds[:16]:
        bad = pc.damaged(colour, k)
        assert bad.words is not colour.words and bad.words.dtype == np.uint32
        assert len(bad.words) in (len(colour.words) - 1, len(colour.words), len(colour.words) + 1,
                                  0)
        assert (bad.sel, bad.sel2, bad.states) == colour[:3]


@pytest.mark.parametrize("N", [1, 8, 64])
def test_the_damage_set_yields_every_outcome(N):
    """For plain entries (the one-way reference, or the N-way one) and for colour entries alike:
    status 0 beside a final state other than L, 8, 16, 24, 32 with every state L, and 48."""
    cases = pc.damage_set(BIG, N)
    for col in (False, True):
        part = [c for c in cases if (c.entry.sel2 is not None) == col]
        got = _outcomes(part)
        assert {(0, False), (U, False), (O, False), (U | O, False), (W, True),
                (W | O, False)} <= got, (col, sorted(got))
        dmg = _damaged(part)
        # OUT_OF_WINDOW with a decoded 0 and with a decoded 255
        assert any(c.want[3]["low"] for c in dmg) and any(c.want[3]["high"] for c in dmg)
        # UNDERFLOW at the first read, mid-stream and at the last read
        seen = []
        for content in pc.CONTENTS:
            by = {c.name.split(": ")[1]: c for c in dmg if c.name.startswith(content)}
            first, last = by["no words"], by["first pushed word dropped"]
            assert first.want[2] & U and last.want[2] & U
            assert first.want[3]["reached"] <= last.want[3]["reached"] < 768
            seen += [c.name for c in by.values() if c.want[2] & U and len(c.entry.words)
                     and first.want[3]["reached"] < c.want[3]["reached"] < last.want[3]["reached"]]
        assert seen
    if N == 64:  # a step that lacks a word leaves words behind
        assert any(c.want[2] & (U | W) == U | W for c in _damaged(cases))
    # the small one-plane unit takes part too, and every intact entry decodes to its bytes
    small = pc.damage_set((1, 12, 8), N)
    assert len(_damaged(small)) >= 20
    for c in cases + small:
        if c.planes is not None:
            assert np.array_equal(c.want[0], c.planes) and c.want[2] == 0, c.name
            assert all(s == L for s in c.want[1]), c.name


def test_the_rectangle_cases():
    for N in (1, 64):
        by = {c.name: c for c in pc.damage_set(BIG, N)}
        above = by["rect above the tile"]
        assert above.rect[0] > 16 and above.rect[1] > 16 and above.want[0].shape == (3, 16, 16)
        for name in ("rect (-1, 16)", "rect (16, -5)", "rect (-2, -2)"):
            c = by[name]
            assert c.want[0].size == 0 and c.want[2] == W and len(c.entry.words) > 0
            assert tuple(c.want[1]) == c.entry.states
        c = by["rect (-1, -1) without words"]
        assert c.want[0].size == 0 and c.want[2] == 0 and tuple(c.want[1]) == c.entry.states


@pytest.mark.parametrize("shape,N", [(BIG, 8), (BIG, 64), ((1, 12, 8), 16), ((1, 12, 8), 32)])
def test_step_stop_equals_serial_stop_up_to_the_step_that_lacks_a_word(shape, N):
    C, h, w = shape
    t = wref.steps_slots(C, h, w, N)[0].reshape(C, h, w)
    q = wref.order(C, h, w, N)
    n_under = 0
    for c in pc.damage_set(shape, N):
        hh, ww = (0, 0) if min(c.rect) < 0 else (h, w)
        e = c.entry
        ser = wref.decode(e.sel, e.states, e.words, C, hh, ww, N, e.sel2, "serial", trace := {})
        step = c.want
        if not ser[2] & U:
            assert np.array_equal(step[0], ser[0]) and step[1] == ser[1] and step[2] == ser[2]
            continue
        # the serial loop stopped inside some step: the step rule decodes the steps before it
        n_under += 1
        assert step[2] & U and step[2] & O <= ser[2] & O and not ser[2] & W
        stop_t = int(t.reshape(-1)[np.flatnonzero(q.reshape(-1) == trace["reached"])[0]])
        early = t < stop_t
        assert step[3]["reached"] == int(early.sum()) <= trace["reached"]
        if step[2] & W:   # too few words for the step: the serial loop used them inside it
            assert step[3]["reached"] < trace["reached"]
        if e.sel2 is not None:   # the inverse needs plane 1 of the same pixel
            early = early & np.broadcast_to(early[1], early.shape)
        assert np.array_equal(step[0][early], ser[0][early]), c.name
    assert n_under >= (10 if shape == BIG else 3)


# ------------------------------------------------------------------ the big geometries
def test_big_units_reach_their_regimes():
    units = pc.big_units()
    geos = {(k, C, th, tw): (Ns, ps) for k, C, th, tw, Ns, ps in units}
    assert set(geos) == {("ways", 2, 70, 130), ("ways", 1, 3, 200), ("ways", 4, 120, 126),
                         ("one", 1, 1, 32768), ("one", 4, 1, 15000)}
    Ns, ps = geos["ways", 2, 70, 130]
    assert Ns == (8, 16, 32, 64) and [p.shape for p in ps] == [(2, 70, 130), (2, 70, 65)]
    assert all(p.shape[2] > 64 for p in ps)                       # win > N at N = 64: P = win
    assert -(-140 // 64) == 3 and 140 % 64 == 12 and -(-140 // 8) == 18
    assert geos["ways", 1, 3, 200][0] == (64,)
    # the LDS limit, by the header's formula
    assert pc.ways_lds_bytes(4, 120, 126) == 320 + 480 + 60480 == 61280 <= 61440
    assert pc.ways_lds_bytes(4, 120, 127) == 61760 > 61440
    for N in wref.WAYS:
        assert predict.ways_supported(4, 120, 126, N) and not predict.ways_supported(4, 120, 127, N)
        assert predict.ways_supported(2, 70, 130, N) and predict.ways_supported(4, 64, 64, N)
    # every big unit packs at every N it runs at (noise-free)
    for kind, C, th, tw, Ns, ps in units:
        for p in ps:
            for N in Ns:
                e = pc.encode(p, N)
                cost = (16 if N == 1 else 8 + 8 * N) + 4 * len(e.words)
                if p.size > 4096:
                    assert cost < p.size, (kind, C, th, tw, N)
                    assert len(e.words) > 128                      # both word windows refill


@pytest.mark.parametrize("C", [1, 3, 4])
def test_the_64x64_contents_pack_unless_they_are_noise(C):
    case = pc.case64(C)
    assert set(case["rects"]) == {(64, 64), (1, 64), (64, 1), (5, 5), (64, 5), (5, 64)}
    assert C * 64 * 64 in (4096, 12288, 16384) and (C * 64) // 64 == C   # C bands at N = 64
    full = [e for e, r in enumerate(case["rects"]) if r == (64, 64)]
    assert len(full) == 4 * len(pc.CONTENTS)
    for N in (1, 64):
        nw = pc.coded64(C, N)["nw"]
        for e in full:
            cost = (16 if N == 1 else 8 + 8 * N) + 4 * int(nw[e])
            assert (cost < case["counts"][e]) == (case["names"][e] != "noise"), (N, e)
        assert int(nw.max()) > 128
