"""The 8-bit predictive decoders on damaged streams, compared with the references entry by entry:
idf_predict_decode_u8 under each search shape, idf_predict_decode2_u8 and
idf_predict_decode_ways_u8 at N = 8, 16, 32, 64 over plain and colour entries, one launch per
configuration holding every damaged unit of tests/predict_cases.py between intact ones, the
outputs handed out in reverse order with gaps inside a guarded buffer.

For every entry -- none is skipped or filtered by outcome -- d_status, every final state and the
bytes equal the reference's (predict_ref, colour_ref, predict_ways_ref with the device's "step"
stop rule).  The bytes: at N ways all C hin win of them, the zeros of the pixels not reached
included (a colour entry's after the inverse transform, which runs over them too).  At one way
the bytes the reference reached, and every byte behind an UNDERFLOW is still the guard value; in a
colour entry stopped by UNDERFLOW the inverse transform has run over unwritten bytes, so there a
byte of plane 0 or 2 is compared only where the reference reached it and its partner in plane 1,
and the guard value is asserted behind the stop in the planes the inverse does not touch.

The rectangle cases ride along: a rectangle above the tile decodes as the tile, a negative one
holds no symbol (nothing written, the final state the initial one, WORDS_LEFT iff words were
given).  All of it is data: every offset and count stays inside its allocation."""
import numpy as np
import pytest
import torch

import predict_cases as pc
import predict_ref as ref
from test_gpu_safe import GUARD, _dev, _guarded

pytestmark = pytest.mark.gpu

L = ref.L
SHAPES = pc.UNIT_SHAPES
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _launch(cases, C, th, tw, N, call):
    """One launch over `cases` -> (big, out, offsets, room, final uint64 [n, N], status)."""
    from idfcodec.predict import (device_predict_decode, device_predict_decode2,
                                  device_predict_decode_ways)
    n, room = len(cases), C * th * tw
    a = pc.launch_arrays(cases, N)
    offs, total = pc.reverse_layout([room] * n)
    big, (out,) = _guarded([(total,)])
    final = torch.zeros(n * N, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    i32 = lambda v: torch.from_numpy(v.view(np.int32).copy()).cuda()  # noqa: E731
    head = (i32(a["words"]), _dev(a["w_off"], torch.int64), _dev(a["nw"], torch.int64),
            torch.from_numpy(a["states"].view(np.int64).reshape(-1).copy()).cuda(), i32(a["sel"]))
    tail = (_dev(a["rects"], torch.int32), _dev(offs, torch.int64), out, final, status)
    nc = int(a["col"].sum())
    colour = (i32(a["sel2"]), torch.from_numpy(a["col"]).cuda(), nc) if nc else (None, None, 0)
    if call == "one":
        assert nc == 0
        device_predict_decode(n, C, th, tw, *head, *tail)
    elif call == "two":
        device_predict_decode2(n, C, th, tw, *head, *colour, *tail)
    else:
        device_predict_decode_ways(n, N, C, th, tw, *head, *colour, *tail)
    torch.cuda.synchronize()
    return (big, out.cpu().numpy(), offs, room,
            final.cpu().numpy().view(np.uint64).reshape(n, N), status.cpu().numpy())


def _check(cases, C, th, tw, N, call):
    big, got, offs, room, final, status = _launch(cases, C, th, tw, N, call)
    assert sum(c.planes is None for c in cases) >= 20 and any(c.planes is not None for c in cases)
    for e, c in enumerate(cases):
        want, want_S, want_status, trace = c.want
        assert int(status[e]) == want_status, (c.name, int(status[e]), want_status)
        assert [int(s) for s in final[e]] == [int(s) for s in want_S], c.name
        if c.planes is not None:            # an intact entry: exact, state L, status 0
            assert np.array_equal(want, c.planes) and want_status == 0
            assert all(s == L for s in want_S)
        seg = got[offs[e]:offs[e] + room + 5]
        flat, n = want.reshape(-1), want.size
        assert (seg[n:] == GUARD).all(), c.name
        if N > 1 or not want_status & ref.UNDERFLOW:
            assert np.array_equal(seg[:n], flat), c.name
            continue
        r = trace["reached"]                # one way: the entry stopped behind r bytes
        assert r < n
        if c.entry.sel2 is None:
            assert np.array_equal(seg[:r], flat[:r]), c.name
            assert (seg[r:n] == GUARD).all(), c.name
            continue
        npl = n // C
        idx = np.arange(n)
        plane, q = idx // npl, idx % npl
        known = np.where(plane == 0, npl + q < r, idx < r)
        assert np.array_equal(seg[:n][known], flat[known]), c.name
        behind = (idx >= r) & (plane != 0) & (plane != 2)
        assert (seg[:n][behind] == GUARD).all(), c.name
    # the guard bytes around the output buffer
    o = big.cpu().numpy()
    assert (o[:64] == GUARD).all() and (o[64 + len(got):] == GUARD).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("search", [None, "1", "2"])
def test_one_way_decoder_equals_the_reference_on_every_damaged_entry(monkeypatch, shape, search):
    """idf_predict_decode_u8 (no colour flag exists: the plain entries, a colour coding with its
    flag cleared among them) under IDF_PREDICT_SEARCH unset, 1 and 2."""
    if search is None:
        monkeypatch.delenv("IDF_PREDICT_SEARCH", raising=False)
    else:
        monkeypatch.setenv("IDF_PREDICT_SEARCH", search)
    _check(pc.plain_only(pc.damage_set(shape, 1)), *shape, 1, "one")


@pytest.mark.parametrize("search", [None, "1", "2"])
def test_one_way_decoder_of_plain_and_colour_entries_equals_the_reference(monkeypatch, search):
    """idf_predict_decode2_u8: plain and colour entries mixed, the inverse transform behind."""
    if search is None:
        monkeypatch.delenv("IDF_PREDICT_SEARCH", raising=False)
    else:
        monkeypatch.setenv("IDF_PREDICT_SEARCH", search)
    cases = pc.damage_set(SHAPES[0], 1)
    assert any(c.entry.sel2 is not None and c.want[2] & ref.UNDERFLOW for c in cases)
    _check(cases, *SHAPES[0], 1, "two")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_n_way_decoder_equals_the_step_reference_on_every_damaged_entry(shape, N):
    """idf_predict_decode_ways_u8, plain and colour entries mixed (C >= 3): symbol for symbol
    the serial loop up to the step that lacks a word."""
    _check(pc.damage_set(shape, N), *shape, N, "ways")
