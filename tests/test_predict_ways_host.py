"""The predictive coder's interleaved streams on the host (no device): the wavefront schedule's
properties, the library's closed-form order against the reference's sort, the reference's round
trip with every state back at L, the container's flags field and its refusals, and the cost rule
8 + 8 N + 4 nwords."""
import struct

import numpy as np
import pytest
import torch

import predict_ref as ref
import predict_ways_ref as wref
from idfcodec import predict  # the module under test: every test here needs it
from test_predict_colour_host import _col
from test_predict_host import MIXED, PACKED, SHAPES, _pred, contents
from test_safe_host import SIZES, _safe

# the rectangles of tests/test_gpu_predict_ways.py, and a full 64 x 64 x 3 entry
RECTS = [(1, 1, 1), (3, 16, 16), (3, 12, 8), (3, 40, 33), (1, 5, 5), (4, 5, 1), (3, 1, 7),
         (2, 9, 3), (3, 64, 64)]
NS = [1, 8, 16, 32, 64]


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("shape", RECTS, ids=lambda s: "x".join(map(str, s)))
def test_schedule_properties(shape, N):
    C, h, w = shape
    t, j = wref.steps_slots(C, h, w, N)
    q = wref.order(C, h, w, N).reshape(C * h, w)
    n = q.size
    # every step holds at most N pixels of distinct slots
    tf, jf, qf = t.reshape(-1), j.reshape(-1), q.reshape(-1)
    by_q = np.argsort(qf)
    assert np.array_equal(np.sort(qf), np.arange(n))
    for step in np.unique(tf):
        slots = jf[tf == step]
        assert len(slots) <= N and len(set(slots.tolist())) == len(slots)
        # the symbols of one step are consecutive: they meet distinct states
        ranks = np.sort(qf[tf == step])
        assert np.array_equal(ranks, np.arange(ranks[0], ranks[0] + len(ranks)))
        states = (n - 1 - ranks) % N
        assert len(set(states.tolist())) == len(ranks)
    assert (np.diff(tf[by_q]) >= 0).all()                      # q ascends with the step
    # a, b and c lie in strictly earlier steps (rows of one plane only: y > 0)
    rho = np.arange(C * h)
    up = (rho % h) > 0
    assert (t[:, 1:] > t[:, :-1]).all()                        # a
    assert (t[up][:, :] > t[rho[up] - 1][:, :]).all()          # b
    assert (t[up][:, 1:] > t[rho[up] - 1][:, :-1]).all()       # c
    if N == 1:
        assert np.array_equal(qf, np.arange(n))                # today's raster order


def test_step_counts_of_a_full_entry():
    """The steps a 64 x 64 x 3 entry takes: 1543 / 783 / 415 / 255 at 8 / 16 / 32 / 64 ways."""
    got = [int(wref.steps_slots(3, 64, 64, N)[0].max()) + 1 for N in (8, 16, 32, 64)]
    assert got == [1543, 783, 415, 255]
    # no step is idle
    for N in (8, 16, 32, 64):
        for shape in RECTS:
            t = wref.steps_slots(*shape, N)[0]
            assert len(np.unique(t)) == int(t.max()) + 1


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("shape", RECTS, ids=lambda s: "x".join(map(str, s)))
def test_library_order_is_the_reference_order(shape, N):
    got = predict.order(*shape, N)
    assert got.dtype == np.int64 and got.shape == shape
    assert np.array_equal(got, wref.order(*shape, N))


def test_order_and_support_refuse_bad_arguments():
    from idfcodec._lib import lib
    buf = (np.zeros(16, dtype=np.int64)).ctypes.data
    for ways in (0, 2, 4, 7, 128, -8):
        assert lib().idf_predict_order(1, 2, 2, ways, buf) == 1
        assert lib().idf_predict_ways_supported(3, 16, 16, ways) == 1
    assert lib().idf_predict_ways_supported(3, 16, 16, 1) == 1     # one way has its own decoder
    assert lib().idf_predict_order(1, 2, 2, 8, None) == 1
    assert lib().idf_predict_order(5, 2, 2, 8, buf) == 1 and lib().idf_predict_order(1, 0, 2, 8,
                                                                                      buf) == 1
    assert predict.ways_supported(3, 64, 64, 64) and predict.ways_supported(4, 40, 33, 8)
    # an entry that cannot live in LDS: unsupported, not an argument error
    assert lib().idf_predict_ways_supported(3, 256, 256, 8) == 4
    assert not predict.ways_supported(3, 256, 256, 8)
    assert not predict.ways_supported(1, 1, 1 << 30, 8)
    with pytest.raises(ValueError, match="predict_ways"):
        predict.check_predict_ways(4)
    with pytest.raises(ValueError, match="predict_ways"):
        predict.check_predict_ways(True)


def test_launchers_refuse_bad_ways_before_any_launch():
    """IDF_ERR_ARG (1) for ways outside {8, 16, 32, 64} and for the one-way calls' bad arguments;
    IDF_ERR_UNSUPPORTED (4) for a geometry that does not fit.  None reaches the device."""
    from idfcodec._lib import lib
    L = lib()
    one = 8  # any non-NULL address: the calls below return before it is read
    prep = lambda ways, n=1, C=3, p=one: L.idf_predict_prep_ways_u8(  # noqa: E731
        None, n, C, 16, 16, p, p, p, p, p, p, ways)
    prep2 = lambda ways, n=1, C=3, p=one: L.idf_predict_prep2_ways_u8(  # noqa: E731
        None, n, C, 16, 16, p, p, p, p, p, p, ways)
    dec = lambda ways, n=1, C=3, th=16, tw=16, p=one, nc=0: L.idf_predict_decode_ways_u8(  # noqa: E731
        None, n, nc, ways, C, th, tw, p, p, p, p, p, p, p, p, p, p, p, p)
    for call in (prep, prep2, dec):
        for ways in (1, 4, 128, 0, 12):
            assert call(ways) == 1 and call(ways, n=0) == 1
        assert call(8, n=0) == 0
        assert call(8, p=None) == 1
        assert call(8, n=-1) == 1 and call(8, C=5) == 1
    assert prep2(8, C=2) == 1
    assert dec(8, C=2, nc=1) == 1 and dec(8, nc=2) == 1
    assert dec(64, th=256, tw=256) == 4


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_round_trips_with_every_state_at_L(shape):
    big = shape[1] * shape[2] > 400
    for i, (name, p) in enumerate(contents(shape).items()):
        if big and name not in ("ramp", "noise"):
            continue  # the serial decoder calls the oracle per probe: two contents at 40x33
        for N in ((8, 64)[i % 2:][:1] if big else wref.WAYS):
            sel, _, S, words = wref.encode(p, N)
            assert sel == ref.choose_sel(p)
            out, final, status = wref.decode(sel, S, words, *shape, N)
            assert np.array_equal(out, p) and status == 0, (name, N)
            assert final == [ref.L] * N, (name, N)


def test_reference_round_trips_a_colour_entry():
    import colour_ref as cref
    p = cref.correlated(12, 8, 5)
    for N in (8, 32):
        sel, sel2, S, words = wref.encode(p, N, colour=True)
        assert (sel, sel2) == cref.choose_sels(p)
        out, final, status = wref.decode(sel, S, words, 3, 12, 8, N, sel2=sel2)
        assert np.array_equal(out, p) and status == 0 and final == [ref.L] * N


def test_one_way_is_the_serial_stream():
    p = contents((3, 12, 8))["ramp"]
    for a, b in zip(wref.arrays(p, 1), ref.arrays(p)):
        assert np.array_equal(a, b)
    sel, state, words = ref.encode(p)
    _, _, S, w1 = wref.encode(p, 1)
    assert S == [state] and np.array_equal(w1, words)


def test_the_symbols_are_a_permutation_of_the_serial_ones():
    p = contents((3, 40, 33))["noise"]
    base = ref.arrays(p)
    for N in wref.WAYS:
        q = wref.order(3, 40, 33, N).reshape(-1)
        for a, b in zip(wref.arrays(p, N), base):
            assert np.array_equal(a[p.size - 1 - q], b[::-1])


def test_a_damaged_reference_stream_is_flagged():
    p = contents((3, 16, 16))["noise"]
    sel, _, S, words = wref.encode(p, 8)
    out, final, status = wref.decode(sel, S, words[1:], 3, 16, 16, 8)
    assert status & ref.UNDERFLOW
    bad = words.copy()
    bad[len(bad) // 2] ^= 0x00010000
    out, final, status = wref.decode(sel, S, bad, 3, 16, 16, 8)
    assert status != 0 or final != [ref.L] * 8


# ------------------------------------------------------------------ the container
def _ways(pbs, N):
    """The hand-made bitstream with N states an entry: state w of packed entry p is
    L + 1000 * p + w."""
    P = pbs.n_packed
    pbs.states = (np.uint64(1 << 32) + np.uint64(1000) * np.arange(P, dtype=np.uint64)[:, None]
                  + np.arange(N, dtype=np.uint64)[None, :])
    pbs.predict_ways = N
    return pbs


@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("make,magic", [(_pred, b"IDFP"), (lambda e, p: _col(e, p), b"IDFQ")])
def test_container_round_trip_and_layout(make, magic, N):
    from idfcodec.predict import PredictiveTiledBitstream as PB
    pbs = _ways(make(MIXED, PACKED), N)
    buf = pbs.to_bytes()
    one = make(MIXED, PACKED).to_bytes()
    assert buf[:4] == magic and struct.unpack_from("<H", buf, 6)[0] == N
    assert struct.unpack_from("<H", one, 6)[0] == 0
    assert len(buf) == len(one) + 2 * 8 * (N - 1)
    o_map = 24 + 8 * len(SIZES)
    o_sect = o_map + (3 if magic == b"IDFQ" else 2) + 8 + 3     # entry 0 is raw: 3 bytes
    P = 2
    assert struct.unpack_from("<QI", buf, o_sect)[1] == P
    # entry-major, way-minor behind sel[P]
    st = np.frombuffer(buf, "<u8", P * N, o_sect + 12 + 4 * P).reshape(P, N)
    assert np.array_equal(st, pbs.states)
    assert struct.unpack_from("<II", buf, o_sect + 12 + 4 * P + 8 * N * P) == (2, 3)   # nwords
    got = PB.from_bytes(buf)
    assert got.predict_ways == N and got.states.shape == (P, N)
    assert got.to_bytes() == buf
    assert np.array_equal(got.states, pbs.states) and np.array_equal(got.sel, pbs.sel)
    assert np.array_equal(got.nwords, pbs.nwords) and torch.equal(got.words, pbs.words)
    assert (got.colour is None) == (magic == b"IDFP")
    assert got.bits() == make(MIXED, PACKED).bits() + 64 * (N - 1) * P
    # one way reads back as before
    assert PB.from_bytes(one).predict_ways == 1 and PB.from_bytes(one).states.shape == (P,)


def test_one_way_bytes_are_unchanged():
    """predict_ways = 1 is the default and writes flags 0: test_predict_host's frozen digest."""
    import hashlib
    pbs = _pred(MIXED, PACKED)
    assert pbs.predict_ways == 1
    assert hashlib.sha256(pbs.to_bytes()).hexdigest() == \
        "cbdaa07fe420b1c402ae6e41a5e4fac0521fac36b6753031fd3ff00402a69cc7"


def test_flags_refused():
    from idfcodec.predict import PredictiveTiledBitstream as PB
    from idfcodec.safe import SafeTiledBitstream
    from idfcodec.tiled import TiledBitstream, TileLayout
    buf = _ways(_pred(MIXED, PACKED), 8).to_bytes()
    for make in (_pred, lambda e, p: _col(e, p)):
        good = _ways(make(MIXED, PACKED), 8).to_bytes()
        for flags in (3, 128, 1, 4, 9, 0x8000):
            bad = good[:6] + struct.pack("<H", flags) + good[8:]
            with pytest.raises(ValueError, match="flags"):
                PB.from_bytes(bad)
        # the flags say 16 or one way, the section holds 8 states an entry: its length (in an
        # IDFQ file the count of second tables, read first) does not fit
        for flags in (16, 0, 64):
            with pytest.raises(ValueError, match="packed section|colour tiles"):
                PB.from_bytes(good[:6] + struct.pack("<H", flags) + good[8:])
    # the other tiled containers take no flags
    lay = TileLayout(SIZES, 3, (16, 16))
    with pytest.raises(ValueError, match="flags"):
        TiledBitstream.from_bytes(lay.pack(b"IDFT", 8) + bytes(64))
    safe = _safe(MIXED).to_bytes()
    assert SafeTiledBitstream.from_bytes(safe).to_bytes() == safe
    with pytest.raises(ValueError, match="flags"):
        SafeTiledBitstream.from_bytes(safe[:6] + struct.pack("<H", 8) + safe[8:])
    assert buf[:4] == b"IDFP"
    with pytest.raises(ValueError, match="not an IDF"):
        SafeTiledBitstream.from_bytes(buf)


def test_sealed_container_takes_no_flags():
    import zlib
    from idfcodec.integrity import SealedBitstream
    head = struct.pack("<4sHH", b"IDFC", 1, 8) + bytes(16)
    with pytest.raises(ValueError, match="flags|truncated|version"):
        SealedBitstream.from_bytes(head + struct.pack("<I", zlib.crc32(head)))


def test_a_section_truncated_by_one_state_is_refused():
    from idfcodec.predict import PredictiveTiledBitstream as PB
    N = 8
    buf = _ways(_pred(MIXED, PACKED), N).to_bytes()
    o_sect = 24 + 8 * len(SIZES) + 2 + 8 + 3
    (n_sect,) = struct.unpack_from("<Q", buf, o_sect)
    assert n_sect == 4 + (8 + 8 * N) * 2 + 4 * 5
    o_st = o_sect + 8 + 4 + 4 * 2                        # the first state
    cut = buf[:o_sect] + struct.pack("<Q", n_sect - 8) + buf[o_sect + 8:o_st] + buf[o_st + 8:]
    with pytest.raises(ValueError, match="packed section"):
        PB.from_bytes(cut)
    # the writer refuses tables that do not hold N states an entry
    bad = _ways(_pred(MIXED, PACKED), N)
    bad.states = bad.states[:, :N - 1]
    with pytest.raises(ValueError, match="states"):
        bad.to_bytes()
    bad = _ways(_pred(MIXED, PACKED), N)
    bad.predict_ways = 4
    with pytest.raises(ValueError, match="predict_ways"):
        bad.to_bytes()


# ------------------------------------------------------------------ the cost rule
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_cost_rule_is_eight_a_state(N):
    from idfcodec.predict import choose_streams, entry_overhead, is_packed
    assert entry_overhead(1) == 16 == predict.ENTRY_BYTES
    assert entry_overhead(1, True) == 20 == predict.ENTRY_BYTES_COLOUR
    assert entry_overhead(N) == 8 + 8 * N == wref.entry_cost(0, N)
    assert entry_overhead(N, True) == wref.entry_cost(0, N, colour=True)
    fixed = 8 + 8 * N
    n_bytes = fixed + 4 * 10 + 1
    # 10 words fit below the bytes, 11 do not; a tie stores raw; a status stores raw
    got = is_packed([0, 0, 0, 16], [10, 11, 10, 0], [n_bytes, n_bytes, n_bytes - 1, n_bytes], N)
    assert got.tolist() == [True, False, False, False]
    assert not is_packed([0], [0], [fixed], N)[0] and is_packed([0], [0], [fixed + 1], N)[0]
    # both candidates: colour iff nw_c + 1 < nw_p ... by 4 bytes, whatever N
    nw = np.array([10, 8, 10, 9, 10, 10, 30, 1])           # (plain, colour) per entry
    col, pick, hit = choose_streams(nw, np.zeros(8, np.int32), [n_bytes] * 4, N)
    assert col.tolist() == [True, False, False, True]
    assert pick.tolist() == [1, 2, 4, 7]
    want = [fixed + 4 + 4 * 8 < n_bytes, fixed + 4 * 10 < n_bytes, True, True]
    assert hit.tolist() == want
    # small rectangles stay raw: 8 N bytes of state exceed a 5 x 5 x 3 entry at every N >= 16
    assert not is_packed([0], [0], [75], 16)[0]


def test_reference_costs_follow_the_rule():
    import colour_ref as cref
    p = cref.correlated(16, 16, 3)
    for N in (8, 16):
        kind, cost = wref.choice(p, N, colour=True)
        nw_p, nw_c = len(wref.encode(p, N)[3]), len(wref.encode(p, N, True)[3])
        plain, col = 8 + 8 * N + 4 * nw_p, 12 + 8 * N + 4 * nw_c
        best = min(plain, col)
        want = ("raw", p.size) if best >= p.size else (("colour", col) if col < plain else
                                                       ("plain", plain))
        assert (kind, cost) == want


# ------------------------------------------------------------------ the interface
def test_codec_and_model_take_predict_ways():
    from idfcodec import synthetic
    from idfcodec.configs import _dense, _flows
    model = synthetic.build_model(_flows("IDFlows", 2, 1, 8, 8, 3, _dense(8, 1), _dense(8, 1), 2))
    pc = predict.PredictiveTileCodec(model, max_batch=3)
    assert pc.predict_ways == 1 and pc.ways == 1
    pc = predict.PredictiveTileCodec(model, predict_ways=16, ways=8)
    assert pc.predict_ways == 16 and pc.ways == 8            # the two are independent
    for bad in (4, 128, 0, 2, "8"):
        with pytest.raises(ValueError, match="predict_ways"):
            predict.PredictiveTileCodec(model, predict_ways=bad)
    big = synthetic.build_model(_flows("IDFlows", 2, 1, 256, 256, 3, _dense(8, 1), _dense(8, 1),
                                       2))
    assert predict.PredictiveTileCodec(big).predict_ways == 1
    with pytest.raises(ValueError, match="LDS"):
        predict.PredictiveTileCodec(big, predict_ways=8)


def test_file_tool_reads_interleaved_files_by_magic():
    import importlib.util
    import os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pbs = _ways(_col(), 16)
    got, safe = tool.read_container(pbs.to_bytes(), None)
    assert safe and got.predict_ways == 16 and got.to_bytes() == pbs.to_bytes()
    args = tool.parser().parse_args(["bench", "--escape", "--predict", "--predict-ways", "8"]) \
        if hasattr(tool, "parser") else None
    assert args is None or args.predict_ways == 8
