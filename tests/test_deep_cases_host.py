"""tests/deep_cases.py's mechanics set, on the host.  No GPU.

First what the set covers, through tests/deep_ref.py alone: tests/test_gpu_deep_units.py runs the
device kernels over this set, and these assertions keep it from passing on units that have stopped
reaching the lines they were made for.  Then csrc/idf_deep.h's host model (idf_deep_prep_host,
idf_deep_decode_host) over the same units, as tests/test_deep_host.py does over its own."""
import numpy as np
import pytest

import deep_ref as R
from deep_cases import SHAPES, damage_units, damaged, mechanics_units, small_units


@pytest.fixture(scope="module")
def coded(oracle):
    """[(name, unit, class, model, state, words)] of the mechanics set, by deep_ref"""
    return [(name, u, *R.unit_class(u)) for name, u in mechanics_units()]


def nibbles(u, m):
    """the scale nibbles of the buckets present in unit u"""
    return {(m["sel"] >> (4 * int(k))) & 15 for k in np.unique(R.buckets(u, m["shift"]))}


def test_the_set_keeps_its_shapes_and_names():
    units = mechanics_units()
    assert len({name for name, _ in units}) == len(units)
    assert [u.shape for _, u in units[-len(SHAPES):]] == list(SHAPES)
    assert all(u.dtype == np.uint16 and u.ndim == 2 for _, u in units)
    again = mechanics_units()
    assert all(np.array_equal(u, v) for (_, u), (_, v) in zip(units, again))


def test_the_set_covers_what_it_is_meant_to(coded):
    packed = [c for c in coded if c[2] == R.PACKED]
    live = [c for c in coded if c[3] is not None]           # everything but the constant unit
    # every shift, each with refills of the low-bit window (64 words) for s >= 1
    assert {c[3]["shift"] for c in packed} == set(range(9))
    for s in range(9):
        name, u, k, m, _, words = coded[s]
        assert (name, k, m["shift"]) == (f"shift {s}", R.PACKED, s)
        assert len(words) > 2 * 128                         # the word window refills, and again
        assert len(m["low"]) == 72 * s
    for s in range(1, 9):
        assert any(c[3]["shift"] == s and len(c[3]["low"]) > 64 for c in packed), s
    assert any(len(c[5]) > 128 for c in packed)
    # every scale nibble among the buckets that are present; 0..13 from packed units
    assert set().union(*(nibbles(c[1], c[3]) for c in live)) == set(range(16))
    assert set(range(14)) <= set().union(*(nibbles(c[1], c[3]) for c in packed))
    # escapes: both signs, the first sample, the last sample, two side by side
    signs, first, last, pair = set(), False, False, False
    for _, u, _, m, _, _ in packed:
        em = m["esc_mask"]
        q, pq = u.astype(np.int64) >> m["shift"], R.predict(u)[0] >> m["shift"]
        signs |= set(np.sign((q - pq)[em]).tolist())
        first |= bool(em.flat[0])
        last |= bool(em.flat[-1])
        pair |= bool((em[:, 1:] & em[:, :-1]).any())
    assert signs == {-1, 1} and first and last and pair
    # long one-column and one-row units, the widest row the decoder holds
    assert any(u.shape[1] == 1 and u.size > 64 for _, u, *_ in packed)
    assert any(u.shape[0] == 1 and u.size > 64 for _, u, *_ in packed)
    from idfcodec import deep
    assert max(u.shape[1] for _, u, *_ in packed) == deep.tw_max()
    assert any(u.shape[0] > 1 and u.shape[1] == deep.tw_max() for _, u, *_ in packed)
    # every shape packs but the single sample, so the file tests decode them too
    for name, u, k, *_ in coded[-len(SHAPES):]:
        assert k == (R.CONSTANT if u.size == 1 else R.PACKED), name
    # what only a direct call decodes: units a file stores raw
    assert sum(c[2] == R.RAW for c in coded) >= 3


def test_prep_host_equals_the_reference_over_the_set(coded):
    from idfcodec import deep
    for name, u, _, m, _, _ in coded:
        want = m if m is not None else R.model(u)
        got = deep.host_prep(u)
        assert got["shift"] == want["shift"], name
        assert got["sel"] == want["sel"], name
        assert (got["min"], got["max"]) == (want["min"], want["max"]), name
        assert np.array_equal(got["esc"], want["esc"]), name
        assert np.array_equal(got["low"], want["low"]), name
        for k in ("x", "mean", "scale"):
            assert np.array_equal(got[k], want[k]), (name, k)


def test_decode_host_returns_the_samples_over_the_set(coded):
    from idfcodec import deep
    for name, u, _, m, state, words in coded:
        if m is None:
            m, state, words = R.encode(u)
        out, final, status = deep.host_decode(*u.shape, m["shift"], m["sel"], state, words,
                                              m["low"], m["esc"])
        assert status == 0 and final == R.L, name
        assert np.array_equal(out, u), name


def test_decode_host_equals_the_reference_on_damaged_units(oracle):
    """Every change of deep_cases.damaged on every unit of damage_units: samples, final state and
    status as deep_ref.decode gives them.  Between them the changes reach every flag."""
    from idfcodec import deep
    seen, changes = 0, set()
    for u in damage_units():
        for change, d in damaged(u, *R.encode(u), R.buckets):
            args = (d["shift"], d["sel"], d["state"], d["words"], d["low"], d["esc"])
            want = R.decode(*args, *u.shape)
            got = deep.host_decode(*u.shape, *args)
            assert (got[1], got[2]) == (want[1], want[2]), (u.shape, change)
            assert np.array_equal(got[0], want[0]), (u.shape, change)
            seen |= want[2]
            changes.add(change)
    assert seen & R.UNDERFLOW and seen & R.OUT_OF_WINDOW and seen & R.WORDS_LEFT
    assert len(changes) == 9


def test_small_units_are_the_host_tests_set():
    units = small_units()
    assert len(units) == 306 and max(u.size for u in units) <= 256
