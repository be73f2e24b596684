"""What the tiled containers' parsers do with damaged files, pinned: every truncation and every
single changed byte of nine hand-made files (IDFT, IDFS, IDFP, IDFQ, IDFM, IDFD) either parses --
and then writes what its digest says, or refuses to be written -- or raises ValueError with the
text recorded.  tests/golden/container_outcomes.sha256 holds one digest a file over all its
outcomes; run as a script this module prints that file.  No GPU."""
import hashlib
import os

import pytest

from conftest import GOLDEN  # first: as a script, it is what puts the package on the path

import deep_ref
from test_planes_host import _hand
from test_predict_colour_host import _col
from test_predict_host import MIXED, PACKED, _pred
from test_safe_host import _safe
from test_tiled_host import _tiled


def _files() -> dict:
    """name -> (the container's class, its bytes)"""
    from idfcodec import deep, planes, predict, safe, tiled
    a, b, c = deep_ref.hand_images()        # test_deep_host.hand_files' two files
    return {
        "idft": (tiled.TiledBitstream, _tiled().to_bytes()),
        "idfs_mixed": (safe.SafeTiledBitstream, _safe(MIXED).to_bytes()),
        "idfs_all_raw": (safe.SafeTiledBitstream, _safe([True] * 6).to_bytes()),
        "idfp": (predict.PredictiveTiledBitstream, _pred(MIXED, PACKED).to_bytes()),
        "idfq": (predict.PredictiveTiledBitstream, _col().to_bytes()),
        "idfm_rgba": (planes.PlaneSetBitstream, _hand().to_bytes()),
        "idfm_grey_alpha_8_ways": (planes.PlaneSetBitstream, _hand(0, 2, 8).to_bytes()),
        "idfd_grey": (deep.DeepTiledBitstream, deep_ref.write_file([a, c], 8, 8)),
        "idfd_rgb": (deep.DeepTiledBitstream, deep_ref.write_file([b], 8, 8)),
    }


def _outcome(cls, buf: bytes) -> str:
    """Any exception but ValueError passes through and fails the test."""
    try:
        parsed = cls.from_bytes(buf)
    except ValueError as e:
        return "ValueError " + str(e)
    try:
        return "ok " + hashlib.sha256(parsed.to_bytes()).hexdigest()
    except ValueError as e:
        return "ok, unwritable: " + str(e)


def _outcomes(cls, buf: bytes):
    """-> (the outcome of every truncation buf[:n], the outcomes of every offset's byte b changed
    to b ^ 1, b ^ 0x80 and 0xFF)"""
    cut = [_outcome(cls, buf[:n]) for n in range(len(buf))]
    changed = [_outcome(cls, buf[:o] + bytes([v]) + buf[o + 1:])
               for o in range(len(buf)) for v in (buf[o] ^ 1, buf[o] ^ 0x80, 0xFF)]
    return cut, changed


def _digest(cut, changed) -> str:
    return hashlib.sha256("\n".join(cut + changed).encode()).hexdigest()


@pytest.fixture(scope="module")
def outcomes():
    return {name: _outcomes(cls, buf) for name, (cls, buf) in _files().items()}


def test_no_truncation_is_accepted(outcomes):
    for name, (cut, _) in outcomes.items():
        bad = [n for n, got in enumerate(cut) if not got.startswith("ValueError ")]
        assert not bad, f"{name}: the first {bad[:8]} bytes alone are accepted"


def test_outcomes_match_the_pinned_digests(outcomes):
    with open(os.path.join(GOLDEN, "container_outcomes.sha256")) as f:
        want = {name: digest for digest, name in (line.split() for line in f)}
    assert set(want) == set(outcomes)
    for name, (cut, changed) in outcomes.items():
        assert _digest(cut, changed) == want[name], name


if __name__ == "__main__":
    for name, (cls, buf) in _files().items():
        print(_digest(*_outcomes(cls, buf)), name)
