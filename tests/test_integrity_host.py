"""The seal of the tiled containers on the host (no device): the library's host CRC-32 helpers
and csrc/idf_crc.h itself against zlib, the Python restatement of the identity (tests/crc_ref.py)
against zlib, and the IDFC container: layout, frozen bytes, size, and every refusal of its
reader."""
import ctypes
import hashlib
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import crc_ref
from conftest import PKG, REPO

LENGTHS = [*range(0, 71), 255, 256, 257, 4095, 4096, 4097, (1 << 20) + 3]


# ------------------------------------------------------------------ the CRC core
def test_reference_restatement_equals_zlib():
    """crc_ref on short inputs: parts at random cuts taken in shuffled order, combine, and the
    CRC of a run of zero bytes."""
    rng = np.random.default_rng(11)
    for n in [*range(0, 40), 63, 64, 65, 255, 256, 257, 300]:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        want = zlib.crc32(data)
        assert crc_ref.crc32_parts(data, []) == want, n
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 6))))
        order = [int(i) for i in rng.permutation(len(cuts) + 1)]
        assert crc_ref.crc32_parts(data, cuts, order) == want, (n, cuts, order)
        k = int(rng.integers(0, n + 1))
        assert crc_ref.combine(zlib.crc32(data[:k]), zlib.crc32(data[k:]), n - k) == want
        assert crc_ref.crc32_zeros(n) == zlib.crc32(bytes(n))
    assert crc_ref.crc32_zeros(1 << 20) == zlib.crc32(bytes(1 << 20))


def test_host_crc_equals_zlib_at_every_length_and_offset():
    from idfcodec._lib import lib
    L = lib()
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, (1 << 20) + 3 + 8, dtype=np.uint8)
    raw = buf.tobytes()
    base = buf.ctypes.data
    for off in range(8):
        for n in LENGTHS:
            assert L.idf_crc32_host(base + off, n) == zlib.crc32(raw[off:off + n]), (off, n)
    assert L.idf_crc32_host(None, 0) == 0 and L.idf_crc32_host(base, -5) == 0


def test_host_combine_equals_zlib_of_the_concatenation():
    from idfcodec._lib import lib
    L = lib()
    rng = np.random.default_rng(13)
    splits = [(0, 0), (0, 17), (17, 0), (1, 1)]
    while len(splits) < 200:
        splits.append((int(rng.integers(0, 5000)), int(rng.integers(0, 5000))))
    for na, nb in splits:
        a = rng.integers(0, 256, na, dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, nb, dtype=np.uint8).tobytes()
        assert L.idf_crc32_combine(zlib.crc32(a), zlib.crc32(b), nb) == zlib.crc32(a + b), (na, nb)
    # a second part too long to build: zero bytes, against the restated identity
    a = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    for nb in (1 << 20, (1 << 31) + 5, 1 << 32, (1 << 33) - 1, 1 << 33):
        zeros = crc_ref.crc32_zeros(nb)
        want = crc_ref.combine(zlib.crc32(a), zeros, nb)
        assert L.idf_crc32_combine(zlib.crc32(a), zeros, nb) == want, nb
        # and the run of zeros alone, as two halves
        assert L.idf_crc32_combine(crc_ref.crc32_zeros(nb - nb // 2),
                                   crc_ref.crc32_zeros(nb // 2), nb // 2) == zeros, nb
    assert want != zlib.crc32(a)
    assert L.idf_crc32_combine(zlib.crc32(a), crc_ref.crc32_zeros(1 << 20), 1 << 20) == \
        zlib.crc32(a + bytes(1 << 20))


def _host_compiler():
    for cc in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_header_compiles_alone_on_the_host_and_equals_zlib(tmp_path):
    """csrc/idf_crc.h without hipcc: tests/crc_host_check.cpp, every line against zlib."""
    exe = str(tmp_path / "crc_host_check")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "crc_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    i = np.arange((1 << 20) + 3 + 8, dtype=np.int64)
    raw = ((i * 131 + 89) % 251).astype(np.uint8).tobytes()
    lines = [ln.split() for ln in out if ln]
    assert [(int(o), int(n)) for o, n, _ in lines] == [(o, n) for o in range(8) for n in LENGTHS]
    for o, n, c in lines:
        assert int(c, 16) == zlib.crc32(raw[int(o):int(o) + int(n)]), (o, n)


# ------------------------------------------------------------------ the IDFC container
SIZES = [(1, 1), (17, 16), (5, 40)]     # 1 + 2 + 3 tiles at 16x16
RECTS = [(1, 1), (16, 16), (1, 16), (5, 16), (5, 16), (5, 8)]
C = 3
RAW = [C * h * w for h, w in RECTS]
MIXED = [True, False, True, False, False, True]
CRCS = [0xDEADBEEF, 0, 1, 0x80000000, 0xFFFFFFFF, 0x12345678]
FP = 0xA1B2C3D4


def _hand_bitstream(N, n_lvl=2, ways=1):
    """Stream (l, e) holds nw = (3 * l + e) % 4 words of value 100 * (l * N + e) + j."""
    from idfcodec.codec import Bitstream
    nw = [(3 * l + e) % 4 for l in range(n_lvl) for e in range(N)]
    words = [100 * k + j for k, n in enumerate(nw) for j in range(n)]
    states = [(1 << 32) + k for k in range(n_lvl * N * ways)]
    t = lambda a, dt: torch.tensor(a, dtype=dt)  # noqa: E731
    return Bitstream(N, [(6, 8, 8), (12, 4, 4)][:n_lvl], t(states, torch.int64),
                     t(nw, torch.int64), t(words, torch.int32),
                     meta={"n_subpixels": N * 3 * 16 * 16, "conv": "f32"},
                     host_nwords=t(nw, torch.int64), ways=ways)


def _tiled():
    from idfcodec.tiled import TiledBitstream
    return TiledBitstream(_hand_bitstream(6), list(SIZES), C, (16, 16))


def _safe(escaped=MIXED):
    """A SafeTiledBitstream over SIZES: raw byte j of escaped entry e is (7 * e + j) % 251."""
    from idfcodec.safe import SafeTiledBitstream
    escaped = np.asarray(escaped, dtype=bool)
    K = int((~escaped).sum())
    raw = [np.arange(RAW[e], dtype=np.int64) + 7 * e for e in range(6) if escaped[e]]
    raw = (np.concatenate(raw) % 251).astype(np.uint8) if raw else np.zeros(0, np.uint8)
    return SafeTiledBitstream(_hand_bitstream(K) if K else None, list(SIZES), C, (16, 16),
                              escaped, torch.from_numpy(raw))


def _sealed(inner):
    from idfcodec.integrity import SealedBitstream
    return SealedBitstream(inner, np.array(CRCS, dtype=np.uint32), FP)


INNERS = [_tiled, _safe, lambda: _safe([True] * 6), lambda: _safe([False] * 6)]


@pytest.mark.parametrize("make", INNERS)
def test_idfc_round_trip_layout_and_size(make):
    from idfcodec.integrity import OVERHEAD, SealedBitstream
    inner = make()
    body = inner.to_bytes()
    buf = _sealed(inner).to_bytes()
    head = (struct.pack("<4sHHII", b"IDFC", 1, 0, FP, 6) + struct.pack("<6I", *CRCS)
            + struct.pack("<Q", len(body)))
    assert buf == head + struct.pack("<I", zlib.crc32(head)) + body
    assert len(buf) == len(body) + 28 + 4 * 6 and OVERHEAD == 28
    back = SealedBitstream.from_bytes(buf)
    assert type(back.inner) is type(inner) and back.inner.to_bytes() == body
    assert back.crc.dtype == np.uint32 and back.crc.tolist() == CRCS and back.fingerprint == FP
    assert back.to_bytes() == buf
    assert back.layout.n_tiles == 6


def test_idfc_bytes_are_frozen():
    assert hashlib.sha256(_sealed(_tiled()).to_bytes()).hexdigest() == \
        "48e531fadab0c919194b8df6c55d35e7317326be2e7c8008711557247390456e"
    assert hashlib.sha256(_sealed(_safe()).to_bytes()).hexdigest() == \
        "3ec86c8a1ce1b079495c5c556ae217f4b097679028d7e68fbc7fa329fbf2aeef"


def _patched(raw, fmt, offset, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def _resealed(raw, n_tiles=6):
    """raw with its header CRC computed anew: what a writer of such a header would store."""
    o = 16 + 4 * n_tiles + 8
    return _patched(raw, "<I", o, zlib.crc32(raw[:o]))


def _flipped(raw, byte, bit=0):
    b = bytearray(raw)
    b[byte] ^= 1 << bit
    return bytes(b)


@pytest.mark.parametrize("make", [_tiled, _safe])
def test_idfc_errors(make):
    from idfcodec.integrity import SealedBitstream
    raw = _sealed(make()).to_bytes()
    o_len, o_crc, o_inner = 16 + 24, 16 + 24 + 8, 16 + 24 + 12
    n_inner = len(raw) - o_inner
    cases = {
        "magic": (_patched(raw, "<4s", 0, b"IDFT"), "not an IDF"),
        "version": (_resealed(_patched(raw, "<H", 4, 2)), "version"),
        "flags": (_resealed(_patched(raw, "<H", 6, 1)), "flags"),
        "truncated header": (raw[:15], "truncated"),
        "truncated crcs": (raw[:o_crc + 3], "truncated"),
        "truncated inner": (raw[:-1], "inner bytes"),
        "empty inner": (raw[:o_inner], "inner bytes"),
        "trailing": (raw + b"\0", "inner bytes"),
        # one flipped bit in each header field: the header CRC sees it
        "fingerprint bit": (_flipped(raw, 8, 3), "header's CRC"),
        "n_tiles bit": (_flipped(raw, 12, 0), None),
        "tile crc bit": (_flipped(raw, 16 + 4 * 2 + 1, 7), "header's CRC"),
        "inner length bit": (_flipped(raw, o_len, 0), "header's CRC"),
        "inner length high bit": (_flipped(raw, o_len + 7, 7), "header's CRC"),
        "header crc bit": (_flipped(raw, o_crc, 5), "header's CRC"),
        # consistent headers that do not fit what follows
        "inner magic": (raw[:o_inner] + b"IDFB" + raw[o_inner + 4:], "unknown magic"),
        "longer inner length": (_resealed(_patched(raw, "<Q", o_len, n_inner + 1)),
                                "inner bytes"),
        "shorter inner length": (_resealed(_patched(raw, "<Q", o_len, n_inner - 1)),
                                 "inner bytes"),
    }
    for name, (buf, match) in cases.items():
        with pytest.raises(ValueError, match=match):
            SealedBitstream.from_bytes(buf)
    # n_tiles that differs from the inner layout's: 5 CRCs before an inner file of 6 tiles
    head = (struct.pack("<4sHHII", b"IDFC", 1, 0, FP, 5) + struct.pack("<5I", *CRCS[:5])
            + struct.pack("<Q", n_inner))
    with pytest.raises(ValueError, match="5 tile CRCs, its inner file 6"):
        SealedBitstream.from_bytes(head + struct.pack("<I", zlib.crc32(head)) + raw[o_inner:])
    # inner damage is the inner reader's to report
    with pytest.raises(ValueError):
        SealedBitstream.from_bytes(_patched(raw, "<H", o_inner + 4, 9))
    # the writer refuses a CRC list of another length
    from idfcodec.integrity import SealedBitstream as S
    with pytest.raises(ValueError, match="5 tile CRCs for 6"):
        S(make(), np.array(CRCS[:5], dtype=np.uint32), FP).to_bytes()


def test_sealed_codec_wraps_tiled_codecs_only():
    from idfcodec import integrity
    with pytest.raises(TypeError):
        integrity.SealedCodec(torch.nn.Identity())
    with pytest.raises(Exception):      # no CPU fallback: the device calls take device tensors
        integrity.device_crc32_segments(torch.zeros((1, 2), dtype=torch.int64), 1,
                                        torch.zeros(1, dtype=torch.int32))


def test_file_tool_reads_sealed_files_by_magic():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "bench_tiled", os.path.join(REPO, "tools", "bench_tiled.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from idfcodec.integrity import SealedBitstream
    from idfcodec.safe import SafeTiledBitstream
    for inner, is_safe in ((_tiled(), False), (_safe(), True)):
        buf = _sealed(inner).to_bytes()
        got, escape, sealed = tool.read_file(buf, None)
        assert sealed and escape == is_safe and isinstance(got, SealedBitstream)
        assert got.to_bytes() == buf
        got, escape, sealed = tool.read_file(inner.to_bytes(), None)
        assert not sealed and escape == is_safe
        assert isinstance(got, SafeTiledBitstream) == is_safe
