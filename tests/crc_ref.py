"""A Python restatement of the CRC-32 identity csrc/idf_crc.h computes with (no device, no
library): values are polynomials over GF(2) mod P in the reflected representation, bit 31 the
coefficient of x^0.  test_integrity_host.py pins it to zlib on short inputs and uses it where
zlib cannot go (a second part of 2^33 bytes)."""
import zlib

POLY = 0xEDB88320
ONE = 0x80000000
X8 = 0x00800000


def mul(a: int, b: int) -> int:
    """a * b mod P"""
    p = 0
    for i in range(32):
        if a & (ONE >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow8(k: int) -> int:
    """x^(8 k) mod P"""
    r, b = ONE, X8
    while k:
        if k & 1:
            r = mul(r, b)
        b = mul(b, b)
        k >>= 1
    return r


def raw0(data: bytes) -> int:
    """The bitwise CRC with init 0 and no final XOR."""
    crc = 0
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (POLY if crc & 1 else 0)
    return crc


def frame(n: int) -> int:
    """What init and final XOR add to raw0 of n bytes."""
    return mul(0xFFFFFFFF, xpow8(n)) ^ 0xFFFFFFFF


def crc32_parts(data: bytes, cuts, order=None) -> int:
    """crc32(data) from its parts between the offsets `cuts` (sorted, inside the data), the
    parts taken in `order`."""
    n = len(data)
    edges = [0, *cuts, n]
    parts = list(zip(edges[:-1], edges[1:]))
    acc = 0
    for i in (order if order is not None else range(len(parts))):
        a, b = parts[i]
        acc ^= mul(raw0(data[a:b]), xpow8(n - b))
    return acc ^ frame(n)


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """crc32(a + b) from crc32(a), crc32(b) and len(b)."""
    return mul(crc_a, xpow8(len_b)) ^ crc_b


def crc32_zeros(n: int) -> int:
    """crc32 of n zero bytes: raw0 of zeros is 0."""
    return frame(n)


def tile_bytes(img, ty: int, tx: int, th: int, tw: int) -> bytes:
    """The in-image rectangle of tile (ty, tx) of a numpy image [C, H, W] as bytes [C][hin][win]."""
    return img[:, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].tobytes()


def tile_crcs(imgs, th: int, tw: int) -> list:
    """zlib.crc32 of every tile's source bytes, entry order (by image, tile row, tile column)."""
    out = []
    for img in imgs:
        _, H, W = img.shape
        out += [zlib.crc32(tile_bytes(img, ty, tx, th, tw))
                for ty in range(-(-H // th)) for tx in range(-(-W // tw))]
    return out
