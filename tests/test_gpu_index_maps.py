"""The index-map kernels one by one, against the oracle's restatements (oracle/flow_oracle.py and
oracle/vqvae_oracle.py, which tests/test_oracle_golden.py pins to the reference) or plain numpy:
idf_squeeze / idf_unsqueeze, idf_permute_couple_in, idf_copy_cols, idf_pm_to_nchw /
idf_nchw_to_pm, idf_quant_u8, idf_patch, idf_vq_gather, idf_vq_pointwise, idf_pack_bits /
idf_unpack_bits / idf_pack_bits_words, idf_gather_words.

Every comparison is exact.  A round trip cannot see a map that is wrong in a self-inverse way, so
each direction is compared with its reference on its own, on non-square geometries, with row
strides larger than the natural width; every destination has sentinel columns past the written
width and sentinel rows past P.  The argument rules of include/idf_codec.h (a NULL buffer, a row
stride below the columns touched) are tested by return code only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7777.25
ERR_ARG = 1


def dev():
    return torch.device("cuda")


def L():
    from idfcodec._lib import lib
    return lib()


def S():
    from idfcodec import _lib
    return _lib.stream_ptr()


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def sent(rows, cols):
    return torch.full((rows, cols), SENT, device=dev())


def values(*shape, seed=0):
    """Distinct values, so any misplaced element shows."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(n, generator=g).float() - n // 2).view(*shape)


def to_pm(x, ld, extra_rows=0, c0=0):
    """NCHW -> pixel-major [P + extra_rows][ld] with the channels at columns [c0, c0 + C) and the
    sentinel everywhere else."""
    B, C, H, W = x.shape
    pm = torch.full((B * H * W + extra_rows, ld), SENT)
    pm[:B * H * W, c0:c0 + C] = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return pm


def from_pm(pm, B, C, H, W, c0=0):
    return pm[:B * H * W, c0:c0 + C].reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def assert_margins(pm, P, C, c0=0):
    assert (pm[P:] == SENT).all(), "wrote rows past P"
    assert (pm[:, :c0] == SENT).all() and (pm[:, c0 + C:] == SENT).all(), "wrote outside the columns"


# ------------------------------------------------------------------ squeeze / unsqueeze
@pytest.mark.parametrize("B,H,W,C,s,window", [
    (3, 6, 10, 3, 2, 0), (2, 4, 12, 5, 4, 0), (2, 5, 7, 4, 1, 0), (1, 2, 2, 1, 2, 0),
    (3, 6, 10, 3, 2, 4)])
def test_squeeze_unsqueeze_vs_oracle(B, H, W, C, s, window):
    """idf_squeeze against FO.extend_fwd and idf_unsqueeze against FO.extend_bwd, each on its own;
    window = 4: the unsqueezed side is a column window of a wider buffer (pointer offset by 4
    columns)."""
    import flow_oracle as FO
    x = values(B, C, H, W, seed=H * W + C)
    Ho, Wo, Co = H // s, W // s, C * s * s
    P, Po = B * H * W, B * Ho * Wo
    ld_x, ld_y = C + window + 5, Co + 3
    y_ref = FO.extend_fwd(x, s)
    # forward
    src = to_pm(x, ld_x, 2, c0=window).to(dev())
    dst = sent(Po + 2, ld_y)
    ok(L().idf_squeeze(S(), B, H, W, C, s, ptr(src) + 4 * window, ld_x, ptr(dst), ld_y))
    dst = dst.cpu()
    assert_margins(dst, Po, Co)
    assert torch.equal(from_pm(dst, B, Co, Ho, Wo), y_ref)
    # backward, from the reference's squeezed tensor (not from the kernel's own output)
    y = values(B, Co, Ho, Wo, seed=7 + C)
    src = to_pm(y, ld_y, 2).to(dev())
    dst = sent(P + 2, ld_x)
    ok(L().idf_unsqueeze(S(), B, H, W, C, s, ptr(src), ld_y, ptr(dst) + 4 * window, ld_x))
    dst = dst.cpu()
    assert_margins(dst, P, C, c0=window)
    assert torch.equal(from_pm(dst, B, C, H, W, c0=window), FO.extend_bwd(y, s))


def test_squeeze_argument_rules():
    src, dst = sent(64, 16), sent(64, 16)
    for fn in (L().idf_squeeze, L().idf_unsqueeze):
        assert fn(S(), 1, 5, 4, 2, 2, ptr(src), 16, ptr(dst), 16) == ERR_ARG      # H % s
        assert fn(S(), 1, 4, 5, 2, 2, ptr(src), 16, ptr(dst), 16) == ERR_ARG      # W % s
        assert fn(S(), 1, 4, 4, 2, 0, ptr(src), 16, ptr(dst), 16) == ERR_ARG      # s = 0
        assert fn(S(), 1, 4, 4, 2, 2, None, 16, ptr(dst), 16) == ERR_ARG
        assert fn(S(), 1, 4, 4, 2, 2, ptr(src), 16, None, 16) == ERR_ARG
    # strides: the unsqueezed side holds C = 2 columns, the squeezed side C s^2 = 8
    assert L().idf_squeeze(S(), 1, 4, 4, 2, 2, ptr(src), 1, ptr(dst), 16) == ERR_ARG
    assert L().idf_squeeze(S(), 1, 4, 4, 2, 2, ptr(src), 16, ptr(dst), 7) == ERR_ARG
    assert L().idf_unsqueeze(S(), 1, 4, 4, 2, 2, ptr(src), 7, ptr(dst), 16) == ERR_ARG
    assert L().idf_unsqueeze(S(), 1, 4, 4, 2, 2, ptr(src), 16, ptr(dst), 1) == ERR_ARG
    torch.cuda.synchronize()
    assert (dst == SENT).all()


# ------------------------------------------------------------------ permute + coupling input
@pytest.mark.parametrize("C,a,a_pad,with_feat", [(12, 6, 16, True), (12, 3, 4, True),
                                                 (7, 3, 8, True), (12, 6, 16, False)])
def test_permute_couple_in_vs_oracle(C, a, a_pad, with_feat):
    """dst = FO.permute_fwd(src) for a random permutation; feat[:, :a] = dst[:, :a] and
    feat[:, a:a_pad] = 0 (a_pad above and below C; feat = NULL); the inverse permutation restores
    the source.  P = 300: the last block is ragged."""
    import flow_oracle as FO
    P = 300
    g = torch.Generator().manual_seed(C * 31 + a)
    ids = torch.randperm(C, generator=g)
    assert not torch.equal(ids, torch.arange(C))
    Pm = torch.zeros(C, C)
    Pm[torch.arange(C), ids] = 1.0                     # y = F.linear(x, Pm): y[:, i] = x[:, ids[i]]
    x = values(P, C, seed=C)
    ld_s, ld_d, ld_f = C + 1, C + 5, a_pad + 4
    src = torch.full((P + 2, ld_s), SENT)
    src[:P, :C] = x
    src = src.to(dev())
    dst, feat = sent(P + 2, ld_d), sent(P + 2, ld_f)
    ids_d = ids.to(torch.int32).to(dev())
    ok(L().idf_permute_couple_in(S(), P, C, ptr(ids_d), ptr(src), ld_s, ptr(dst), ld_d, a, a_pad,
                                 ptr(feat) if with_feat else None, ld_f))
    want = FO.permute_fwd(x, Pm)
    assert torch.equal(want, x[:, ids])
    dst_c, feat_c = dst.cpu(), feat.cpu()
    assert_margins(dst_c, P, C)
    assert torch.equal(dst_c[:P, :C], want)
    if with_feat:
        assert_margins(feat_c, P, a_pad)
        assert torch.equal(feat_c[:P, :a], want[:, :a]) and (feat_c[:P, a:a_pad] == 0).all()
    else:
        assert (feat_c == SENT).all()
    # the inverse permutation (what the decoder runs) restores the source
    inv = torch.empty_like(ids)
    inv[ids] = torch.arange(C)
    back = sent(P + 2, ld_s)
    inv_d = inv.to(torch.int32).to(dev())
    ok(L().idf_permute_couple_in(S(), P, C, ptr(inv_d), ptr(dst), ld_d,
                                 ptr(back), ld_s, 0, 0, None, 0))
    assert torch.equal(back.cpu()[:P, :C], x) and torch.equal(back.cpu()[:P, :C], FO.permute_bwd(want, Pm))
    assert_margins(back.cpu(), P, C)


def test_permute_couple_in_argument_rules():
    src, dst, feat = sent(8, 8), sent(8, 8), sent(8, 8)
    ids = torch.arange(4, dtype=torch.int32, device=dev())
    f = L().idf_permute_couple_in
    assert f(S(), 8, 4, None, ptr(src), 8, ptr(dst), 8, 2, 4, ptr(feat), 8) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), None, 8, ptr(dst), 8, 2, 4, ptr(feat), 8) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), ptr(src), 8, None, 8, 2, 4, ptr(feat), 8) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), ptr(src), 3, ptr(dst), 8, 2, 4, ptr(feat), 8) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), ptr(src), 8, ptr(dst), 3, 2, 4, ptr(feat), 8) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), ptr(src), 8, ptr(dst), 8, 2, 4, ptr(feat), 3) == ERR_ARG
    assert f(S(), 8, 4, ptr(ids), ptr(src), 8, ptr(dst), 8, 5, 4, ptr(feat), 8) == ERR_ARG
    torch.cuda.synchronize()
    assert (dst == SENT).all() and (feat == SENT).all()


# ------------------------------------------------------------------ copy_cols
@pytest.mark.parametrize("n,n_pad", [(5, 8), (8, 8), (0, 8)])
def test_copy_cols(n, n_pad):
    """dst[:, :n] = src[:, :n], zeros on to n_pad; n = 0 with src = NULL is the engine's zero fill
    and stays legal."""
    P = 300
    x = values(P, 9, seed=n)
    src = x.to(dev())
    dst = sent(P + 2, 12)
    ok(L().idf_copy_cols(S(), P, n, n_pad, ptr(src) if n else None, 9 if n else 0, ptr(dst), 12))
    d = dst.cpu()
    assert_margins(d, P, n_pad)
    assert torch.equal(d[:P, :n], x[:, :n]) and (d[:P, n:n_pad] == 0).all()


def test_copy_cols_argument_rules():
    src, dst = sent(8, 8), sent(8, 8)
    f = L().idf_copy_cols
    assert f(S(), 8, 4, 8, ptr(src), 8, None, 8) == ERR_ARG
    assert f(S(), 8, 4, 8, None, 8, ptr(dst), 8) == ERR_ARG     # n > 0 reads src
    assert f(S(), 8, 4, 8, ptr(src), 3, ptr(dst), 8) == ERR_ARG
    assert f(S(), 8, 4, 8, ptr(src), 8, ptr(dst), 7) == ERR_ARG
    assert f(S(), 8, -1, 8, ptr(src), 8, ptr(dst), 8) == ERR_ARG
    torch.cuda.synchronize()
    assert (dst == SENT).all()
    ok(f(S(), 8, 0, 8, None, 0, ptr(dst), 8))                   # the zero fill: IDF_OK
    assert (dst == 0).all()


# ------------------------------------------------------------------ pixel-major <-> NCHW
@pytest.mark.parametrize("C,ld", [(3, 4), (5, 8)])
def test_pm_nchw_vs_permute(C, ld):
    B, H, W = 3, 5, 7
    P, n, pad = B * H * W, B * C * H * W, 32
    x = values(B, C, H, W, seed=C)
    # pm -> nchw
    src = to_pm(x, ld, 1).to(dev())
    out = torch.full((pad + n + pad,), SENT, device=dev())
    ok(L().idf_pm_to_nchw(S(), B, C, H, W, ptr(src), ld, ptr(out) + 4 * pad))
    o = out.cpu()
    assert (o[:pad] == SENT).all() and (o[pad + n:] == SENT).all()
    assert torch.equal(o[pad:pad + n].view(B, C, H, W), x)
    # nchw -> pm
    dst = sent(P + 2, ld)
    xd = x.to(dev())
    ok(L().idf_nchw_to_pm(S(), B, C, H, W, ptr(xd), ptr(dst), ld))
    d = dst.cpu()
    assert_margins(d, P, C)
    assert torch.equal(d[:P, :C], x.permute(0, 2, 3, 1).reshape(P, C))
    # both round trips
    back = torch.empty(n, device=dev())
    ok(L().idf_pm_to_nchw(S(), B, C, H, W, ptr(dst), ld, ptr(back)))
    assert torch.equal(back.cpu().view(B, C, H, W), x)
    again = sent(P + 2, ld)
    ok(L().idf_nchw_to_pm(S(), B, C, H, W, ptr(out) + 4 * pad, ptr(again), ld))
    assert torch.equal(again.cpu(), d)


def test_pm_nchw_argument_rules():
    pm, nchw = sent(16, 4), torch.full((64,), SENT, device=dev())
    assert L().idf_pm_to_nchw(S(), 1, 3, 4, 4, None, 4, ptr(nchw)) == ERR_ARG
    assert L().idf_pm_to_nchw(S(), 1, 3, 4, 4, ptr(pm), 4, None) == ERR_ARG
    assert L().idf_pm_to_nchw(S(), 1, 3, 4, 4, ptr(pm), 2, ptr(nchw)) == ERR_ARG
    assert L().idf_nchw_to_pm(S(), 1, 3, 4, 4, None, ptr(pm), 4) == ERR_ARG
    assert L().idf_nchw_to_pm(S(), 1, 3, 4, 4, ptr(nchw), None, 4) == ERR_ARG
    assert L().idf_nchw_to_pm(S(), 1, 3, 4, 4, ptr(nchw), ptr(pm), 2) == ERR_ARG
    torch.cuda.synchronize()
    assert (pm == SENT).all() and (nchw == SENT).all()


# ------------------------------------------------------------------ quant_u8
def test_quant_u8_counts_and_clamps():
    """Known counts of off-grid values, exactly 128/256, negatives and values above 1: `bad` is
    their number and the bytes are the documented clamp; on-grid values invert idf_dequant_u8."""
    B, C, H, W, ld = 2, 3, 5, 7, 4
    n = B * C * H * W
    g = torch.Generator().manual_seed(3)
    k = torch.randint(0, 256, (n,), generator=g)
    k[:4] = torch.tensor([0, 127, 128, 255])
    v = (k + (k >= 128).long()).float() / 256          # the dequantised grid (never 128/256)
    want = k.clone()
    cases = [  # (position, value, byte)
        (10, 128 / 256, 128),          # the hole of the grid: m = 128 -> k = 128, counted
        (11, 128 / 256, 128),
        (20, 37.5 / 256, 38),          # off grid: rint to even 38 -> k = 38
        (21, 200.25 / 256, 199),       # off grid: m = 200 -> k = 199
        (22, 36.5 / 256, 36),          # off grid, tie to even
        (30, -1 / 256, 0),             # below: clamped to 0
        (31, -3.0, 0),
        (32, -0.4 / 256, 0),           # off grid and rounds to -0
        (40, 257 / 256, 255),          # above: m = 257 -> k = 256 -> clamped to 255
        (41, 2.0, 255),
        (42, 300 / 256, 255),
    ]
    for pos, val, byte in cases:
        v[pos], want[pos] = val, byte
    x = v.view(B, C, H, W)
    src = to_pm(x, ld, 1).to(dev())
    img = torch.full((n + 16,), 77, dtype=torch.uint8, device=dev())
    bad = torch.zeros(3, dtype=torch.int32, device=dev())
    bad[0], bad[2] = 0, -5
    ok(L().idf_quant_u8(S(), B, C, H, W, ptr(src), ld, ptr(img), ptr(bad) + 4))
    assert bad.cpu().tolist() == [0, len(cases), -5]
    assert torch.equal(img.cpu()[:n].long(), want) and (img.cpu()[n:] == 77).all()
    # 256/256 is on the grid (k = 255) and not counted
    assert want[3] == 255 and v[3] == 1.0
    # argument rules
    assert L().idf_quant_u8(S(), B, C, H, W, None, ld, ptr(img), ptr(bad)) == ERR_ARG
    assert L().idf_quant_u8(S(), B, C, H, W, ptr(src), ld, None, ptr(bad)) == ERR_ARG
    assert L().idf_quant_u8(S(), B, C, H, W, ptr(src), ld, ptr(img), None) == ERR_ARG
    assert L().idf_quant_u8(S(), B, C, H, W, ptr(src), 2, ptr(img), ptr(bad)) == ERR_ARG


# ------------------------------------------------------------------ patch
@pytest.mark.parametrize("B,C,H,W,h,w", [(2, 3, 6, 9, 3, 3), (1, 1, 4, 4, 4, 4), (3, 2, 8, 4, 2, 4)])
def test_patch_vs_oracle(B, C, H, W, h, w):
    import vqvae_oracle as VO
    n, pad = B * C * H * W, 16
    x = values(B, C, H, W, seed=h * w)
    out = torch.full((pad + n + pad,), SENT, device=dev())
    xd = x.to(dev())
    ok(L().idf_patch(S(), B, C, H, W, h, w, 0, ptr(xd), ptr(out) + 4 * pad))
    o = out.cpu()
    assert (o[:pad] == SENT).all() and (o[pad + n:] == SENT).all()
    want = VO.patch(x, h, w)
    assert torch.equal(o[pad:pad + n].view(want.shape), want)
    # the inverse, from its own reference input
    y = values(*want.shape, seed=5)
    out = torch.full((pad + n + pad,), SENT, device=dev())
    yd = y.to(dev())
    ok(L().idf_patch(S(), B, C, H, W, h, w, 1, ptr(yd), ptr(out) + 4 * pad))
    o = out.cpu()
    assert (o[:pad] == SENT).all() and (o[pad + n:] == SENT).all()
    assert torch.equal(o[pad:pad + n].view(B, C, H, W), VO.unpatch(y, H, W))
    assert torch.equal(VO.unpatch(want, H, W), x)


def test_patch_argument_rules():
    a, b = torch.full((64,), SENT, device=dev()), torch.full((64,), SENT, device=dev())
    assert L().idf_patch(S(), 1, 1, 6, 6, 4, 3, 0, ptr(a), ptr(b)) == ERR_ARG   # 6 % 4
    assert L().idf_patch(S(), 1, 1, 6, 6, 3, 4, 0, ptr(a), ptr(b)) == ERR_ARG
    assert L().idf_patch(S(), 1, 1, 6, 6, 0, 3, 0, ptr(a), ptr(b)) == ERR_ARG
    assert L().idf_patch(S(), 1, 1, 6, 6, 3, 3, 0, None, ptr(b)) == ERR_ARG
    assert L().idf_patch(S(), 1, 1, 6, 6, 3, 3, 1, ptr(a), None) == ERR_ARG
    torch.cuda.synchronize()
    assert (b == SENT).all()


# ------------------------------------------------------------------ VQ gather / pointwise
def test_vq_gather():
    P, D, lde, K, ldo = 77, 20, 24, 11, 23
    E = torch.full((K, lde), SENT)
    E[:, :D] = values(K, D, seed=1)
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, K, (P,), generator=g)
    idx[:6] = torch.tensor([0, K - 1, 3, 3, 0, K - 1])       # both ends and repeats
    out = sent(P + 2, ldo)
    idx_d = idx.to(torch.int32).to(dev())
    Ed = E.to(dev())
    ok(L().idf_vq_gather(S(), P, D, ptr(idx_d), ptr(Ed), lde, ptr(out), ldo))
    o = out.cpu()
    assert_margins(o, P, D)
    assert torch.equal(o[:P, :D], E[idx, :D])
    f = L().idf_vq_gather
    assert f(S(), P, D, None, ptr(Ed), lde, ptr(out), ldo) == ERR_ARG
    assert f(S(), P, D, ptr(idx_d), None, lde, ptr(out), ldo) == ERR_ARG
    assert f(S(), P, D, ptr(idx_d), ptr(Ed), lde, None, ldo) == ERR_ARG
    assert f(S(), P, D, ptr(idx_d), ptr(Ed), D - 1, ptr(out), ldo) == ERR_ARG
    assert f(S(), P, D, ptr(idx_d), ptr(Ed), lde, ptr(out), D - 1) == ERR_ARG


@pytest.mark.parametrize("source", ["tanh", "grid"])
@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_vq_pointwise_bit_exact(op, source):
    """Ops 0..3 against the same expression in numpy float32, bit for bit; C = 3 with ld = 4."""
    P, C, ld = 301, 3, 4
    g = torch.Generator().manual_seed(op * 2 + (source == "grid"))
    if source == "tanh":
        x, z = torch.tanh(torch.randn(P, C, generator=g)), torch.tanh(torch.randn(P, C, generator=g))
    else:
        x = torch.randint(0, 257, (P, C), generator=g).float() / 256
        z = torch.randint(-256, 257, (P, C), generator=g).float() / 256
    buf = lambda v: torch.cat((torch.cat((v, torch.full((P, ld - C), SENT)), 1),  # noqa: E731
                               torch.full((2, ld), SENT))).to(dev())
    xd, zd, y = buf(x), buf(z), sent(P + 2, ld)
    ok(L().idf_vq_pointwise(S(), P, C, op, ptr(xd), ld, ptr(zd) if op >= 2 else None,
                            ld if op >= 2 else 0, ptr(y), ld))
    f = np.float32
    xn, zn = x.numpy(), z.numpy()
    want = [lambda: (xn - f(0.5)) / f(0.5),
            lambda: np.rint((xn * f(0.5) + f(0.5)) * f(256.0)) / f(256.0),
            lambda: xn - zn, lambda: xn + zn][op]().astype(np.float32)
    yc = y.cpu()
    assert_margins(yc, P, C)
    assert np.array_equal(yc[:P, :C].numpy().view(np.uint32), want.view(np.uint32))


def test_vq_pointwise_argument_rules():
    x, z, y = sent(8, 4), sent(8, 4), sent(8, 4)
    f = L().idf_vq_pointwise
    assert f(S(), 8, 3, 4, ptr(x), 4, ptr(z), 4, ptr(y), 4) == ERR_ARG          # op = 4
    assert f(S(), 8, 3, -1, ptr(x), 4, ptr(z), 4, ptr(y), 4) == ERR_ARG
    assert f(S(), 8, 3, 2, ptr(x), 4, None, 4, ptr(y), 4) == ERR_ARG            # op 2 reads z
    assert f(S(), 8, 3, 3, ptr(x), 4, ptr(z), 2, ptr(y), 4) == ERR_ARG
    assert f(S(), 8, 3, 0, None, 4, None, 0, ptr(y), 4) == ERR_ARG
    assert f(S(), 8, 3, 0, ptr(x), 4, None, 0, None, 4) == ERR_ARG
    assert f(S(), 8, 3, 0, ptr(x), 2, None, 0, ptr(y), 4) == ERR_ARG
    assert f(S(), 8, 3, 0, ptr(x), 4, None, 0, ptr(y), 2) == ERR_ARG
    torch.cuda.synchronize()
    assert (y == SENT).all()


# ------------------------------------------------------------------ fixed-width index code
def pack_ref(idx, groups, per, bits):
    """The documented layout: run g starts at word g * ceil(per * bits / 32); index j of the run
    occupies bits [j * bits, (j + 1) * bits) of its little-endian uint32 run."""
    wpg = (per * bits + 31) // 32
    words = np.zeros(groups * wpg, np.uint32)
    for g in range(groups):
        acc = 0
        for j in range(per):
            acc |= (int(idx[g * per + j]) & ((1 << bits) - 1)) << (j * bits)
        for w in range(wpg):
            words[g * wpg + w] = (acc >> (32 * w)) & 0xFFFFFFFF
    return words


@pytest.mark.parametrize("bits,per", [(1, 37), (5, 13), (9, 11), (14, 7), (31, 5)])
def test_pack_unpack_bits_vs_numpy(bits, per):
    """Three groups whose per * bits is no multiple of 32 (each starts on its own word); indices
    with bits set above `bits` (masked); a garbage-filled word buffer with a sentinel word after
    it; unpack(pack(idx)) == idx & mask."""
    groups = 3
    assert (per * bits) % 32
    g = torch.Generator().manual_seed(bits)
    idx = torch.randint(0, 2 ** 31 - 1, (groups * per,), generator=g, dtype=torch.int64)
    idx[0], idx[1], idx[2] = 0, (1 << bits) - 1, 2 ** 31 - 1
    idx[3] = -1                                                   # every bit set
    mask = (1 << bits) - 1
    assert int((idx[4:] > mask).sum()) > 0 or bits == 31
    nw = int(L().idf_pack_bits_words(groups, per, bits))
    assert nw == groups * ((per * bits + 31) // 32)
    idx_d = idx.to(torch.int32).to(dev())
    words = torch.full((nw + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev())  # garbage
    words[nw] = 0x7EADBEEF
    ok(L().idf_pack_bits(S(), groups, per, bits, ptr(idx_d), ptr(words)))
    got = words.cpu().numpy().view(np.uint32)
    assert got[nw] == 0x7EADBEEF, "wrote past the packed words"
    want = pack_ref(idx.numpy() & 0xFFFFFFFF, groups, per, bits)
    assert np.array_equal(got[:nw], want)
    out = torch.full((groups * per + 1,), -9, dtype=torch.int32, device=dev())
    ok(L().idf_unpack_bits(S(), groups, per, bits, ptr(words), ptr(out)))
    o = out.cpu()
    assert o[-1] == -9
    assert torch.equal(o[:-1].long(), idx & mask)
    # unpack against the layout on its own: words from the reference packer
    ref_words = torch.from_numpy(want.view(np.int32)).to(dev())
    out2 = torch.full((groups * per,), -9, dtype=torch.int32, device=dev())
    ok(L().idf_unpack_bits(S(), groups, per, bits, ptr(ref_words), ptr(out2)))
    assert torch.equal(out2.cpu().long(), idx & mask)


def test_pack_bits_argument_rules():
    idx = torch.zeros(8, dtype=torch.int32, device=dev())
    words = torch.full((8,), 0x11111111, dtype=torch.int32, device=dev())
    for f in (L().idf_pack_bits, L().idf_unpack_bits):
        a, b = (ptr(idx), ptr(words)) if f is L().idf_pack_bits else (ptr(words), ptr(idx))
        assert f(S(), 2, 4, 0, a, b) == ERR_ARG
        assert f(S(), 2, 4, 32, a, b) == ERR_ARG
        assert f(S(), 2, 4, 5, None, b) == ERR_ARG
        assert f(S(), 2, 4, 5, a, None) == ERR_ARG
        assert f(S(), -1, 4, 5, a, b) == ERR_ARG
    torch.cuda.synchronize()
    assert (words == 0x11111111).all() and (idx == 0).all()


# ------------------------------------------------------------------ gather_words
def test_gather_words_vs_numpy():
    """Seven streams, two of zero words and one of more than 256 (several strides of the block),
    non-monotonic source offsets, compacted back to back; the sentinel after the last run stays."""
    nwords = np.array([5, 0, 300, 1, 0, 64, 17], np.int64)
    src_off = np.array([700, 50, 100, 690, 0, 420, 10], np.int64)   # non-monotonic, disjoint runs
    dst_off = np.concatenate(([0], np.cumsum(nwords)[:-1])).astype(np.int64)
    total = int(nwords.sum())
    rng = np.random.default_rng(4)
    src = rng.integers(0, 2 ** 32, 800, dtype=np.uint64).astype(np.uint32)
    dst = torch.full((total + 4,), 0x5EA7BEEF, dtype=torch.int32, device=dev())
    t = lambda a: torch.from_numpy(a).to(dev())  # noqa: E731
    so, nw, do, sr = t(src_off), t(nwords), t(dst_off), t(src.view(np.int32))
    ok(L().idf_gather_words(S(), 7, ptr(so), ptr(nw), ptr(do), ptr(sr), ptr(dst)))
    got = dst.cpu().numpy().view(np.uint32)
    want = np.concatenate([src[o:o + n] for o, n in zip(src_off, nwords)])
    assert np.array_equal(got[:total], want)
    assert (got[total:] == 0x5EA7BEEF).all(), "wrote past the last run"
    f = L().idf_gather_words
    assert f(S(), 7, None, ptr(nw), ptr(do), ptr(sr), ptr(dst)) == ERR_ARG
    assert f(S(), 7, ptr(so), None, ptr(do), ptr(sr), ptr(dst)) == ERR_ARG
    assert f(S(), 7, ptr(so), ptr(nw), None, ptr(sr), ptr(dst)) == ERR_ARG
    assert f(S(), -1, ptr(so), ptr(nw), ptr(do), ptr(sr), ptr(dst)) == ERR_ARG
