"""The fp32 GEMM (gemm_f32_kernel, flow_kernels.hip) through its three C entry points --
idf_conv1x1_f32 (every head mode), idf_conv3x3_f32, idf_conv3x3_fold_f32 -- one call at a time.

Reference and tolerance.  The reference is the same operation in float64 on the CPU, on the
unpadded slices.  The tolerance is derived, not tuned: per output element

    |got - ref| <= 2 (n + 2) 2^-24 (sum_k |a_k| |w_k| + |bias terms|)

with n the number of products (K, or 9 C for the 3x3) and the sum taken in float64 by a second
reference pass over |A| and |W|: the textbook bound for fp32 accumulation in any order (n fused
multiply-adds and the bias add), doubled because the MFMA's internal 4-term rounding is not
documented as round-to-nearest.  ReLU and LeakyReLU are 1-Lipschitz and keep the bound (one more
rounding for the Leaky slope).  The folded 3x3 adds its bias terms first (b3 + up to nine vtap, ten
roundings): 2 (9 C + 2) >= 76 of them are allowed on |bias terms|, so the same form holds.  A
kernel that drops a K chunk, a tap or a bias term misses the bound by orders of magnitude.  Every
test prints its largest error / bound ratio (DESIGN.md records them).

Buffers.  Outputs have extra columns (ld_out > N) and extra rows past P, prefilled with a sentinel
that must survive; A has NaN in columns [K, lda), which the kernel must not read; weights are
zero-padded as the ABI requires.

The tests run in file order: the last one asserts that together they launched every (BM, BN) tile
the dispatcher can pick, every IDF_EPI_* mode and both 3x3 forms."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -7777.25
NAN = float("nan")
LAUNCHED = set()                                   # (BM, BN) of every launch made here
RAN = {"epi": set(), "conv3": set(), "block": set()}


def dev():
    return torch.device("cuda")


def note(P, N):
    """Record the tile the dispatcher picks for a launch of P rows, N columns."""
    from idfcodec._lib import gemm_launch_info
    info = gemm_launch_info(P, N)
    LAUNCHED.add((info["BM"], info["BN"]))
    return info


def check_bound(got, ref, mag, n, what):
    bound = 2.0 * (n + 2) * U * mag
    err = (got.double() - ref).abs()
    pos = bound > 0
    ratio = (err[pos] / bound[pos]).max().item() if pos.any() else 0.0
    print(f"{what}: max |error| / bound = {ratio:.4f} (max |error| {err.max().item():.3e})")
    assert torch.isfinite(got).all(), what
    assert (err <= bound).all(), (what, ratio)
    return ratio


def act64(v, act):
    return {"ReLU": F.relu, "LeakyReLU": lambda t: F.leaky_relu(t, 0.01), "None": lambda t: t}[act](v)


def head_out(mode, out=None, ld_out=0, base=None, ld_base=0, n_mean=0, mean=None, logscale=None,
             scale=None):
    from idfcodec._lib import IdfHeadOut
    h = IdfHeadOut()
    h.mode, h.out, h.ld_out, h.base, h.ld_base = mode, out, ld_out, base, ld_base
    h.n_mean, h.mean, h.logscale, h.scale = n_mean, mean, logscale, scale
    return h


# ------------------------------------------------------------------ dense mode
def dense_problem(P, K, N, seed, ties=0):
    """A [P][K + 4] with NaN past K, W [n_alloc][round16(K)] and bias zero-padded.  ties > 0: the
    first `ties` rows are one-hot (column 0) and W[n, 0] = (2 m_n + 1) / 512, bias 0 on the even
    columns, so there acc + bias lands exactly on a rounding tie of the 1/256 grid."""
    from idfcodec._lib import gemm_launch_info
    from idfcodec.packing import round_up
    g = torch.Generator().manual_seed(seed)
    lda = K + 4
    A = torch.randn(P, lda, generator=g)
    ldw = round_up(K, 16)
    n_alloc = gemm_launch_info(P, N)["n_alloc_min"]
    W = torch.zeros(n_alloc, ldw)
    W[:N, :K] = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.zeros(n_alloc)
    bias[:N] = torch.randn(N, generator=g) * 0.1
    if ties:
        A[:ties] = 0.0
        A[:ties, 0] = 1.0
        m = torch.arange(N) // 2 - N // 4          # even and odd, negative and positive, on both
                                                   # the zero-bias (even) and the other columns
        W[:N, 0] = (2 * m + 1).float() / 512
        bias[0:N:2] = 0.0
    A[:, K:] = NAN
    return dict(P=P, K=K, N=N, A=A, lda=lda, W=W, ldw=ldw, n_alloc=n_alloc, bias=bias,
                ldo=round_up(N, 4) + 4)


def upload(pr):
    return pr["A"].to(dev()), pr["W"].to(dev()), pr["bias"].to(dev())


def conv1x1(pr, d, P=None, row0=0, head=None, out=None, geom=(1, 1, 1)):
    """idf_conv1x1_f32 over rows [row0, row0 + P) of the problem; returns the [P + 3][ldo] output
    (sentinel-filled) unless `head` names its own targets."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    P = pr["P"] if P is None else P
    Ad, Wd, bd = d
    note(P, pr["N"])
    if out is None and (head is None or not head.out):
        out = torch.full((P + 3, pr["ldo"]), SENT, device=dev())
    check(lib().idf_conv1x1_f32(_lib.stream_ptr(), P, pr["K"], pr["N"],
                                ptr(Ad) + 4 * row0 * pr["lda"], pr["lda"], ptr(Wd), pr["ldw"],
                                pr["n_alloc"], ptr(bd), ptr(out), pr["ldo"], *geom,
                                ctypes.byref(head) if head is not None else None), "conv1x1")
    torch.cuda.synchronize()
    return out


def assert_margins(out, P, N, what=""):
    assert (out[P:] == SENT).all(), f"{what}: wrote rows past P"
    assert (out[:, N:] == SENT).all(), f"{what}: wrote columns past N"


def dense_ref(pr, rows=slice(None)):
    K, N = pr["K"], pr["N"]
    A, W, b = pr["A"][rows, :K].double(), pr["W"][:N, :K].double(), pr["bias"][:N].double()
    return A @ W.T + b, A.abs() @ W.abs().T + b.abs()


@pytest.mark.parametrize("N,K,P", T.DENSE)
def test_dense_store_vs_fp64(N, K, P):
    """idf_conv1x1_f32, head = NULL (IDF_EPI_STORE), at the smallest shapes that reach each tile
    width, ragged tiles, short and multi-chunk K and both arms of the block remap."""
    pr = dense_problem(P, K, N, seed=N * 100003 + K * 101 + P)
    assert note(P, N)["BM"] == 64
    out = conv1x1(pr, upload(pr)).cpu()
    RAN["epi"].add("STORE")
    assert_margins(out, P, N)
    ref, mag = dense_ref(pr)
    check_bound(out[:P, :N], ref, mag, K, f"dense N={N} K={K} P={P}")


@pytest.mark.parametrize("bm,bn", sorted(t for t in T.ALL_TILES if t[0] > 64))
def test_dense_every_bm_and_bits_do_not_depend_on_it(bm, bn):
    """The taller row tiles, at the smallest P that selects each (plus 37 rows: a ragged last
    tile): the whole output within the float64 bound, and its first and last 100 rows bit for bit
    what two BM = 64 calls over those rows alone give -- the invariance (flow_kernels.hip: "every
    output's bits are identical for any BM") that lets a decoder at B = 1 read a B = 256 stream."""
    from idfcodec._lib import gemm_launch_info
    N, K = T.WIDEST_N[bn], T.BM_K
    P0 = T.first_p(bm, 1)
    assert gemm_launch_info(P0, N)["BM"] == bm and gemm_launch_info(P0 - 1, N)["BM"] < bm
    P = P0 + T.BM_RAGGED
    info = note(P, N)
    assert (info["BM"], info["BN"]) == (bm, bn) and P % bm
    pr = dense_problem(P, K, N, seed=bm * 1000 + bn)
    d = upload(pr)
    big = conv1x1(pr, d)
    for row0 in (0, P - 100):
        assert note(100, N)["BM"] == 64
        part = conv1x1(pr, d, P=100, row0=row0)
        assert (part[100:] == SENT).all() and (part[:, N:] == SENT).all()
        assert torch.equal(part[:100, :N].view(torch.int32),
                           big[row0:row0 + 100, :N].view(torch.int32)), (bm, bn, row0)
    big = big.cpu()
    assert_margins(big, P, N)
    ref, mag = dense_ref(pr)
    check_bound(big[:P, :N], ref, mag, K, f"dense BM={bm} BN={bn} P={P}")


# ------------------------------------------------------------------ 3x3 mode
def conv3_problem(B, H, W, C, N, seed):
    from idfcodec._lib import gemm_launch_info
    from idfcodec.packing import round_up
    g = torch.Generator().manual_seed(seed)
    P = B * H * W
    ld = C + 4
    X = torch.randn(P, ld, generator=g)
    X[:, C:] = NAN
    ldw = round_up(C, 16)
    n_alloc = gemm_launch_info(P, N)["n_alloc_min"]
    Wt = torch.zeros(n_alloc, 9, ldw)
    Wt[:N, :, :C] = torch.randn(N, 9, C, generator=g) / (9 * C) ** 0.5
    b3 = torch.zeros(n_alloc)
    b3[:N] = torch.randn(N, generator=g) * 0.1
    vt = torch.zeros(9, n_alloc)
    vt[:, :N] = torch.randn(9, N, generator=g) * 0.1
    bfull = b3.clone()
    for t in range(9):                             # fp32, tap order: the kernel's border loop
        bfull = bfull + vt[t]
    return dict(B=B, H=H, W=W, C=C, N=N, P=P, ld=ld, X=X, ldw=ldw, n_alloc=n_alloc, Wt=Wt, b3=b3,
                vt=vt, bfull=bfull, ldo=round_up(N, 4) + 4)


def conv3_upload(cs):
    return tuple(cs[k].to(dev()) for k in ("X", "Wt", "b3", "vt", "bfull"))


def conv3(cs, d, fold, act, B=None, img0=0):
    """idf_conv3x3_f32 / idf_conv3x3_fold_f32 over images [img0, img0 + B)."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    B = cs["B"] if B is None else B
    H, W, C, N = cs["H"], cs["W"], cs["C"], cs["N"]
    P = B * H * W
    note(P, N)
    Xd, Wd, b3d, vtd, bfd = d
    out = torch.full((P + 3, cs["ldo"]), SENT, device=dev())
    x = ptr(Xd) + 4 * img0 * H * W * cs["ld"]
    s = _lib.stream_ptr()
    if fold:
        check(lib().idf_conv3x3_fold_f32(s, B, H, W, C, x, cs["ld"], ptr(Wd), cs["ldw"],
                                         cs["n_alloc"], ptr(b3d), ptr(vtd), cs["n_alloc"], ptr(bfd),
                                         N, ptr(out), cs["ldo"], _lib.ACT[act], 0.01), "conv3x3 fold")
    else:
        check(lib().idf_conv3x3_f32(s, B, H, W, C, x, cs["ld"], ptr(Wd), cs["ldw"], cs["n_alloc"],
                                    ptr(b3d), N, ptr(out), cs["ldo"], _lib.ACT[act], 0.01), "conv3x3")
    torch.cuda.synchronize()
    RAN["conv3"].add("fold" if fold else "plain")
    return out


def conv3_ref(cs, fold, act, imgs=slice(None)):
    """float64 conv2d of the unpadded slices (and its |.| pass); fold: + the tap-mask bias of
    test_conv3x3_halo_kernel_vs_fp64.  Returns (ref, mag) as [B', H*W, N] pixel-major."""
    B, H, W, C, N = cs["B"], cs["H"], cs["W"], cs["C"], cs["N"]
    x4 = cs["X"][:, :C].double().view(B, H, W, C).permute(0, 3, 1, 2)[imgs]
    w4 = cs["Wt"][:N, :, :C].double().permute(0, 2, 1).reshape(N, C, 3, 3)
    b = cs["b3"][:N].double().view(1, -1, 1, 1)
    ref = F.conv2d(x4, w4, padding=1) + b
    mag = F.conv2d(x4.abs(), w4.abs(), padding=1) + b.abs()
    if fold:
        mask = F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64),
                        torch.eye(9, dtype=torch.float64).view(9, 1, 3, 3), padding=1)
        v = cs["vt"][:, :N].double()
        ref = ref + torch.einsum("tn,bthw->bnhw", v, mask)
        mag = mag + torch.einsum("tn,bthw->bnhw", v.abs(), mask)
    ref = act64(ref, act)
    pm = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], H * W, N)  # noqa: E731
    return pm(ref), pm(mag)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("B,H,W,C,N,act", T.CONV3)
def test_conv3x3_vs_fp64(B, H, W, C, N, act, fold):
    """idf_conv3x3_f32 and idf_conv3x3_fold_f32 at border-only images, H = 1, W = 1, a row tile
    that spans two images (neighbours must not leak across the image boundary), one interior
    pixel, several slabs and column tiles."""
    cs = conv3_problem(B, H, W, C, N, seed=B * 7919 + H * 131 + W * 17 + C)
    out = conv3(cs, conv3_upload(cs), fold, act).cpu()
    assert_margins(out, cs["P"], N)
    ref, mag = conv3_ref(cs, fold, act)
    n = 9 * C + (1 if act == "LeakyReLU" else 0)
    check_bound(out[:cs["P"], :N].reshape(B, H * W, N), ref, mag, n,
                f"conv3x3{' fold' if fold else ''} {B}x{H}x{W} C={C} N={N} {act}")


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("bm", [128, 256])
def test_conv3x3_large_p_and_bits_do_not_depend_on_batch(bm, fold):
    """The 3x3 mode on the taller row tiles (B = 64 at 64 x 64 is BM = 256; the first batch that
    lands on BM = 128): first and last image within the float64 bound, and bit for bit the B = 1
    (BM = 64) runs of those two images."""
    from idfcodec._lib import gemm_launch_info
    H, W, C, N = T.CONV3_LARGE
    B = T.CONV3_LARGE_B256 if bm == 256 else next(
        b for b in range(1, 65) if gemm_launch_info(b * H * W, N)["BM"] == 128)
    assert note(B * H * W, N)["BM"] == bm and gemm_launch_info(H * W, N)["BM"] == 64
    cs = conv3_problem(B, H, W, C, N, seed=bm + fold)
    d = conv3_upload(cs)
    big = conv3(cs, d, fold, "ReLU")
    assert (big[cs["P"]:] == SENT).all() and (big[:, N:] == SENT).all()
    for img in (0, B - 1):
        one = conv3(cs, d, fold, "ReLU", B=1, img0=img)
        assert (one[H * W:] == SENT).all() and (one[:, N:] == SENT).all()
        rows = slice(img * H * W, (img + 1) * H * W)
        assert torch.equal(one[:H * W, :N].view(torch.int32), big[rows, :N].view(torch.int32)), img
        ref, mag = conv3_ref(cs, fold, "ReLU", imgs=slice(img, img + 1))
        check_bound(big[rows, :N].cpu().reshape(1, H * W, N), ref, mag, 9 * C,
                    f"conv3x3{' fold' if fold else ''} BM={bm} B={B} image {img}")


def test_conv3x3_fold_argument_rule():
    """idf_conv3x3_fold_f32 with vtap or bfull NULL, or ldv < N, is IDF_ERR_ARG (return code
    only: nothing is launched)."""
    from idfcodec import _lib
    from idfcodec._lib import lib, ptr
    cs = conv3_problem(1, 4, 4, 8, 16, seed=1)
    Xd, Wd, b3d, vtd, bfd = conv3_upload(cs)
    out = torch.full((cs["P"], cs["ldo"]), SENT, device=dev())

    def call(vt, bf, ldv, o=ptr(out), x=ptr(Xd), w=ptr(Wd), b=ptr(b3d), ldo=cs["ldo"]):
        return lib().idf_conv3x3_fold_f32(_lib.stream_ptr(), 1, 4, 4, 8, x, cs["ld"], w, cs["ldw"],
                                          cs["n_alloc"], b, vt, ldv, bf, 16, o, ldo, 0, 0.01)
    assert call(None, ptr(bfd), cs["n_alloc"]) == 1
    assert call(ptr(vtd), None, cs["n_alloc"]) == 1
    assert call(ptr(vtd), ptr(bfd), 15) == 1
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"], o=None) == 1
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"], x=None) == 1
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"], w=None) == 1
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"], b=None) == 1
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"], ldo=15) == 1
    plain = lambda **k: lib().idf_conv3x3_f32(  # noqa: E731
        _lib.stream_ptr(), 1, 4, 4, 8, k.get("x", ptr(Xd)), cs["ld"], k.get("w", ptr(Wd)), cs["ldw"],
        k.get("n_alloc", cs["n_alloc"]), k.get("b", ptr(b3d)), 16, k.get("o", ptr(out)),
        k.get("ldo", cs["ldo"]), 0, 0.01)
    for bad in (dict(x=None), dict(w=None), dict(b=None), dict(o=None), dict(ldo=12),
                dict(n_alloc=15)):
        assert plain(**bad) == 1, bad
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert call(ptr(vtd), ptr(bfd), cs["n_alloc"]) == 0 and plain() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ epilogues
def np_round8(v):
    """rint(v * 256) / 256 in float32, half to even: round8 of flow_kernels.hip."""
    v = np.asarray(v, np.float32)
    return (np.rint(v * np.float32(256.0)) / np.float32(256.0)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


N_TIES = 5


@pytest.fixture(scope="module")
def epi_store():
    """{N: (problem, device tensors, v)}: the IDF_EPI_STORE run every epilogue test starts from
    (the accumulation is the same fixed chain in every epilogue; contraction is off)."""
    B, H, W = T.EPI_GEOM
    cache = {}

    def get(N):
        if N not in cache:
            pr = dense_problem(B * H * W, T.EPI_K, N, seed=4242 + N, ties=N_TIES)
            d = upload(pr)
            out = conv1x1(pr, d, geom=T.EPI_GEOM).cpu()
            assert_margins(out, pr["P"], N)
            ref, mag = dense_ref(pr)
            check_bound(out[:pr["P"], :N], ref, mag, T.EPI_K, f"epilogue STORE N={N}")
            cache[N] = (pr, d, out[:pr["P"], :N].numpy().copy())
        return cache[N]
    return get


@pytest.mark.parametrize("N", T.COUPLE_N)
def test_couple_epilogues_bit_exact(epi_store, N):
    """IDF_EPI_COUPLE_ADD / _SUB: bit for bit base +- rint(v * 256) / 256 in numpy float32 from the
    STORE run's own v, with base in a separate buffer (ld_base != ld_out) and in place; rows built
    to land exactly on ties pin half-to-even; ADD then SUB on a 1/256-grid base restores it."""
    from idfcodec import _lib
    from idfcodec._lib import ptr
    pr, d, v = epi_store(N)
    P = pr["P"]
    # the tie rows: v * 256 = m + 1/2 exactly on the zero-bias columns, m even and odd
    tie = v[:N_TIES, 0:N:2].astype(np.float64) * 256
    assert np.all(tie - np.floor(tie) == 0.5) and len({int(t) % 2 for t in np.floor(tie[0])}) == 2
    r = np_round8(v)
    assert np.array_equal(r[:N_TIES, 0:N:2] * 256, 2 * np.rint(tie / 2))  # ties went to even
    g = torch.Generator().manual_seed(N)
    ldb, ldo = N + 7, pr["ldo"]
    grid = (torch.randint(-1024, 1024, (P, N), generator=g).float() / 256)
    for name, base_vals in (("any", torch.randn(P, N, generator=g)), ("grid", grid)):
        base = torch.full((P + 3, ldb), SENT)
        base[:P, :N] = base_vals
        base_d = base.to(dev())
        for mode, sign in ((_lib.EPI_COUPLE_ADD, 1), (_lib.EPI_COUPLE_SUB, -1)):
            RAN["epi"].add("COUPLE_ADD" if sign > 0 else "COUPLE_SUB")
            want = (base_vals.numpy() + np.float32(sign) * r).astype(np.float32)
            # separate base
            out = torch.full((P + 3, ldo), SENT, device=dev())
            conv1x1(pr, d, geom=T.EPI_GEOM,
                    head=head_out(mode, ptr(out), ldo, ptr(base_d), ldb))
            out = out.cpu()
            assert_margins(out, P, N, name)
            assert np.array_equal(bits(out[:P, :N].numpy()), bits(want)), (name, sign)
            assert torch.equal(base_d.cpu(), base), "the epilogue wrote its base"
            # in place: base == out
            io = torch.full((P + 3, ldo), SENT)
            io[:P, :N] = base_vals
            io = io.to(dev())
            conv1x1(pr, d, geom=T.EPI_GEOM, head=head_out(mode, ptr(io), ldo, ptr(io), ldo))
            assert_margins(io.cpu(), P, N, name)
            assert np.array_equal(bits(io.cpu()[:P, :N].numpy()), bits(want)), (name, sign, "in place")
            if name == "grid":  # exact on the grid: the inverse coupling restores the base
                back = _lib.EPI_COUPLE_SUB if sign > 0 else _lib.EPI_COUPLE_ADD
                conv1x1(pr, d, geom=T.EPI_GEOM, head=head_out(back, ptr(io), ldo, ptr(io), ldo))
                assert torch.equal(io.cpu()[:P, :N], base_vals), sign


@pytest.mark.parametrize("n_mean", T.PRIOR_N_MEAN)
def test_prior_epilogue_bit_exact(epi_store, n_mean):
    """IDF_EPI_PRIOR: mean and logscale are the STORE columns transposed to NCHW, bit for bit;
    scale is idf_expf_glibc(logscale), bit for bit; sentinels around all three buffers."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    B, H, W = T.EPI_GEOM
    N = 2 * n_mean
    pr, d, v = epi_store(N)
    n, pad = B * n_mean * H * W, 64
    bufs = [torch.full((pad + n + pad,), SENT, device=dev()) for _ in range(3)]
    p = [ptr(b) + 4 * pad for b in bufs]
    conv1x1(pr, d, geom=T.EPI_GEOM,
            head=head_out(_lib.EPI_PRIOR, n_mean=n_mean, mean=p[0], logscale=p[1], scale=p[2]))
    RAN["epi"].add("PRIOR")
    for b in bufs:
        assert (b[:pad] == SENT).all() and (b[pad + n:] == SENT).all()
    mean, logscale, scale = (b[pad:pad + n].cpu().numpy() for b in bufs)
    nchw = lambda a: a.reshape(B, H * W, n_mean).transpose(0, 2, 1).reshape(-1)  # noqa: E731
    assert np.array_equal(bits(mean), bits(nchw(v[:, :n_mean])))
    assert np.array_equal(bits(logscale), bits(nchw(v[:, n_mean:])))
    want = torch.empty(n, device=dev())
    check(lib().idf_expf_glibc(_lib.stream_ptr(), n, p[1], ptr(want)), "expf")
    torch.cuda.synchronize()
    assert np.array_equal(bits(scale), bits(want.cpu().numpy()))
    e = np.exp(logscale.astype(np.float64))
    assert (np.abs(scale - e) <= 1e-6 * e).all()


def test_gemm_argument_checks(epi_store):
    """launch_gemm returns IDF_ERR_ARG before any launch for a NULL A, W or bias, a NULL output of
    the chosen epilogue, PRIOR with N != 2 n_mean, and ld_out (ld_base) < N.  Return codes only."""
    from idfcodec import _lib
    from idfcodec._lib import lib, ptr
    B, H, W = T.EPI_GEOM
    N = 6
    pr, (Ad, Wd, bd), _ = epi_store(N)
    P, ldo = pr["P"], pr["ldo"]
    out = torch.full((P, ldo), SENT, device=dev())
    nchw = [torch.full((B * 3 * H * W,), SENT, device=dev()) for _ in range(3)]

    def call(head=None, a=ptr(Ad), w=ptr(Wd), b=ptr(bd), o=ptr(out), ld=ldo, n_alloc=pr["n_alloc"],
             lda=pr["lda"], geom=T.EPI_GEOM):
        return lib().idf_conv1x1_f32(_lib.stream_ptr(), P, pr["K"], N, a, lda, w, pr["ldw"], n_alloc,
                                     b, o, ld, *geom,
                                     ctypes.byref(head) if head is not None else None)
    ERR = 1
    assert call(a=None) == ERR and call(w=None) == ERR and call(b=None) == ERR
    assert call(o=None) == ERR and call(ld=N - 1) == ERR and call(n_alloc=15) == ERR
    assert call(lda=pr["K"] - 4) == ERR
    assert call(head=head_out(_lib.EPI_STORE, None, 0), o=None) == ERR
    for mode in (_lib.EPI_COUPLE_ADD, _lib.EPI_COUPLE_SUB):
        assert call(head=head_out(mode, ptr(out), ldo, None, ldo)) == ERR          # base
        assert call(head=head_out(mode, None, ldo, ptr(out), ldo), o=None) == ERR  # out
        assert call(head=head_out(mode, ptr(out), N - 1, ptr(out), ldo)) == ERR    # ld_out
        assert call(head=head_out(mode, ptr(out), ldo, ptr(out), N - 1)) == ERR    # ld_base
        assert call(head=head_out(mode, ptr(out), ldo, ptr(out), ldo), a=None) == ERR
    m, ls, sc = (ptr(t) for t in nchw)
    pri = lambda **k: head_out(_lib.EPI_PRIOR, n_mean=k.get("n_mean", 3), mean=k.get("mean", m),  # noqa: E731
                               logscale=k.get("logscale", ls), scale=k.get("scale", sc))
    assert call(head=pri(mean=None)) == ERR and call(head=pri(logscale=None)) == ERR
    assert call(head=pri(scale=None)) == ERR
    assert call(head=pri(n_mean=2)) == ERR and call(head=pri(n_mean=6)) == ERR
    assert call(head=pri(), geom=(B, H, W + 1)) == ERR      # NCHW geometry that is not P rows
    assert call(head=pri(), w=None) == ERR
    torch.cuda.synchronize()
    assert (out == SENT).all() and all((t == SENT).all() for t in nchw)
    # and the same calls with every argument in place are fine (PRIOR needs no `out`)
    assert call() == 0 and call(head=pri(), o=None, ld=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ a whole block, plain path
def block_state(a, growth, depth, n_head, seed):
    from idfcodec.packing import growths
    g = torch.Generator().manual_seed(seed)
    sd, c = {}, a
    for i, gi in enumerate(growths(growth, depth)):
        sd[f"layers.{i}.layers.0.weight"] = torch.randn(c, c, 1, 1, generator=g) / c ** 0.5
        sd[f"layers.{i}.layers.0.bias"] = torch.randn(c, generator=g) * 0.1
        sd[f"layers.{i}.layers.1.weight"] = torch.randn(gi, c, 3, 3, generator=g) / (9 * c) ** 0.5
        sd[f"layers.{i}.layers.1.bias"] = torch.randn(gi, generator=g) * 0.1
        c += gi
    sd[f"layers.{depth}.weight"] = torch.randn(n_head, c, 1, 1, generator=g) / c ** 0.5
    sd[f"layers.{depth}.bias"] = torch.randn(n_head, generator=g) * 0.1
    return sd


def layer_bound(x, E, w1, b1, w3, b3):
    """A bound on |device - float64| of one DenseLayer's 3x3 output (before the 1-Lipschitz
    activation) for an input x (float64) known to within E: E carried through |W3| |W1|, plus the
    layer's own rounding, 2 (n + 2) 2^-24 times its |.| pass conv3(|W3|, conv1(|W1|, |x| + E) +
    |b1|) + |b3| with n = 10 c + 4.  That covers both forms: the 1x1 (c products) then the 3x3
    (9 c products) with the 1x1's error carried through |W3|, and their fold (9 c products of
    weights and per-tap biases that are float64 products rounded once to fp32)."""
    c = x.shape[1]
    h_abs = F.conv2d(F.conv2d(x.abs() + E, w1.abs(), b1.abs()), w3.abs(), b3.abs(), padding=1)
    return F.conv2d(F.conv2d(E, w1.abs()), w3.abs(), padding=1) + 2 * (10 * c + 6) * U * h_abs


def layer_params(sd, i):
    return tuple(sd[f"layers.{i}.layers.{j}.{k}"].double() for j in (0, 1) for k in ("weight", "bias"))


def block_bound(x, sd, depth, act):
    """A first-order bound on |device - float64 oracle| of a whole DenseBlock's head output:
    layer_bound carried from layer to layer (the |.| passes run on |x| + the bound so far), then
    the head's 2 (c + 2) 2^-24 form.  Rigorous but loose: it grows with the |weights| gain of every
    layer, where the values themselves do not, so the sharp checks are the per-layer ones."""
    x = x.double()
    E = torch.zeros_like(x)
    for i in range(depth):
        w1, b1, w3, b3 = layer_params(sd, i)
        h = F.conv2d(F.conv2d(x, w1, b1), w3, b3, padding=1)
        Eh = layer_bound(x, E, w1, b1, w3, b3)
        x, E = torch.cat((x, act64(h, act)), 1), torch.cat((E, Eh), 1)
    wh, bh = sd[f"layers.{depth}.weight"].double(), sd[f"layers.{depth}.bias"].double()
    return F.conv2d(E, wh.abs()) + 2 * (x.shape[1] + 2) * U * F.conv2d(x.abs() + E, wh.abs(), bh.abs())


@pytest.mark.parametrize("fold", [0, 1])
def test_dense_block_plain_path_vs_oracle(fold):
    """idf_dense_block_f32 with halo = wino = 0, depth 3, at (2, 7, 5): fold = 0 is the only route
    to idf_conv3x3_f32 through the block runner (1x1 then 3x3 per layer), fold = 1 runs
    idf_conv3x3_fold_f32.  With a STORE head:
    - the feature buffer and the head output are bit for bit what the same chain of direct calls
      (each checked against float64 above) gives;
    - every layer, teacher-forced on the device's own input features, is within layer_bound of
      oracle/flow_oracle.py dense_layer in float64, and the head within the GEMM bound;
    - the whole block is within block_bound of the oracle's dense_block.
    The COUPLE_ADD and PRIOR heads are bit for bit what their epilogues make of the STORE output."""
    import flow_oracle as FO
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    from idfcodec.engine import DeviceBlock
    from idfcodec.packing import pack_dense_block
    B, H, W = T.BLOCK_GEOM
    P, depth, a, n_head = B * H * W, T.BLOCK_DEPTH, 12, 20
    sd = block_state(a, 40, depth, n_head, seed=77)
    sd64 = {k: t.double() for k, t in sd.items()}
    pb = pack_dense_block(sd, "", depth, "ReLU", fold=bool(fold))
    geom = pb.geom
    db = DeviceBlock(pb, dev())
    db.desc.halo = 0
    assert (db.desc.fold, db.desc.wino, db.desc.bf16, db.desc.dx3) == (fold, 0, 0, 0)
    x = torch.randn(B, a, H, W, generator=torch.Generator().manual_seed(78))
    ld = geom.ld_feat + 4
    x_pm = x.permute(0, 2, 3, 1).reshape(P, a)
    s = _lib.stream_ptr()

    def fresh_feat():
        feat = torch.zeros(P + 2, ld)
        feat[P:] = SENT
        feat[:P, :a] = x_pm
        feat[:P, geom.width:] = SENT
        return feat.to(dev())

    def run(head):
        feat = fresh_feat()
        tmp = torch.full((P + 2, ld), NAN, device=dev())
        for i in range(depth):
            note(P, geom.g_pad)
            if not fold:
                note(P, geom.k_in[i])
        note(P, n_head)
        check(lib().idf_dense_block_f32(s, ctypes.byref(db.desc), B, H, W, ptr(feat), ld, ptr(tmp),
                                        ld, ctypes.byref(head)), "dense block")
        torch.cuda.synchronize()
        feat = feat.cpu()
        assert (feat[P:] == SENT).all() and (feat[:P, geom.width:] == SENT).all()
        assert torch.equal(feat[:P, :a], x_pm) and torch.isnan(tmp[P:]).all()
        return feat

    ldo = n_head + 4
    out = torch.full((P + 3, ldo), SENT, device=dev())
    feat = run(head_out(_lib.EPI_STORE, ptr(out), ldo))
    out = out.cpu()
    assert_margins(out, P, n_head)
    v = out[:P, :n_head]
    RAN["block"].add(fold)

    # the same chain by direct calls: bit for bit
    hand, tmp2 = fresh_feat(), torch.full((P + 2, ld), NAN, device=dev())
    act, g_pad = _lib.ACT["ReLU"], geom.g_pad
    for i in range(depth):
        c = geom.k_in[i]
        if fold:
            check(lib().idf_conv3x3_fold_f32(s, B, H, W, c, ptr(hand), ld, ptr(db.w3[i]), pb.ldw3[i],
                                             pb.g_alloc, ptr(db.b3[i]), ptr(db.vtap[i]), pb.g_alloc,
                                             ptr(db.bfull[i]), g_pad, ptr(hand) + 4 * c, ld, act,
                                             pb.slope), "fold")
            continue
        check(lib().idf_conv1x1_f32(s, P, c, c, ptr(hand), ld, ptr(db.w1[i]), pb.ldw1[i],
                                    pb.n1_alloc[i], ptr(db.b1[i]), ptr(tmp2), ld, B, H, W, None), "1x1")
        check(lib().idf_conv3x3_f32(s, B, H, W, c, ptr(tmp2), ld, ptr(db.w3[i]), pb.ldw3[i],
                                    pb.g_alloc, ptr(db.b3[i]), g_pad, ptr(hand) + 4 * c, ld, act,
                                    pb.slope), "3x3")
    out2 = torch.full((P + 3, ldo), SENT, device=dev())
    check(lib().idf_conv1x1_f32(s, P, geom.width, n_head, ptr(hand), ld, ptr(db.wh), pb.ldwh,
                                pb.nh_alloc, ptr(db.bh), ptr(out2), ldo, B, H, W, None), "head")
    torch.cuda.synchronize()
    assert torch.equal(hand.cpu().view(torch.int32), feat.view(torch.int32))
    assert torch.equal(out2.cpu().view(torch.int32), out.view(torch.int32))

    # every layer teacher-forced against the oracle's dense_layer, then the head
    nchw = lambda t: t.reshape(B, H, W, -1).permute(0, 3, 1, 2).double()  # noqa: E731
    c = a
    for i, gi in enumerate(geom.growth):
        xin = nchw(feat[:P, geom.positions(c)])
        ref = FO.dense_layer(xin, sd64, f"layers.{i}.", "ReLU")[:, c:]
        bound = layer_bound(xin, torch.zeros_like(xin), *layer_params(sd, i))
        k = geom.k_in[i]
        err = (nchw(feat[:P, k:k + gi]) - ref).abs()
        print(f"dense block fold={fold} layer {i}: max |error| / bound = "
              f"{(err / bound).max().item():.2e} (max |error| {err.max().item():.3e})")
        assert (err <= bound).all(), i
        assert (feat[:P, k + gi:k + g_pad] == 0).all(), "padding columns of a layer not zero"
        c += gi
    xin = nchw(feat[:P, geom.positions(c)])
    wh, bh = sd64[f"layers.{depth}.weight"], sd64[f"layers.{depth}.bias"]
    check_bound(nchw(v), F.conv2d(xin, wh, bh), F.conv2d(xin.abs(), wh.abs(), bh.abs()), c,
                f"dense block fold={fold} head")

    # the whole block against the oracle's dense_block
    ref = FO.dense_block(x.double(), sd64, "", depth, "ReLU")
    bound = block_bound(x, sd, depth, "ReLU")
    err = (nchw(v) - ref).abs()
    print(f"dense block fold={fold}: max |error| / bound = {(err / bound).max().item():.2e} "
          f"(max |error| {err.max().item():.3e})")
    assert (err <= bound).all()
    # COUPLE_ADD head
    base = torch.randint(-512, 512, (P, n_head), generator=torch.Generator().manual_seed(5)).float() / 256
    io = torch.full((P + 3, ldo), SENT)
    io[:P, :n_head] = base
    io = io.to(dev())
    run(head_out(_lib.EPI_COUPLE_ADD, ptr(io), ldo, ptr(io), ldo))
    io = io.cpu()
    assert_margins(io, P, n_head)
    assert np.array_equal(bits(io[:P, :n_head].numpy()), bits(base.numpy() + np_round8(v.numpy())))
    # PRIOR head
    n_mean = n_head // 2
    n, pad = B * n_mean * H * W, 64
    bufs = [torch.full((pad + n + pad,), SENT, device=dev()) for _ in range(3)]
    p = [ptr(b) + 4 * pad for b in bufs]
    run(head_out(_lib.EPI_PRIOR, n_mean=n_mean, mean=p[0], logscale=p[1], scale=p[2]))
    for b in bufs:
        assert (b[:pad] == SENT).all() and (b[pad + n:] == SENT).all()
    flat = lambda t: t.reshape(B, H * W, n_mean).transpose(0, 2, 1).reshape(-1)  # noqa: E731
    assert np.array_equal(bits(bufs[0][pad:pad + n].cpu().numpy()), bits(flat(v[:, :n_mean].numpy())))
    assert np.array_equal(bits(bufs[1][pad:pad + n].cpu().numpy()), bits(flat(v[:, n_mean:].numpy())))
    want = torch.empty(n, device=dev())
    check(lib().idf_expf_glibc(_lib.stream_ptr(), n, p[1], ptr(want)), "expf")
    torch.cuda.synchronize()
    assert torch.equal(bufs[2][pad:pad + n].view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ coverage
def test_every_dispatcher_variant_ran():
    """The tests above (the module runs in file order) launched every (BM, BN) tile launch_bn can
    pick, every IDF_EPI_* mode, the 3x3 mode plain and folded, and both block forms."""
    assert LAUNCHED == T.ALL_TILES, sorted(T.ALL_TILES - LAUNCHED)
    assert RAN["epi"] == {"STORE", "COUPLE_ADD", "COUPLE_SUB", "PRIOR"}
    assert RAN["conv3"] == {"plain", "fold"}
    assert RAN["block"] == {0, 1}
