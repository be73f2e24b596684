"""The dx3 kernels' per-layer fixed costs (conv3_dx3.hip: the prologue's halo plan, the zero quads
of the split copy stored ahead of the slab loop, the fused DenseBlock kernel's per-layer set-up)
change no bit:

* the fast halo plan (a tile inside one image: the 16-wide canvas) against the generic plan
  (IDF_DX3_PLAN=generic, read at every launch) -- every byte of the fp32 outputs, of the written
  split copy and of the head's running sums, over NaN-poisoned buffers;
* the fused DenseBlock launch against the per-layer launches, for blocks of 1, 2, 3 and 12 layers,
  fused and GEMM heads, split-f16 and bf16, over a NaN-poisoned scratch buffer;
* the 12-layer fused block beside another stream's 32 x 32 launches."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_dx3 as T

pytestmark = pytest.mark.gpu

F16_NAN = T.F16_NAN


def layer_with_head(B, H, W, C, N, nh, generic):
    """split_cols + head_init + one dx3 layer that adds its share to the head's running sums,
    over poisoned buffers.  Returns the bytes of (out, split copy, hacc) and the range flag."""
    from idfcodec import _lib
    from idfcodec._lib import IdfDx3Head, check, lib, ptr
    from idfcodec.packing import dx3_groups, dx3_weights
    dev = torch.device("cuda")
    cs = T.make_case(B, H, W, C, N, fold=True, seed=B * 13 + H + C)
    P, ld, n_alloc = B * H * W, cs["ld"], cs["n_alloc"]
    nf, ngroup = dx3_groups(n_alloc)
    Wd, ysc = dx3_weights(cs["Wt"].numpy(), C)
    Wdd = torch.from_numpy(Wd.view(np.int16)).to(dev)
    Xd, b3d, vtd, bfd = (cs[k].to(dev) for k in ("X", "b3", "vt", "bfull"))
    g = torch.Generator().manual_seed(nh + C)
    ldwh = T.round_up_16(C + N)
    whd = (torch.randn(nh, ldwh, generator=g) / np.sqrt(C + N)).to(dev)
    bhd = (torch.randn(nh, generator=g) * 0.1).to(dev)
    nslab = (C + N + 15) // 16 + 1  # one slab past the layer's: stays poisoned
    xs = torch.full((nslab * 2 * P * 16,), F16_NAN, dtype=torch.int16, device=dev)
    out = torch.full((P, ld), float("nan"), device=dev)
    acc = torch.full((P * 16,), float("nan"), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, wsb, ctr = T.dx3_workspace(B, H, W, C, N, dev)
    s = _lib.stream_ptr()
    old = os.environ.pop("IDF_DX3_PLAN", None)
    if generic:
        os.environ["IDF_DX3_PLAN"] = "generic"
    try:
        check(lib().idf_dx3_split_cols(s, P, 0, C, ptr(Xd), ld, ptr(xs), nslab, ptr(flag), None, 0),
              "split")
        check(lib().idf_dx3_head_init(s, P, min(C, 64) // 4 * 4, ptr(Xd), ld, ptr(whd), ldwh,
                                      ptr(bhd), nh, ptr(acc)), "head init")
        hd = IdfDx3Head()
        hd.w, hd.ldw, hd.n_head, hd.acc, hd.last, hd.skip_f32 = ptr(whd), ldwh, nh, ptr(acc), 0, 0
        check(lib().idf_conv3x3_dx3(s, B, H, W, C, ptr(xs), nslab, ptr(Wdd), nf * ngroup, ysc,
                                    ptr(b3d), ptr(vtd), n_alloc, ptr(bfd), N, ptr(out), ld,
                                    _lib.ACT["ReLU"], 0.01, ptr(flag), ptr(ws), wsb,
                                    ctypes.byref(hd)), "dx3")
        torch.cuda.synchronize()
    finally:
        os.environ.pop("IDF_DX3_PLAN", None)
        if old is not None:
            os.environ["IDF_DX3_PLAN"] = old
    if ws is not None:
        assert not ws[:ctr // 4].any(), "dx3 left a split-K counter non-zero"
    return (out.view(torch.int32).cpu(), xs.cpu(), acc.view(torch.int32).cpu(), int(flag.item()), cs,
            nslab)


# (B, H, W, C, N, launch shape): one-tile blocks, two-tile blocks (even and odd tile counts),
# split K with a partly filled tile -- where the fast plan does not apply both runs are generic
PLAN_CASES = [
    (2, 32, 32, 16, 44, dict(pitch=18, T=1)), (2, 32, 32, 60, 44, dict(pitch=18, T=1)),
    (128, 32, 32, 60, 44, dict(pitch=18, T=2, ntiles=512)),
    (513, 16, 16, 16, 44, dict(pitch=18, T=2, ntiles=513)),
    (5, 8, 8, 36, 44, dict(pitch=10, T=1, nchunk=3)),
]


@pytest.mark.parametrize("B,H,W,C,N,sel", PLAN_CASES)
def test_fast_plan_equals_generic_plan(B, H, W, C, N, sel):
    from idfcodec._lib import dx3_launch_info
    info = dx3_launch_info(B, H, W, C, N)
    assert all(info[k] == v for k, v in sel.items()), info
    fast = layer_with_head(B, H, W, C, N, 12, generic=False)
    gen = layer_with_head(B, H, W, C, N, 12, generic=True)
    for name, a, b in zip(("out", "split copy", "hacc"), fast[:3], gen[:3]):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert fast[3] == gen[3] == 0
    out, xs, acc, _, cs, nslab = fast
    P = B * H * W
    # what a layer writes, and no more: its N fp32 outputs, the split copy from the input's
    # channels to the 16-channel boundary past C + N, the head's sums
    o = out.view(torch.float32)
    assert torch.isfinite(o[:, :N]).all() and torch.isnan(o[:, N:]).all()
    assert torch.isfinite(acc.view(torch.float32)).all()
    top = T.round_up_16(C + N)
    hi, lo = T.xs_channels(xs, P, nslab, 0, nslab * 16)
    assert not (hi[:, :top] == F16_NAN).any() and not (lo[:, :top] == F16_NAN).any()
    assert (hi[:, top:] == F16_NAN).all() and (lo[:, top:] == F16_NAN).all()
    assert not hi[:, C + N:top].any() and not lo[:, C + N:top].any(), "zero quads past C + N"
    h_ref, l_ref = T.split_np(o[:, :N].numpy())
    assert np.array_equal(hi[:, C:C + N], h_ref) and np.array_equal(lo[:, C:C + N], l_ref)


def test_generic_plan_gutter_case():
    """27 x 23 images (gutter packing: the generic plan whatever the switch says): the same bytes
    under both settings, and within the flow contract's 1e-5 of fp64."""
    B, H, W, C, N = 3, 27, 23, 40, 32
    a = layer_with_head(B, H, W, C, N, 6, generic=False)
    b = layer_with_head(B, H, W, C, N, 6, generic=True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    cs = a[4]
    e = T.scaled_err(T.got_nchw(a[0].view(torch.float32), cs), T.reference(cs, "ReLU"))
    print(f"gutter case {e:.2e}")
    assert e <= 1e-5, e


# ---------------------------------------------------------------- fused block against layers
@functools.lru_cache(maxsize=None)
def block_sd(depth, a, g, nh):
    import nnblock
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(depth * 100 + a + g + nh)
        mod = nnblock.DenseBlock(a, nh, {"name": "DenseLayer", "act": "ReLU"},
                                 growth_channel=depth * g, depth=depth)
        head = mod.layers[-1]
        width = a + depth * g
        head.weight.data = torch.randn(nh, width, 1, 1) / width ** 0.5
        head.bias.data = torch.randn(nh) * 0.1
    return {k: v.detach().cpu() for k, v in mod.state_dict().items()}


@functools.lru_cache(maxsize=None)
def build_block(depth, a, g, nh, bf):
    from idfcodec.engine import DeviceBlock
    from idfcodec.packing import pack_dense_block
    sd = block_sd(depth, a, g, nh)
    if bf:
        pk = pack_dense_block(sd, "", depth, "ReLU", fold=True, bf16=True)
    else:
        pk = pack_dense_block(sd, "", depth, "ReLU", fold=True, wino=True, wx3=True, dx3=True)
    return DeviceBlock(pk, torch.device("cuda"))


def run_block(db, x, fuse_layers):
    """idf_dense_block_f32 (STORE head) over NCHW x with every byte of the scratch buffer -- the
    split copy, the head's sums -- poisoned first.  Returns (head outputs, fp32 features)."""
    from idfcodec import _lib
    from idfcodec._lib import IdfHeadOut, check, lib, ptr
    from idfcodec.modules import _feat_from_nchw, dense_tmp
    from idfcodec.packing import round_up
    B, C, H, W = x.shape
    P = B * H * W
    dev = torch.device("cuda")
    feat, ld, s = _feat_from_nchw(x.to(dev), db)
    ld_tmp = ld
    if db.desc.bf16:
        ld_tmp = max(ld, round_up(ld, 64) // 2 + 2 * 48 + 8)
    tmp, ld_tmp = dense_tmp(db, B, H, W, ld_tmp, dev)
    tmp.view(torch.int16).fill_(F16_NAN)
    n = db.geom.n_head
    ldo = round_up(n, 4)
    out = torch.zeros(P, ldo, device=dev)
    h = IdfHeadOut()
    h.mode, h.out, h.ld_out = _lib.EPI_STORE, ptr(out), ldo
    d = db.desc
    saved = (d.fuse_layers, d.keep_feat)
    d.fuse_layers, d.keep_feat = int(fuse_layers), 1
    try:
        check(lib().idf_dense_block_f32(s, ctypes.byref(d), B, H, W, ptr(feat), ld, ptr(tmp), ld_tmp,
                                        ctypes.byref(h)), "dense block")
        torch.cuda.synchronize()
    finally:
        d.fuse_layers, d.keep_feat = saved
    return out[:, :n].cpu(), feat.view(P, ld).cpu()


def block_input(B, a, H, W):
    g = torch.Generator().manual_seed(H * 31 + W + a + B)
    return torch.round((torch.rand((B, a, H, W), generator=g) * 2 - 1) * 256) / 256


# a = g = 12: layers of 12, 24, 36, ... input channels -- 1, 2, 3, 3, 4, 5, 6, 6, ... slabs, so an
# odd slab count is followed by an even one and an even by an odd
BLOCK_CASES = [(geo, depth, nh, bf) for geo in ((3, 16, 16), (70, 4, 4)) for depth in (1, 2, 3, 12)
               for nh in (12, 24) for bf in (False, True) if not (bf and geo[1] == 4)]


@pytest.mark.parametrize("geo,depth,nh,bf", BLOCK_CASES)
def test_fused_block_equals_layer_launches(geo, depth, nh, bf):
    from idfcodec import _lib
    B, H, W = geo
    db = build_block(depth, 12, 12, nh, bf)
    assert (db.desc.dxb if bf else db.desc.dx3) == 1
    assert _lib.lib().idf_dx3_block_supported(H, W, db.geom.g_pad, int(bf)) == 1
    x = block_input(B, 12, H, W)
    out1, feat1 = run_block(db, x, 1)
    out0, feat0 = run_block(db, x, 0)
    assert torch.isfinite(out1).all() and out1.abs().sum() > 0
    assert torch.equal(out1, out0), int((out1 != out0).any(1).sum())
    assert torch.equal(feat1, feat0), int((feat1 != feat0).any(1).sum())


def test_fused_block_beside_another_stream():
    """The 12-layer fused block on one stream while another runs 32 x 32 layers (two-tile
    blocks, the fast halo plan): both give the bits they give alone."""
    from idfcodec import _lib
    from idfcodec._lib import check, lib, ptr
    from idfcodec.packing import dx3_groups, dx3_weights
    dev = torch.device("cuda")
    db = build_block(12, 12, 12, 12, False)
    x = block_input(40, 12, 16, 16)
    ref_blk = run_block(db, x, 1)
    B, H, W, C, N = 128, 32, 32, 60, 44
    cs = T.make_case(B, H, W, C, N, fold=True, seed=9)
    P, ld, n_alloc = B * H * W, cs["ld"], cs["n_alloc"]
    nf, ngroup = dx3_groups(n_alloc)
    Wd, ysc = dx3_weights(cs["Wt"].numpy(), C)
    Wdd = torch.from_numpy(Wd.view(np.int16)).to(dev)
    Xd, b3d, vtd, bfd = (cs[k].to(dev) for k in ("X", "b3", "vt", "bfull"))
    nslab = (C + N + 15) // 16
    xs = torch.full((nslab * 2 * P * 16,), F16_NAN, dtype=torch.int16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros(P, ld, device=dev)
    check(lib().idf_dx3_split_cols(_lib.stream_ptr(), P, 0, C, ptr(Xd), ld, ptr(xs), nslab, ptr(flag),
                                   None, 0), "split")

    def layers(k):
        for _ in range(k):
            check(lib().idf_conv3x3_dx3(_lib.stream_ptr(), B, H, W, C, ptr(xs), nslab, ptr(Wdd),
                                        nf * ngroup, ysc, ptr(b3d), ptr(vtd), n_alloc, ptr(bfd), N,
                                        ptr(out), ld, _lib.ACT["ReLU"], 0.01, ptr(flag), None, 0, None),
                  "dx3")

    layers(1)
    torch.cuda.synchronize()
    ref_out = out.clone()
    side = torch.cuda.Stream()
    out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        layers(6)
    got_blk = run_block(db, x, 1)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out)
    assert torch.equal(got_blk[0], ref_blk[0]) and torch.equal(got_blk[1], ref_blk[1])


# ---------------------------------------------------------------- the plan against the run
# (family, B, H = W, the literal counts: CONV1X1, CONV3X3 and HEAD marks): depth 3, growth 44, a
# 12-output head -- split-K per-layer launches, the fused block (16 x 16, packed 4 x 4), the
# reference's 1x1 + 3x3 pairs, and a bf16 block on the direct conv and on conv3_bf16.hip
PLAN_RUNS = [("dx3", 2, 8, (0, 3, 0)), ("dx3", 2, 16, (0, 1, 0)), ("dx3", 4, 4, (0, 1, 0)),
             ("unfold", 2, 8, (3, 3, 1)), ("dxb", 2, 16, (0, 1, 0)), ("bf16", 2, 16, (0, 3, 1))]


@pytest.mark.parametrize("family,B,H,want", PLAN_RUNS)
def test_timer_counts_equal_the_plan(family, B, H, want):
    """One timed run of the smallest block of each family: the event pairs the run records per
    tag are the plan's conv and head launches (idf_dense_block_plan answers from the plan the run
    follows)."""
    from idfcodec import _lib
    from idfcodec._lib import IdfHeadOut, block_plan, lib, ptr
    from idfcodec.engine import DeviceBlock
    from idfcodec.modules import _feat_from_nchw, dense_tmp
    from idfcodec.packing import pack_dense_block, round_up
    depth, a, g, nh = 3, 12, 44, 12
    dev = torch.device("cuda")
    if family == "unfold":
        db = DeviceBlock(pack_dense_block(block_sd(depth, a, g, nh), "", depth, "ReLU"), dev)
    else:
        db = build_block(depth, a, g, nh, family in ("dxb", "bf16"))
    flags = ("wx3", "dx3", "dxb", "fuse_head", "fuse_layers")
    saved = [getattr(db.desc, k) for k in flags]  # build_block's blocks are shared
    db.set_mode(family, fuse_layers=True)
    timer = lib().idf_timer_create(16)
    assert timer
    try:
        plan = block_plan(db.desc, B, H, H)
        feat, ld, s = _feat_from_nchw(block_input(B, a, H, H).to(dev), db)
        ld_tmp = max(ld, round_up(ld, 64) // 2 + 2 * 48 + 8) if db.desc.bf16 else ld
        tmp, ld_tmp = dense_tmp(db, B, H, H, ld_tmp, dev)
        out = torch.zeros(B * H * H, round_up(nh, 4), device=dev)
        h = IdfHeadOut()
        h.mode, h.out, h.ld_out = _lib.EPI_STORE, ptr(out), round_up(nh, 4)
        db.timer = timer
        db.run(s, B, H, H, ptr(feat), ld, ptr(tmp), ld_tmp, h)
        torch.cuda.synchronize()
        got = []
        for tag in (_lib.TAG_CONV1X1, _lib.TAG_CONV3X3, _lib.TAG_HEAD):
            ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            assert lib().idf_timer_summary(timer, tag, ctypes.byref(ms), ctypes.byref(n),
                                           ctypes.byref(fl)) == 0
            got.append(n.value)
    finally:
        db.timer = None
        lib().idf_timer_destroy(timer)
        for k, v in zip(flags, saved):
            setattr(db.desc, k, v)
    print(family, B, H, plan, got)
    assert got[0] + got[1] == plan["conv_launches"] and got[2] == plan["head_launches"], (plan, got)
    assert got[0] == plan["kind"].count("UNFOLD")
    assert tuple(got) == want and torch.isfinite(out).all() and out.abs().sum() > 0
    kind = {"dx3": "DX3", "dxb": "DXB", "bf16": "BF16", "unfold": "UNFOLD"}[family]
    assert plan["kind"] == (kind,) * depth
    assert plan["fused"] == (want[1] == 1)
