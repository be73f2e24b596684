"""The dx3 / dxb parity tests' shared case table: every row names the kernel instantiation it is
meant to select (conv3_dx3.hip: dx3_plan / dx3_launch_shape decide, dx3_run and
idf_dx3_block_launch switch over them).  tests/test_host_logic.py asks idf_dx3_launch_info -- the
same plan code, no device -- that every row selects what it claims and that the rows together
cover every instantiation the switches can reach; the GPU tests (test_gpu_dx3.py, test_gpu_bf16.py)
parametrise over the rows.  If the plan changes and a row selects something else, change the
row's shape, not its expectation.

Also the runner and the fp64 references of the fused-DenseBlock rows (BLOCK_F32 / BLOCK_BF), which
both GPU test modules use."""
from collections import namedtuple

# ---------------------------------------------------------------- per-layer rows
# sel: the fields of idf_dx3_launch_info the row claims (pitch, T, nf always; flags where the row
# is there for them)
Layer = namedtuple("Layer", "B H W C N act fold sel")


def layer(B, H, W, C, N, act="ReLU", fold=True, *, pitch, nf, T=1, **flags):
    return Layer(B, H, W, C, N, act, fold, dict(pitch=pitch, T=T, nf=nf, **flags))


# idf_conv3x3_dx3 (test_dx3_vs_fp64): (B, H, W, C, N, act, fold)
LAYER_F32 = [
    layer(3, 32, 32, 52, 44, pitch=18, nf=3), layer(5, 16, 16, 100, 44, pitch=18, nf=3),
    layer(3, 32, 32, 496, 44, pitch=18, nf=3), layer(1, 16, 16, 520, 44, pitch=18, nf=3),
    layer(2, 64, 64, 8, 16, "LeakyReLU", pitch=18, nf=1),
    layer(2, 20, 32, 24, 32, pitch=18, nf=2),
    layer(2, 16, 48, 12, 43, "LeakyReLU", pitch=18, nf=3), layer(1, 5, 16, 40, 44, pitch=18, nf=3),
    layer(4, 16, 16, 36, 12, "ReLU", False, pitch=18, nf=1),
    layer(2, 32, 32, 100, 48, "LeakyReLU", pitch=18, nf=3),
    layer(3, 17, 16, 20, 44, "None", pitch=18, nf=3),
    # packed tiles: 8x8 images 2x2 to a tile with K split in 4 chunks (imagenet64's 8x8
    # level: a partial last band, 1 slab a chunk, 9 slabs a chunk), one group of 1 fragment
    layer(5, 8, 8, 36, 44, pitch=10, nf=3, nchunk=3), layer(6, 8, 8, 520, 44, pitch=10, nf=3, nchunk=4),
    layer(4, 8, 8, 52, 44, pitch=10, nf=3, nchunk=4),
    layer(2, 8, 8, 12, 16, "LeakyReLU", pitch=10, nf=1, nchunk=1),
    # 4x4 images 4x4 to a tile (config 4's first level): 64 outputs (4 fragments), 128 (two
    # groups of 4), a partial band
    layer(3, 4, 4, 100, 64, pitch=6, nf=4), layer(2, 4, 4, 36, 128, pitch=6, nf=4, ngroup=2),
    layer(17, 4, 4, 20, 64, pitch=6, nf=4),
    # gutter packing (images at pitch W + 1 / H + 1, the zero column / row between two images
    # shared): 27x23 (config 5's patches, 2 x 4 a band), 24- and 40-wide, 2x2 (config 4's
    # second level: 16 x 16 a band, 128 outputs), 7x7 (split K), 12x12, 8-wide with 4 rows (its
    # segment canvas would not fit); 8-wide segments with rows that do not pack
    layer(3, 27, 23, 40, 32, "LeakyReLU", pitch=18, nf=2, gut=1),
    layer(2, 8, 24, 20, 44, pitch=18, nf=3, gut=1), layer(1, 8, 40, 20, 44, pitch=18, nf=3, gut=1),
    layer(37, 2, 2, 24, 128, pitch=25, nf=4, ngroup=2, xskip=1),
    layer(5, 7, 7, 20, 44, pitch=18, nf=3, gut=1, nchunk=2),
    layer(3, 12, 12, 36, 44, "LeakyReLU", pitch=18, nf=3, gut=1),
    layer(6, 4, 8, 40, 44, pitch=18, nf=3, gut=1),
    layer(2, 5, 8, 24, 44, pitch=10, nf=3, nchunk=2), layer(2, 16, 8, 24, 44, pitch=10, nf=3, nchunk=1),
    # 2-wide images with every lane on an image column (xskip): config 4's 2x2 level at 64
    # outputs, a batch over one 16 x 16 band (partial second band), odd heights, one row
    layer(5, 2, 2, 100, 64, pitch=25, nf=4, xskip=1),
    layer(300, 2, 2, 36, 44, "LeakyReLU", pitch=25, nf=3, xskip=1),
    layer(3, 5, 2, 20, 44, pitch=25, nf=3, xskip=1), layer(4, 1, 2, 12, 16, pitch=25, nf=1, xskip=1),
    layer(9, 2, 2, 20, 12, "None", False, pitch=25, nf=1, xskip=1),
    # two tiles per block (from 512 tiles on the 16-wide canvas): 1, 2 and 3 fragments, an odd
    # tile count (the last block holds one tile), the gutter canvas (config 5's 2048-patch
    # batches: 25 bands of 21 tiles, the last band holding one image)
    layer(128, 32, 32, 8, 16, pitch=18, T=2, nf=1, ntiles=512),
    layer(128, 32, 32, 12, 32, "LeakyReLU", pitch=18, T=2, nf=2, ntiles=512),
    layer(171, 48, 16, 20, 44, pitch=18, T=2, nf=3, ntiles=513),
    layer(193, 27, 23, 8, 32, "LeakyReLU", pitch=18, T=2, nf=2, gut=1, ntiles=525),
    # one tile per block, the instantiations no row above selects: 4 fragments on the 16-wide
    # canvas (tiles, gutter), the 8-wide segments at 2 and 4 fragments (3 chunks) and 12 rows
    # (no split), 2-wide images at 2 fragments, the 4-wide segments at 1 - 3 fragments, 8x4
    # images, 4-wide segments with rows that do not pack (split K)
    layer(2, 16, 16, 20, 64, pitch=18, nf=4), layer(3, 5, 5, 20, 64, pitch=18, nf=4, gut=1),
    layer(3, 8, 8, 20, 32, pitch=10, nf=2, nchunk=2), layer(3, 8, 8, 36, 64, pitch=10, nf=4, nchunk=3),
    layer(3, 12, 8, 20, 16, "LeakyReLU", pitch=10, nf=1, nchunk=1),
    layer(9, 2, 2, 20, 32, pitch=25, nf=2, xskip=1),
    layer(5, 4, 4, 20, 16, pitch=6, nf=1), layer(5, 4, 4, 36, 32, "LeakyReLU", pitch=6, nf=2),
    layer(17, 4, 4, 20, 44, pitch=6, nf=3), layer(5, 8, 4, 20, 44, pitch=6, nf=3, nchunk=1),
    layer(3, 3, 4, 36, 44, pitch=6, nf=3, nchunk=3),
]

# idf_conv3x3_dxb (test_conv3x3_dxb_vs_fp64): (B, H, W, C, N), ReLU, folded
LAYER_BF = [
    layer(3, 32, 32, 52, 43, pitch=18, nf=3), layer(130, 32, 32, 100, 44, pitch=18, T=2, nf=3),
    layer(5, 16, 16, 100, 43, pitch=18, nf=3), layer(9, 8, 8, 168, 43, pitch=10, nf=3, nchunk=4),
    layer(4, 27, 23, 40, 32, pitch=18, nf=2, gut=1), layer(1, 16, 16, 520, 43, pitch=18, nf=3),
    layer(2, 32, 32, 12, 16, pitch=18, nf=1), layer(3, 8, 8, 20, 20, pitch=10, nf=2, nchunk=2),
    # two tiles per block at 1 and 2 fragments; the 8 x 8 segments at 1 fragment
    layer(128, 32, 32, 12, 16, pitch=18, T=2, nf=1, ntiles=512),
    layer(128, 32, 32, 20, 32, pitch=18, T=2, nf=2, ntiles=512),
    layer(3, 8, 8, 20, 16, pitch=10, nf=1, nchunk=2),
]


def layer_params(rows, fields="B H W C N act fold"):
    return [tuple(getattr(r, f) for f in fields.split()) for r in rows]


def two_tile_rows(rows):
    return [r for r in rows if r.sel["T"] == 2]


# test_dx3_fused_head: (B, H, W, nh, N) -- two layers of C = 20 and 20 + N inputs; T = 2 rows on
# tiles (even and odd tile counts) and on the gutter canvas
Head = namedtuple("Head", "B H W nh N sel")
HEAD_C0 = 20
HEAD_F32 = [
    Head(2, 32, 32, 3, 44, dict(pitch=18, T=1, nf=3)), Head(3, 16, 16, 12, 44, dict(pitch=18, T=1, nf=3)),
    Head(5, 8, 8, 16, 44, dict(pitch=10, T=1, nf=3)), Head(3, 27, 23, 6, 44, dict(pitch=18, T=1, nf=3, gut=1)),
    Head(40, 2, 2, 12, 44, dict(pitch=25, T=1, nf=3)), Head(37, 4, 4, 6, 64, dict(pitch=6, T=1, nf=4)),
    Head(150, 2, 2, 12, 64, dict(pitch=25, T=1, nf=4)), Head(9, 27, 23, 6, 64, dict(pitch=18, T=1, nf=4, gut=1)),
    Head(128, 32, 32, 3, 44, dict(pitch=18, T=2, nf=3, ntiles=512)),
    Head(171, 48, 16, 12, 32, dict(pitch=18, T=2, nf=2, ntiles=513)),
    Head(193, 27, 23, 6, 44, dict(pitch=18, T=2, nf=3, gut=1, ntiles=525)),
]

# ---------------------------------------------------------------- fused-DenseBlock rows
# conv3_dx3_block_kernel through idf_dense_block_f32 (fuse_layers): depth-3 DenseBlocks of `a`
# input channels growing by g a layer, an n_head-output head.  head: "fused" (n_head <= 16 and an
# input of <= 64 channels: the sums ride in the block kernel's registers) or "gemm".  B leaves the
# last tile partly filled and gives more than one tile.  sel: (pitch, nf).
Block = namedtuple("Block", "B H W a g nh act head sel")
BLOCK_DEPTH = 3
BLOCK_F32 = [
    # 16-wide images of up to 16 rows, one a tile
    Block(3, 16, 16, 3, 12, 3, "ReLU", "fused", (18, 1)),
    Block(3, 9, 16, 10, 28, 12, "LeakyReLU", "fused", (18, 2)),
    Block(3, 5, 16, 64, 44, 16, "ReLU", "fused", (18, 3)),
    Block(3, 16, 16, 10, 60, 12, "ReLU", "fused", (18, 4)),
    Block(3, 16, 16, 12, 44, 24, "ReLU", "gemm", (18, 3)),
    Block(3, 9, 16, 66, 16, 12, "LeakyReLU", "gemm", (18, 1)),
    # 8-wide images of 9 - 16 rows, two a tile
    Block(5, 12, 8, 10, 16, 12, "ReLU", "fused", (10, 1)),
    Block(5, 16, 8, 3, 32, 3, "LeakyReLU", "fused", (10, 2)),
    Block(5, 9, 8, 64, 44, 16, "ReLU", "fused", (10, 3)),
    Block(5, 12, 8, 12, 64, 12, "ReLU", "fused", (10, 4)),
    Block(5, 16, 8, 12, 44, 24, "ReLU", "gemm", (10, 3)),
    # 4-wide images: 4x4 (16 a tile), 8x4 (8 a tile)
    Block(21, 4, 4, 10, 12, 12, "ReLU", "fused", (6, 1)),
    Block(11, 8, 4, 3, 24, 3, "LeakyReLU", "fused", (6, 2)),
    Block(21, 4, 4, 64, 44, 16, "ReLU", "fused", (6, 3)),
    Block(11, 8, 4, 12, 64, 12, "ReLU", "fused", (6, 4)),
    Block(21, 4, 4, 66, 28, 6, "ReLU", "gemm", (6, 2)),
]
BLOCK_BF = [
    Block(3, 16, 16, 10, 16, 12, "ReLU", "fused", (18, 1)),
    Block(3, 9, 16, 3, 32, 3, "LeakyReLU", "fused", (18, 2)),
    Block(3, 5, 16, 64, 44, 16, "ReLU", "fused", (18, 3)),
    Block(3, 16, 16, 12, 44, 24, "ReLU", "gemm", (18, 3)),
    Block(5, 12, 8, 10, 12, 12, "ReLU", "fused", (10, 1)),
    Block(5, 16, 8, 3, 28, 3, "LeakyReLU", "fused", (10, 2)),
    Block(5, 9, 8, 64, 44, 16, "ReLU", "fused", (10, 3)),
    Block(5, 12, 8, 66, 32, 12, "ReLU", "gemm", (10, 2)),
]


def block_id(r):
    return f"{r.B}x{r.H}x{r.W}-a{r.a}-g{r.g}-h{r.nh}-{r.head}"


def block_widths(r):
    """(padded growth N, [padded input channels of every layer]) as packing.BlockGeometry lays
    the features out."""
    a_pad, g_pad = (r.a + 3) // 4 * 4, (r.g + 3) // 4 * 4
    return g_pad, [a_pad + i * g_pad for i in range(BLOCK_DEPTH)]


# ---------------------------------------------------------------- the block rows' runner
TOL = 1e-5  # the flow contract (BASELINE): scaled error against fp64


def scaled_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()


def build_block(r, bf):
    """(DenseBlock module with random weights -- the head too, which the reference zero-
    initialises --, its state dict on the CPU, its DeviceBlock packed for dx3 / dxb)."""
    import torch
    import nnblock
    from idfcodec.engine import DeviceBlock
    from idfcodec.packing import pack_dense_block
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(r.B * 1000 + r.H * 100 + r.a + r.g + r.nh)
        mod = nnblock.DenseBlock(r.a, r.nh, {"name": "DenseLayer", "act": r.act},
                                 growth_channel=BLOCK_DEPTH * r.g, depth=BLOCK_DEPTH)
        head = mod.layers[-1]
        width = r.a + BLOCK_DEPTH * r.g
        head.weight.data = torch.randn(r.nh, width, 1, 1) / width ** 0.5
        head.bias.data = torch.randn(r.nh) * 0.1
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    if bf:
        pk = pack_dense_block(sd, "", BLOCK_DEPTH, r.act, fold=True, bf16=True)
    else:
        pk = pack_dense_block(sd, "", BLOCK_DEPTH, r.act, fold=True, wino=True, wx3=True, dx3=True)
    db = DeviceBlock(pk, torch.device("cuda"))
    assert (db.desc.dxb if bf else db.desc.dx3) == 1 and db.desc.fuse_head == 1
    return mod, sd, db


def block_input(r, B=None):
    """[B, a, H, W] on the 1/256 grid in [-1, 1] (flow activations live on it)."""
    import torch
    g = torch.Generator().manual_seed(r.H * 31 + r.W + r.a)
    x = torch.round((torch.rand((r.B, r.a, r.H, r.W), generator=g) * 2 - 1) * 256) / 256
    return x if B is None else x[:B]


def run_block(db, x, mode, fuse_layers, keep_feat, flag=None, base=None):
    """idf_dense_block_f32 over NCHW x with the head epilogue `mode`.  Returns (out [P, n_head]
    for STORE / COUPLE_*, or (mean, logscale, scale) NCHW for PRIOR; the fp32 features
    [P, ld_feat])."""
    import ctypes
    import torch
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
    n = db.geom.n_head
    ldo = round_up(n, 4)
    out = torch.zeros(P, ldo, device=dev)
    h = IdfHeadOut()
    h.mode, h.out, h.ld_out = mode, ptr(out), ldo
    if base is not None:
        based = base.to(dev)
        h.base, h.ld_base = ptr(based), ldo
    prior = None
    if mode == _lib.EPI_PRIOR:
        prior = [torch.zeros(B, n // 2, H, W, device=dev) for _ in range(3)]
        h.n_mean = n // 2
        h.mean, h.logscale, h.scale = (ptr(t) for t in prior)
    d = db.desc
    saved = (d.fuse_layers, d.keep_feat, d.range_flag)
    d.fuse_layers, d.keep_feat = int(fuse_layers), int(keep_feat)
    d.range_flag = flag.data_ptr() if flag is not None else None
    try:
        check(lib().idf_dense_block_f32(s, ctypes.byref(d), B, H, W, ptr(feat), ld, ptr(tmp),
                                        ld_tmp, ctypes.byref(h)), "dense block")
        torch.cuda.synchronize()
    finally:
        d.fuse_layers, d.keep_feat, d.range_flag = saved
    res = tuple(t.cpu() for t in prior) if prior else out[:, :n].cpu()
    return res, feat.view(P, ld).cpu()


def layer_ref_f32(feat, geom, sd, i, H, W, act, slope=0.01):
    """nnlayer.py:48-51 in fp64 on the kernel's own layer-i input (teacher-forced):
    act(conv3x3(pad0(W1 x + b1)) + b3), [P, g]."""
    import torch
    import torch.nn.functional as F
    c = geom.a + sum(geom.growth[:i])
    B = feat.shape[0] // (H * W)
    x = feat[:, torch.as_tensor(geom.positions(c))].double().view(B, H, W, c).permute(0, 3, 1, 2)
    t = F.conv2d(x, sd[f"layers.{i}.layers.0.weight"].double(), sd[f"layers.{i}.layers.0.bias"].double())
    h = F.conv2d(t, sd[f"layers.{i}.layers.1.weight"].double(), sd[f"layers.{i}.layers.1.bias"].double(),
                 padding=1)
    h = F.relu(h) if act == "ReLU" else F.leaky_relu(h, slope)
    return h.permute(0, 2, 3, 1).reshape(B * H * W, -1)


def layer_ref_bf(feat, geom, pk, i, H, W, act, slope=0.01):
    """The bf16 layer in fp64 over its bf16-rounded operands: the folded weights the kernel holds,
    the bf16 rounding of its own fp32 layer input; the 1x1 bias through the taps inside the
    image (vtap) and b3 in fp32."""
    import torch
    import torch.nn.functional as F
    k, gi = geom.k_in[i], geom.growth[i]
    B = feat.shape[0] // (H * W)
    xr = feat[:, :k].to(torch.bfloat16).double().view(B, H, W, k).permute(0, 3, 1, 2)
    w = torch.from_numpy(pk.w3[i][:gi, :, :k]).to(torch.bfloat16).double()
    w = w.permute(0, 2, 1).reshape(gi, k, 3, 3)
    mask = F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64),
                    torch.eye(9, dtype=torch.float64).view(9, 1, 3, 3), padding=1)
    ref = F.conv2d(xr, w, padding=1) + torch.from_numpy(pk.b3[i][:gi]).double().view(1, -1, 1, 1)
    ref = ref + torch.einsum("tn,bthw->bnhw", torch.from_numpy(pk.vtap[i][:, :gi]).double(), mask)
    ref = F.relu(ref) if act == "ReLU" else F.leaky_relu(ref, slope)
    return ref.permute(0, 2, 3, 1).reshape(B * H * W, gi)


def check_block_row(r, bf):
    """One fused-DenseBlock row, assertions (a) - (e) of the test docstrings."""
    import torch
    import flow_oracle as FO
    from idfcodec import _lib
    from idfcodec._lib import dx3_launch_info
    N, Cs = block_widths(r)
    for C in Cs:  # the row runs the instantiation it names, fused
        info = dx3_launch_info(r.B, r.H, r.W, C, N, bf)
        assert info["block"] == 1 and (info["pitch"], info["nf"]) == r.sel and info["ntiles"] > 1, info
    mod, sd, db = build_block(r, bf)
    geom = db.geom
    assert (geom.g_pad, geom.k_in[:BLOCK_DEPTH]) == (N, Cs)
    fused_head = r.nh <= 16 and geom.k_in[0] <= 64
    assert fused_head == (r.head == "fused")
    x = block_input(r)
    hw = r.H * r.W
    P = r.B * hw
    flag = None if bf else torch.zeros(1, dtype=torch.int32, device="cuda")
    STORE = _lib.EPI_STORE
    # (a) one launch and per-layer launches: the same head outputs and fp32 features
    out, feat = run_block(db, x, STORE, 1, 1, flag)
    out0, feat0 = run_block(db, x, STORE, 0, 1, flag)
    assert torch.isfinite(out).all() and out.abs().sum() > 0
    assert torch.equal(out, out0), int((out != out0).any(1).sum())
    assert torch.equal(feat, feat0), int((feat != feat0).any(1).sum())
    # (b) every layer against fp64 on the kernel's own layer input; the head against fp64 over
    # the kernel's features; the whole f32 block against the fp64 DenseBlock
    for i in range(BLOCK_DEPTH):
        got = feat[:, geom.k_in[i + 1] - geom.g_pad:][:, :geom.growth[i]]
        ref = (layer_ref_bf(feat, geom, db.packed, i, r.H, r.W, r.act) if bf
               else layer_ref_f32(feat, geom, sd, i, r.H, r.W, r.act))
        e = scaled_err(got, ref)
        print(f"layer {i} {e:.2e}")
        assert e <= TOL, ("layer", i, e)
        pad = feat[:, geom.k_in[i] + geom.growth[i]:geom.k_in[i + 1]]
        assert not pad.any(), ("pad columns of layer", i)
    wh = torch.from_numpy(db.packed.wh[:r.nh, :geom.width]).double()
    href = feat[:, :geom.width].double() @ wh.T + torch.from_numpy(db.packed.bh[:r.nh]).double()
    e = scaled_err(out, href)
    print(f"head {e:.2e}")
    assert e <= TOL, ("head", e)
    if not bf:
        sd64 = {k: v.double() for k, v in sd.items()}
        ref = FO.dense_block(x.double(), sd64, "", BLOCK_DEPTH, r.act)
        e = scaled_err(out, ref.permute(0, 2, 3, 1).reshape(P, r.nh))
        print(f"block {e:.2e}")
        assert e <= TOL, ("block", e)
    # (c) an image alone equals its slice of the batch
    for i in sorted({0, r.B // 2, r.B - 1}):
        o1, f1 = run_block(db, x[i:i + 1], STORE, 1, 1, flag)
        assert torch.equal(o1, out[i * hw:(i + 1) * hw]), ("alone", i)
        assert torch.equal(f1, feat[i * hw:(i + 1) * hw]), ("alone feat", i)
    # (e) a re-run gives the same bits, also without the fp32 feature stores
    again, _ = run_block(db, x, STORE, 1, 0, flag)
    assert torch.equal(again, out), "re-run (fp32 stores skipped) differs"
    # (d) the head's other epilogues
    g = torch.Generator().manual_seed(r.nh)
    ldo = (r.nh + 3) // 4 * 4
    base = torch.round(torch.randn(P, ldo, generator=g) * 256) / 256
    r8 = torch.round(out * 256) / 256
    for mode, sign in ((_lib.EPI_COUPLE_ADD, 1), (_lib.EPI_COUPLE_SUB, -1)):
        o3, _ = run_block(db, x, mode, 1, 0, flag, base=base)
        assert torch.equal(o3, base[:, :r.nh] + sign * r8), mode
    if r.nh % 2 == 0:
        (mean, logs, scale), _ = run_block(db, x, _lib.EPI_PRIOR, 1, 0, flag)
        hn = out.view(r.B, r.H, r.W, r.nh).permute(0, 3, 1, 2)
        assert torch.equal(mean, hn[:, :r.nh // 2])
        assert torch.equal(logs, hn[:, r.nh // 2:])
        assert torch.allclose(scale, torch.exp(logs), rtol=1e-6, atol=0)
    if flag is not None:
        assert int(flag.item()) == 0, "range flag set"
