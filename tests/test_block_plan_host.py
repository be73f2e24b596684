"""The DenseBlock plan (idf_dense_block_plan: the plan idf_dense_block_f32 itself follows) on the
host: kinds by precedence, the fused block, the head and where its sums start, the error codes,
the tmp bytes and batch invariance.  Descriptors carry fake non-null pointers: nothing launches."""
import ctypes

import pytest

from idfcodec import _lib
from idfcodec._lib import block_plan

DEPTH, G_PAD = 3, 44
K_IN = (12, 56, 100, 144)
# (H, W, g_pad): the four power-of-two levels at both growths, an odd geometry, and one the dx3
# query refuses (more than 1024 outputs)
GEOMS = [(h, h, g) for h in (32, 16, 8, 4) for g in (44, 48)] + [(27, 23, 44), (8, 8, 1028)]
BATCHES = (1, 3, 256, 1024)
ARRAYS = ("wino_u", "wx3_u", "dx3_w", "wb16", "dxb_w")


def desc(g_pad=G_PAD, k0=12, n_head=12, **kw):
    """A depth-3 descriptor; flags by keyword, a weight array by the layers that have it."""
    d = _lib.IdfDenseBlock()
    d.depth, d.g_pad, d.n_head = DEPTH, g_pad, n_head
    for i in range(DEPTH + 1):
        d.k_in[i] = k0 + i * G_PAD
    for k, v in kw.items():
        if k in ARRAYS:
            for i in v:
                getattr(d, k)[i] = 0x100000 * (i + 1)  # never dereferenced: nothing launches
        else:
            setattr(d, k, v)
    return d


def sup(H, W, g):
    L = _lib.lib()
    return {"wino": bool(L.idf_conv3x3_wino_supported(H, W)),
            "dx3": bool(L.idf_conv3x3_dx3_supported(H, W, g)),
            "dxb": bool(L.idf_conv3x3_dxb_supported(H, W, g)),
            "blk": bool(L.idf_dx3_block_supported(H, W, g, 0)),
            "blk_bf": bool(L.idf_dx3_block_supported(H, W, g, 1))}


ALL = tuple(range(DEPTH))
F32 = dict(fold=1, halo=1, wino=1, wino_u=ALL, wx3=1, wx3_u=ALL, dx3=1, fuse_head=1, fuse_layers=1)
BF = dict(fold=1, bf16=1, wb16=ALL, dxb=1, dxb_w=ALL, fuse_head=1, fuse_layers=1)


def kind_rows(H, W, g):
    """(name, descriptor, expected kinds, expected wx3_first) by precedence, support taken from
    the stand-alone *_supported queries."""
    s = sup(H, W, g)
    none = (False,) * DEPTH
    halo = ("HALO",) * DEPTH
    wino = ("WINO",) * DEPTH if s["wino"] else halo
    wx3 = (("WX3",) * DEPTH, (True, False, False)) if s["wino"] else (halo, none)
    pre = ((("DX3", "DX3", wx3[0][2]), (False, False, s["wino"])) if s["dx3"] else wx3)
    return [
        ("unfold", desc(g, fold=0), ("UNFOLD",) * DEPTH, none),
        ("fold", desc(g, fold=1), ("FOLD_GEMM",) * DEPTH, none),
        ("halo", desc(g, fold=1, halo=1), halo, none),
        ("wino", desc(g, fold=1, halo=1, wino=1, wino_u=ALL), wino, none),
        ("wx3", desc(g, fold=1, halo=1, wino=1, wino_u=ALL, wx3=1, wx3_u=ALL), *wx3),
        ("dx3 prefix", desc(g, **{**F32, "dx3_w": (0, 1)}), *pre),
        ("dx3", desc(g, **F32, dx3_w=ALL), ("DX3",) * DEPTH if s["dx3"] else wx3[0],
         none if s["dx3"] else wx3[1]),
        ("bf16", desc(g, fold=1, bf16=1, wb16=ALL), ("BF16",) * DEPTH, none),
        ("dxb", desc(g, **BF), ("DXB" if s["dxb"] else "BF16",) * DEPTH, none),
    ]


@pytest.mark.parametrize("H,W,g", GEOMS)
def test_kinds_by_precedence_and_launch_counts(H, W, g):
    s = sup(H, W, g)
    assert s["dx3"] == (g <= 1024)  # (8, 8, 1028) is the refused geometry
    for name, d, kinds, first in kind_rows(H, W, g):
        p = block_plan(d, 2, H, W)
        assert p["kind"] == kinds and p["wx3_first"] == first, (name, p)
        direct = set(kinds) in ({"DX3"}, {"DXB"})
        fused = direct and s["blk_bf" if kinds[0] == "DXB" else "blk"]
        assert p["fused"] == fused, (name, p)
        assert p["n_dx3"] == sum(k in ("DX3", "DXB") for k in kinds), (name, p)
        assert p["conv_launches"] == (1 if fused else 2 * DEPTH if name == "unfold" else DEPTH)
        assert p["head"] == ("FUSED" if direct else "GEMM"), (name, p)
        assert p["head_launches"] == (0 if direct else 1), (name, p)
        own = p["head_init"] == "OWN_LAUNCH"
        copy = kinds[0] in ("DX3", "DXB", "BF16")
        assert p["setup_launches"] == int(copy) + int(own), (name, p)
    p = block_plan(desc(g, fold=0), 2, H, W)
    assert (p["head"], p["conv_launches"], p["setup_launches"]) == ("GEMM", 2 * DEPTH, 0)


def test_imagenet64_levels_all_dx3_fused_middle_only():
    """The three imagenet64 levels with every flag on: all DX3, the 16 x 16 level as one launch
    (tests/test_host_logic.py test_fused_block_geometries)."""
    for g in (44, 48):
        plans = [block_plan(desc(g, **F32, dx3_w=ALL), 1, h, h) for h in (32, 16, 8)]
        assert all(p["kind"] == ("DX3",) * DEPTH for p in plans)
        assert tuple(int(p["fused"]) for p in plans) == (0, 1, 0)


def head_rows():
    """(descriptor, H, with_head, expected head, expected head_init): full dx3 and dxb blocks at
    8 x 8 (per-layer launches) and 16 x 16 (the fused block)."""
    rows = []
    for H, init, init_bf in ((8, "IN_SPLIT", "OWN_LAUNCH"), (16, "IN_BLOCK", "IN_BLOCK")):
        for base, ini in ((dict(F32, dx3_w=ALL), init), (BF, init_bf)):
            rows += [
                (desc(**base), H, True, "FUSED", ini),
                (desc(n_head=16, **base), H, True, "FUSED", ini),
                (desc(n_head=17, **base), H, True, "GEMM", "NONE"),
                (desc(k0=64, **base), H, True, "FUSED", ini),
                (desc(k0=65, **base), H, True, "GEMM", "NONE"),
                (desc(**{**base, "fuse_head": 0}), H, True, "GEMM", "NONE"),
                (desc(**base), H, False, "NONE", "NONE"),
            ]
    return rows


def test_head_and_where_its_sums_start():
    s8, s16 = sup(8, 8, G_PAD), sup(16, 16, G_PAD)
    assert s8["dx3"] and s8["dxb"] and not s8["blk"] and not s8["blk_bf"]
    assert s16["dx3"] and s16["dxb"] and s16["blk"] and s16["blk_bf"]
    for d, H, with_head, head, init in head_rows():
        p = block_plan(d, 2, H, H, with_head)
        assert (p["head"], p["head_init"]) == (head, init), (H, with_head, d.n_head, d.k_in[0], p)
        assert p["head_launches"] == (1 if head == "GEMM" else 0)
        assert p["fused"] == (H == 16)  # the head does not decide the fused block
    # an own head-init launch is reachable only for dxb blocks on per-layer launches
    seen = False
    for H, W, g in GEOMS:
        for with_head in (True, False):
            for name, d, _, _ in kind_rows(H, W, g):
                p = block_plan(d, 2, H, W, with_head)
                if p["head_init"] == "OWN_LAUNCH":
                    seen = True
                    assert set(p["kind"]) == {"DXB"} and not p["fused"] and with_head, (name, p)
    assert seen


def test_plan_errors_keep_their_codes():
    L = _lib.lib()
    out = (ctypes.c_int32 * (len(_lib.BLOCK_PLAN_FIELDS) + _lib.MAX_DEPTH))()
    q = lambda d, B=2, H=8, W=8: L.idf_dense_block_plan(ctypes.byref(d), B, H, W, 1, out)  # noqa: E731
    ARG = 1
    assert q(desc(**F32, dx3_w=(0, 2))) == ARG        # dx3 weights that are not a prefix
    assert q(desc(**F32, dx3_w=(1, 2))) == ARG        # ... nor weights after a gap at layer 0
    assert q(desc(**{**BF, "fold": 0})) == ARG         # a bf16 block without fold
    assert q(desc(**{**BF, "wb16": (0, 2)})) == ARG    # ... with a missing wb16[i]
    assert q(desc(**{**BF, "dxb_w": (0, 2)})) == ARG   # ... on dxb with a missing dxb_w[i]
    assert q(desc(**{**BF, "dxb_w": (0, 2)}), H=4, W=4) == 0  # no dxb at 4 x 4: dxb_w unread
    # IDF_ERR_UNSUPPORTED (no direct-conv workspace size) cannot be reached through a geometry
    # the *_supported queries take: both answer from the same dx3_plan
    for H, W, g in GEOMS:
        if sup(H, W, g)["dx3"]:
            assert L.idf_conv3x3_dx3_workspace(2, H, W, K_IN[2], g) >= 0
    d = desc(**F32, dx3_w=ALL)
    assert L.idf_dense_block_plan(ctypes.byref(d), 2, 8, 8, 1, None) == ARG
    assert L.idf_dense_block_plan(None, 2, 8, 8, 1, out) == ARG
    assert q(d, B=-1) == ARG and q(d, H=0) == ARG and q(d, W=0) == ARG and q(d, B=0) == 0
    d.depth = _lib.MAX_DEPTH + 1
    assert q(d) == ARG
    # the tmp size reads the same plan: -1 for what the plan refuses
    assert L.idf_dense_block_dx3_tmp_bytes(ctypes.byref(desc(**F32, dx3_w=(0, 2))), 2, 8, 8) == -1


def test_tmp_bytes_are_the_plan_layout():
    """idf_dense_block_dx3_tmp_bytes: the split copy up to the last dx3 layer's input, the split-K
    workspace 256-B aligned after it, the fused head's sums [P][16] f32 256-B aligned after that
    (the block of test_fused_head_tmp_is_required_not_optional, and the fused-launch level)."""
    L = _lib.lib()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for B, H in ((4, 8), (3, 16), (1, 32)):
        P = B * H * H
        for n_dx3 in (2, 3):
            for fuse_head in (0, 1):
                d = desc(**{**F32, "fuse_head": fuse_head}, dx3_w=range(n_dx3))
                cin = K_IN[n_dx3 - 1]
                body = up(L.idf_dx3_split_bytes(P, (cin + 15) // 16 * 16)) + \
                    L.idf_conv3x3_dx3_workspace(B, H, H, cin, G_PAD)
                want = up(body) + P * 64 if (fuse_head and n_dx3 == DEPTH) else body
                assert L.idf_dense_block_dx3_tmp_bytes(ctypes.byref(d), B, H, H) == want
    assert L.idf_dense_block_dx3_tmp_bytes(ctypes.byref(desc(fold=1, halo=1)), 4, 8, 8) == 0
    assert L.idf_dense_block_dx3_tmp_bytes(
        ctypes.byref(desc(fold=1, bf16=1, wb16=ALL)), 4, 8, 8) == 0  # the shadow is not counted


def test_plan_does_not_depend_on_the_batch():
    """kind, fused, head and head_init at B = 1, 3, 256, 1024: a decoder may use another batch
    size than the encoder."""
    rows = [(d, H, W, True) for H, W, g in GEOMS for _, d, _, _ in kind_rows(H, W, g)]
    rows += [(d, H, H, wh) for d, H, wh, _, _ in head_rows()]
    for d, H, W, with_head in rows:
        plans = [block_plan(d, B, H, W, with_head) for B in BATCHES]
        for p in plans[1:]:
            for k in ("kind", "wx3_first", "fused", "head", "head_init", "n_dx3"):
                assert p[k] == plans[0][k], (k, H, W, p, plans[0])
