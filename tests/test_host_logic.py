"""Host-side logic on CPU: C-ABI exports, weight packing, mirror modules,
bitstream container, coder chaining, expf restatement (exhaustive)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from conftest import PKG, REPO


# ------------------------------------------------------------------ C ABI
def _header_functions():
    src = open(os.path.join(REPO, "include", "idf_codec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_0-9]+\s*\*?\s*(idf_[a-z0-9_]+)\s*\(", src,
                                 flags=re.M)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from idfcodec import _lib
    names = _header_functions()
    assert len(names) >= 20
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/idf_codec.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes signatures out of sync with the header"
    lib = _lib.lib()
    assert lib.idf_version().decode().startswith("idfcodec")


def test_dx3_case_table_selects_and_covers_every_instantiation():
    """tests/dx3_cases.py against the dispatch itself (idf_dx3_launch_info: dx3_plan and
    dx3_launch_shape on the host): every row selects the kernel it names, and the rows together
    reach every instantiation the launch switches hold."""
    import dx3_cases as T
    from idfcodec._lib import dx3_launch_info

    def holds(info, sel):
        return info["ok"] == 1 and all(info[k] == v for k, v in sel.items())

    seen = {"layer_f32": set(), "layer_bf": set(), "block_f32": set(), "block_bf": set()}
    flags = set()
    for bf, rows in ((False, T.LAYER_F32), (True, T.LAYER_BF)):
        for r in rows:
            info = dx3_launch_info(r.B, r.H, r.W, r.C, r.N, bf)
            assert holds(info, r.sel), (r, info)
            seen["layer_bf" if bf else "layer_f32"].add((info["pitch"], info["T"], info["nf"]))
            if bf:
                continue
            flags |= {name for name, on in (
                ("gut T1", info["gut"] and info["T"] == 1), ("gut T2", info["gut"] and info["T"] == 2),
                ("split pitch 10", info["nchunk"] > 1 and info["pitch"] == 10),
                ("split pitch 6", info["nchunk"] > 1 and info["pitch"] == 6),
                ("split gutter", info["nchunk"] > 1 and info["gut"]),
                ("groups", info["ngroup"] > 1),
                ("odd tiles T2", info["T"] == 2 and info["ntiles"] % 2 == 1)) if on}
    for r in T.HEAD_F32:  # the fused-head rows: both layers of each
        for C in (T.HEAD_C0, T.HEAD_C0 + r.N):
            info = dx3_launch_info(r.B, r.H, r.W, C, r.N, False)
            assert holds(info, r.sel), (r, C, info)
    assert {(r.sel["gut"] if "gut" in r.sel else 0, r.sel["ntiles"] % 2)
            for r in T.HEAD_F32 if r.sel["T"] == 2} == {(0, 0), (0, 1), (1, 1)}
    for bf, rows in ((False, T.BLOCK_F32), (True, T.BLOCK_BF)):
        for r in rows:
            N, Cs = T.block_widths(r)
            per_tile = None
            for C in Cs:
                info = dx3_launch_info(r.B, r.H, r.W, C, N, bf)
                assert info["ok"] == 1 and info["block"] == 1, (r, info)
                assert (info["pitch"], info["nf"]) == r.sel and info["nchunk"] == 1, (r, info)
                one = dx3_launch_info(1, r.H, r.W, C, N, bf)["ntiles"]
                # more than one tile; where a tile holds several images, the last partly filled
                per_tile = next(b for b in range(1, 257)
                                if dx3_launch_info(b + 1, r.H, r.W, C, N, bf)["ntiles"] > one)
                assert per_tile == {18: 1, 10: 2, 6: 64 // (r.H * r.W) * 4}[r.sel[0]], (r, per_tile)
                assert info["ntiles"] > 1 and (per_tile == 1 or r.B % per_tile), (r, per_tile)
            assert (r.head == "fused") == (r.nh <= 16 and Cs[0] <= 64), r
            seen["block_bf" if bf else "block_f32"].add(r.sel)
    # The full set, literally: conv3_dx3.hip dx3_run -- IDF_DXB_NF over (W4, 18), (W2, 18),
    # (W2, 10) for bf16; the T == 2 switch (nf 1 - 3) and IDF_DX3_NF over pitches 18, 10, 25, 6
    # for f32 -- and idf_dx3_block_launch -- IDF_DX3B_NF over pitches 18, 10 (bf16, nf 1 - 3) and
    # 18, 10, 6 (f32, nf 1 - 4).  (pitch, tiles per block, nf) / (pitch, nf).
    assert seen["layer_f32"] == {
        (18, 1, 1), (18, 1, 2), (18, 1, 3), (18, 1, 4), (18, 2, 1), (18, 2, 2), (18, 2, 3),
        (10, 1, 1), (10, 1, 2), (10, 1, 3), (10, 1, 4), (25, 1, 1), (25, 1, 2), (25, 1, 3),
        (25, 1, 4), (6, 1, 1), (6, 1, 2), (6, 1, 3), (6, 1, 4)}
    assert seen["layer_bf"] == {
        (18, 1, 1), (18, 1, 2), (18, 1, 3), (18, 2, 1), (18, 2, 2), (18, 2, 3),
        (10, 1, 1), (10, 1, 2), (10, 1, 3)}
    assert seen["block_f32"] == {
        (18, 1), (18, 2), (18, 3), (18, 4), (10, 1), (10, 2), (10, 3), (10, 4),
        (6, 1), (6, 2), (6, 3), (6, 4)}
    assert seen["block_bf"] == {(18, 1), (18, 2), (18, 3), (10, 1), (10, 2), (10, 3)}
    assert flags == {"gut T1", "gut T2", "split pitch 10", "split pitch 6", "split gutter",
                     "groups", "odd tiles T2"}
    # heads of the block rows: fused with inputs of 4 / 12 / 64 channels and 3 / 12 / 16 outputs,
    # GEMM with 24 outputs and with an input wider than 64 channels
    for rows in (T.BLOCK_F32, T.BLOCK_BF):
        fused = [r for r in rows if r.head == "fused"]
        assert {T.block_widths(r)[1][0] for r in fused} == {4, 12, 64}
        assert {r.nh for r in fused} == {3, 12, 16}
        gemm = [r for r in rows if r.head == "gemm"]
        assert any(r.nh == 24 for r in gemm) and any(T.block_widths(r)[1][0] > 64 for r in gemm)
    # what the query refuses
    assert dx3_launch_info(1, 8, 8, 16, 1025)["ok"] == 0
    assert dx3_launch_info(1, 4, 4, 16, 44, True)["ok"] == 0   # no bf16 kernel at pitch 6
    assert dx3_launch_info(1, 16, 16, 16, 64, True)["ok"] == 0  # nor at 4 fragments
    assert dx3_launch_info(4, 8, 8, 36, 44)["block"] == 0       # split K: per-layer launches


def test_fused_head_tmp_is_required_not_optional():
    """A dx3 block whose head fuses (by its geometry alone) needs idf_dense_block_dx3_tmp_bytes of
    tmp: one byte less is IDF_ERR_WORKSPACE (no quiet switch to the head GEMM, whose sums run in
    another order), and the need does not depend on the room offered.  Host-side checks only:
    the call returns before any launch."""
    import ctypes
    from idfcodec import _lib
    lib = _lib.lib()
    d = _lib.IdfDenseBlock()
    d.depth, d.g_pad, d.n_head, d.fold, d.wx3, d.dx3, d.fuse_head = 2, 44, 12, 1, 1, 1, 1
    for i, c in enumerate((12, 56, 100)):
        d.k_in[i] = c
    for i in range(2):
        d.dx3_w[i] = 0x100000 * (i + 1)  # never dereferenced before the workspace check
    B, H, W = 4, 8, 8  # the split-K level: its partial sums make the need exceed P * k_in[2] * 4
    P = B * H * W
    need = int(lib.idf_dense_block_dx3_tmp_bytes(ctypes.byref(d), B, H, W))
    assert need >= P * (4 * 64 + 64)  # at least the split copy (4 slabs) and the head sums
    d.fuse_head = 0
    need_nf = int(lib.idf_dense_block_dx3_tmp_bytes(ctypes.byref(d), B, H, W))
    assert need - need_nf >= P * 64
    d.fuse_head = 1
    head = _lib.IdfHeadOut()
    head.mode = _lib.EPI_STORE
    ld_tmp = (need - 1) // (4 * P)  # floats per pixel: P * ld_tmp * 4 < need
    assert P * ld_tmp * 4 < need and ld_tmp >= 100 and (need - P * 64) < P * ld_tmp * 4
    fake = ctypes.c_void_p(0x7f0000000000)  # 256-B aligned, never touched
    rc = lib.idf_dense_block_f32(None, ctypes.byref(d), B, H, W, fake, 112, fake, ld_tmp,
                                 ctypes.byref(head))
    assert rc == 3, _lib.ERR_NAMES.get(rc, rc)  # IDF_ERR_WORKSPACE
    d.n_head = 17  # no fusion for heads of > 16 outputs: only the copy and split-K part
    assert int(lib.idf_dense_block_dx3_tmp_bytes(ctypes.byref(d), B, H, W)) == need_nf


def test_struct_layout_matches_header():
    """ctypes mirror of IdfDenseBlock / IdfHeadOut == the C layout (compiled probe)."""
    from idfcodec import _lib
    import ctypes
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "idf_codec.h"
int main(){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(IdfDenseBlock), offsetof(IdfDenseBlock,w1),
 offsetof(IdfDenseBlock,n_head), offsetof(IdfDenseBlock,bh), sizeof(IdfHeadOut), offsetof(IdfHeadOut,scale));}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        c = os.path.join(t, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(t, "p")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split()))
    D, H = _lib.IdfDenseBlock, _lib.IdfHeadOut
    assert got == [ctypes.sizeof(D), D.w1.offset, D.n_head.offset, D.bh.offset, ctypes.sizeof(H),
                   H.scale.offset]


# ------------------------------------------------------------------ packing
def _simulate_packed_block(pb, x):
    """The device algorithm (padded pixel-major GEMMs) replayed with torch on CPU."""
    from idfcodec.packing import round_up
    g = pb.geom
    B, C, H, W = x.shape
    P = B * H * W
    feat = torch.zeros(P, g.ld_feat, dtype=torch.float64)
    feat[:, :C] = x.permute(0, 2, 3, 1).reshape(P, C).double()
    act = {"ReLU": F.relu, "LeakyReLU": lambda v: F.leaky_relu(v, 0.01)}[pb.act]
    for i in range(g.depth):
        k = g.k_in[i]
        if pb.fold:
            X = feat[:, :k].view(B, H, W, k).permute(0, 3, 1, 2)
            w3 = torch.from_numpy(pb.w3[i]).double()[: g.g_pad, :, :k]
            wc = w3.permute(0, 2, 1).reshape(g.g_pad, k, 3, 3)
            o = F.conv2d(X, wc, padding=1)
            v = torch.from_numpy(pb.vtap[i]).double()[:, : g.g_pad]          # [tap, n]
            ones = torch.ones(1, 1, H, W, dtype=torch.float64)
            # number of in-image taps per pixel and tap, as a 9-channel mask
            mask = F.conv2d(ones, torch.eye(9, dtype=torch.float64).view(9, 1, 3, 3), padding=1)
            bias = torch.einsum("tn,bthw->bnhw", v, mask) + \
                torch.from_numpy(pb.b3[i]).double()[: g.g_pad].view(1, -1, 1, 1)
            feat[:, k:k + g.g_pad] = act(o + bias).permute(0, 2, 3, 1).reshape(P, g.g_pad)
            continue
        w1 = torch.from_numpy(pb.w1[i]).double()
        T = feat[:, :k] @ w1[:k, :k].T + torch.from_numpy(pb.b1[i]).double()[:k]
        Tn = T.view(B, H, W, k).permute(0, 3, 1, 2)
        w3 = torch.from_numpy(pb.w3[i]).double()[: g.g_pad, :, :k]  # [g, tap, c]
        w3c = w3.permute(0, 2, 1).reshape(g.g_pad, k, 3, 3)
        o = F.conv2d(Tn, w3c, torch.from_numpy(pb.b3[i]).double()[: g.g_pad], padding=1)
        feat[:, k:k + g.g_pad] = act(o).permute(0, 2, 3, 1).reshape(P, g.g_pad)
    kh = g.k_in[g.depth]
    out = feat[:, :kh] @ torch.from_numpy(pb.wh).double()[: g.n_head, :kh].T + \
        torch.from_numpy(pb.bh).double()[: g.n_head]
    del round_up
    return out.view(B, H, W, g.n_head).permute(0, 3, 1, 2)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("name", ["t1_idflows_2lvl", "t2_idflows_3lvl_leaky", "t4_cond_s1_odd"])
def test_packed_layout_reproduces_dense_block(golden, name, fold):
    import flow_oracle as FO
    from idfcodec.packing import pack_dense_block
    d = golden(f"flow_{name}.npz")
    cfg = yaml.safe_load(bytes(d["cfg_yaml"]).decode())
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}
    depth = cfg["couple"]["nn"]["depth"]
    act = cfg["couple"]["nn"]["layer"]["act"]
    prefix = "blocks.0.flows.1.dense."
    pb = pack_dense_block(sd, prefix, depth, act, fold=fold)
    a = pb.geom.a
    x = torch.randn(2, a, cfg["H"] // cfg["extenddim"]["scale"], cfg["W"] // cfg["extenddim"]["scale"],
                    generator=torch.Generator().manual_seed(5))
    ref = FO.dense_block(x.double(), {k: v.double() for k, v in sd.items()}, prefix, depth, act)
    got = _simulate_packed_block(pb, x)
    # unfolded: exact layout check; folded: W3.W1 is rounded once to fp32 (~1e-7 rel)
    tol = 1e-6 if fold else 1e-9
    torch.testing.assert_close(got, ref, rtol=tol, atol=tol)
    # padding columns are exactly zero in every weight
    g = pb.geom
    pad_cols = sorted(set(range(g.width)) - set(g.positions(g.a + sum(g.growth)).tolist()))
    assert np.all(pb.wh[:, pad_cols] == 0)


def test_tile_n_matches_kernel_source():
    from idfcodec.packing import tile_n
    src = open(os.path.join(PKG, "csrc", "flow_kernels.hip")).read()
    assert "static int tile_n(int N)" in src
    assert [tile_n(n) for n in (3, 16, 17, 44, 48, 64, 65, 96, 128, 200, 540)] == \
        [16, 16, 32, 48, 48, 64, 128, 128, 128, 128, 64]


def test_flops_per_image_imagenet64():
    """51.41 GFLOP per image per direction (measured with hooks)."""
    from idfcodec.packing import BlockGeometry, growths
    tot = 0
    for C, hw in ((12, 32 * 32), (24, 16 * 16), (48, 8 * 8)):
        a = int(C * 0.75)
        cg = BlockGeometry(a=a, depth=12, growth=growths(512, 12), n_head=C - a)
        tot += 8 * hw * cg.flops_per_pixel()
    for cin, out, hw in ((6, 12, 32 * 32), (12, 24, 16 * 16), (48, 96, 8 * 8)):
        pg = BlockGeometry(a=cin, depth=12, growth=growths(512, 12), n_head=out)
        tot += hw * pg.flops_per_pixel()
    assert abs(tot / 1e9 - 51.41) < 0.05, tot


# ------------------------------------------------------------------ mirror modules
@pytest.mark.parametrize("name", ["t1_idflows_2lvl", "t2_idflows_3lvl_leaky", "t3_cond_convcond",
                                  "t4_cond_s1_odd"])
def test_seeded_mirror_model_equals_reference(golden, name):
    from idfcodec import synthetic
    d = golden(f"flow_{name}.npz")
    cfg = yaml.safe_load(bytes(d["cfg_yaml"]).decode())
    sd = synthetic.build_model(cfg).state_dict()
    ref = {k[3:]: d[k] for k in d.files if k.startswith("sd/")}
    assert list(sd) == list(ref)
    for k in ref:
        assert np.array_equal(sd[k].numpy(), ref[k]), k


@pytest.mark.slow
def test_seeded_imagenet64_equals_reference(golden):
    from idfcodec import configs, synthetic
    d = golden("imagenet64_b2.npz")
    sd = synthetic.build_model(configs.get("imagenet64")).state_dict()
    assert list(sd) == bytes(d["param_names"]).decode().split("\n")
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    assert np.array_equal(sums, d["param_sums"])


def test_configs_restate_reference_yaml():
    """The built-in configs equal the reference's YAML files (tests/golden/configs: the
    reference's own settings files, stored unchanged)."""
    from idfcodec import configs
    from conftest import GOLDEN
    ref_dir = os.path.join(GOLDEN, "configs")
    assert len(configs.CONFIGS) == 4
    for n in configs.CONFIGS:
        assert configs.load_yaml(os.path.join(ref_dir, n + ".yaml")) == configs.get(n)


def test_registry_names():
    import flows  # noqa: F401
    from moduleregister import Register
    for n in ("IDFlows", "ConditionalFlows", "AdditiveCouple", "DenseBlock", "DenseLayer", "Prior",
              "ExtendDim", "DLogistic", "Round"):
        assert Register.get(n).__name__ == n
    with pytest.raises(Exception, match="Can not find object"):
        Register.get("NoSuchThing")


def test_product_modules_refuse_cpu_tensors():
    from idfcodec import configs, synthetic
    from idfcodec._lib import IdfError
    m = synthetic.build_model(configs.get("imagenet64"))
    with pytest.raises((IdfError, RuntimeError)):
        m.forward(torch.zeros(1, 3, 64, 64), None)
    with pytest.raises((IdfError, RuntimeError)):
        m.blocks[0]["flows"][1].dense(torch.zeros(1, 9, 4, 4))


# ------------------------------------------------------------------ bitstream
def test_bitstream_container_roundtrip():
    from idfcodec.codec import Bitstream
    g = torch.Generator().manual_seed(0)
    nw = torch.randint(0, 50, (6,), generator=g).to(torch.int64)
    st = torch.randint(-(2 ** 62), 2 ** 62, (6,), generator=g, dtype=torch.int64)
    w = torch.randint(-(2 ** 31), 2 ** 31 - 1, (int(nw.sum()),), generator=g, dtype=torch.int32)
    bs = Bitstream(2, [(6, 32, 32), (12, 16, 16), (48, 8, 8)], st, nw, w,
                   meta={"n_subpixels": 2 * 3 * 64 * 64})
    raw = bs.to_bytes()
    bs2 = Bitstream.from_bytes(raw)
    assert bs2.n_images == 2 and bs2.level_shapes == bs.level_shapes
    assert torch.equal(bs2.states, st) and torch.equal(bs2.nwords, nw) and torch.equal(bs2.words, w)
    assert bs2.bits() == 64 * 6 + 32 * int(nw.sum())
    assert len(raw) == 20 + 36 + 8 + 8 * 6 + 4 * 6 + 4 * int(nw.sum())
    with pytest.raises(ValueError):
        Bitstream.from_bytes(b"XXXX" + raw[4:])


def test_residual_container_roundtrip_and_source_size():
    """IDFR container: index code + flow streams; version 2 carries the pre-pad source size
    (config 5's 215x178 -> 216x184 ReplicationPad2d), version 1 streams still read."""
    import struct
    from idfcodec.codec import Bitstream
    from idfcodec.residual import ResidualBitstream
    nw = torch.tensor([2, 0, 1], dtype=torch.int64)
    st = torch.tensor([5, -7, 2 ** 40], dtype=torch.int64)
    w = torch.arange(3, dtype=torch.int32)
    flow = Bitstream(1, [(6, 4, 4), (12, 2, 2), (48, 1, 1)], st, nw, w)
    idx = torch.tensor([1, -2, 3], dtype=torch.int32)
    for src in (None, (215, 178)):
        rbs = ResidualBitstream(flow, idx, 1, (3, 216, 184), (27, 23), 8192, src)
        r2 = ResidualBitstream.from_bytes(rbs.to_bytes())
        assert r2.source_hw == src and r2.image_shape == (3, 216, 184) and r2.grid == (27, 23)
        assert r2.source_shape == (3,) + (src or (216, 184))
        assert torch.equal(r2.idx_words, idx) and torch.equal(r2.flow.words, w)
        assert r2.bits() == flow.bits() + 27 * 23 * 13
    raw = ResidualBitstream(flow, idx, 1, (3, 216, 184), (27, 23), 8192).to_bytes()
    v1 = raw[:4] + struct.pack("<H", 1) + raw[6:36] + raw[44:]   # drop the v2 size words
    r1 = ResidualBitstream.from_bytes(v1)
    assert r1.source_hw is None and torch.equal(r1.idx_words, idx)
    with pytest.raises(ValueError):
        ResidualBitstream.from_bytes(b"IDFX" + raw[4:])
    # header flags bit 0: the VQ decoder's conv mode (0 = exact f32, every older stream)
    assert r1.vq_conv == "f32" and struct.unpack_from("<H", raw, 6)[0] == 0
    x3 = ResidualBitstream(flow, idx, 1, (3, 216, 184), (27, 23), 8192, None, "x3").to_bytes()
    assert struct.unpack_from("<H", x3, 6)[0] == 1
    assert ResidualBitstream.from_bytes(x3).vq_conv == "x3"
    x3t = ResidualBitstream(flow, idx, 1, (3, 216, 184), (27, 23), 8192, None, "x3t").to_bytes()
    assert struct.unpack_from("<H", x3t, 6)[0] == 3
    assert ResidualBitstream.from_bytes(x3t).vq_conv == "x3t"
    for bad in (6, 2):  # an unknown bit; the taps bit without the ResBlocks' bit
        with pytest.raises(ValueError, match="flags"):
            ResidualBitstream.from_bytes(x3[:6] + struct.pack("<H", bad) + x3[8:])


# ------------------------------------------------------------------ coder chaining (F4)
def test_coder_decode_fix_roundtrips_with_oracle(golden, oracle, monkeypatch):
    """coder.Encode chains the state across levels; the reference Decode does not
    round-trip, the fixed Decode does.  Exercised on CPU with the
    oracle standing in for rans.rans (same list API)."""
    import coder

    def enc(state, n, x, m, s):
        st, w = oracle.encode(state, x[:n], m[:n], s[:n])
        return st, w.tolist()

    def dec(state, buf, n, m, s):
        # reference convention: buf, m, s reversed; result reversed
        st, out = oracle.decode(state, np.asarray(buf[::-1], np.uint32), n, np.asarray(m[::-1]),
                                np.asarray(s[::-1]))
        return st, out[::-1].astype(np.float64).tolist()

    monkeypatch.setattr(coder, "encode", enc)
    monkeypatch.setattr(coder, "decode", dec)
    d = golden("imagenet64_b2.npz")
    lat = [torch.from_numpy(d[f"latent{i}"]) for i in range(3)]
    mean = [torch.from_numpy(d[f"mean{i}"]) for i in range(3)]
    logs = [torch.from_numpy(d[f"logscale{i}"]) for i in range(3)]
    x, bufs = coder.Encode(lat, mean, logs)
    assert any(len(b) for b in bufs)
    x2, rec = coder.Decode(bufs, mean, logs, x)
    assert x2 == 1 << 32
    for a, b in zip(rec, lat):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ expf restatement
@pytest.mark.slow
def test_restated_expf_equals_libm_on_all_floats(tmp_path):
    exe = tmp_path / "expf_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "native", "expf_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "mismatches=0" in r.stdout


def test_bf16_weight_packing_layout():
    """bf16_weights: uint16 bf16 bits of the fp32 folded weights in the fragment order
    [slab][tap][k-block][n][8] that conv3_bf16.hip reads."""
    import numpy as np
    import torch
    from idfcodec.packing import bf16_weights
    rng = np.random.default_rng(4)
    n_alloc, C, ldw = 48, 52, 64
    w = rng.normal(0, 1, (n_alloc, 9, ldw)).astype(np.float32)
    w[:, :, C:] = 0
    b = bf16_weights(w, C)
    nslab = (C + 31) // 32
    assert b.shape == (nslab, 9, 4, n_alloc, 8) and b.dtype == np.uint16
    ref = torch.from_numpy(w).to(torch.bfloat16).float().numpy()
    back = torch.from_numpy(b.astype(np.int16)).view(torch.bfloat16).float().numpy()
    for s in range(nslab):
        for kb in range(4):
            for e in range(8):
                c = 32 * s + 8 * kb + e
                want = ref[:, :, c] if c < C else np.zeros((n_alloc, 9), np.float32)
                assert np.array_equal(back[s, :, kb, :, e].T, want)


def test_dx3_weight_packing_layout_and_prefix(golden):
    """dx3_weights: [slab][group][hi, lo][tap][nf][out][ch] f16 pairs with (hi + lo) 2^-k equal
    to the float64 weight within f16-pair precision, zeros past C (and past n_alloc in the last
    group); groups of up to 4 fragments (dx3_groups); pack_dense_block(dx3_cmax) packs them for
    the leading layers whose input is at most dx3_cmax wide, nothing after."""
    import numpy as np
    from idfcodec.packing import dx3_groups, dx3_weights, pack_dense_block
    assert [dx3_groups(n) for n in (16, 48, 64, 80, 128, 192)] == \
        [(1, 1), (3, 1), (4, 1), (4, 2), (4, 2), (4, 3)]
    rng = np.random.default_rng(6)
    for n_alloc, C, ldw, shape in ((48, 40, 48, (3, 1, 2, 9, 3, 16, 16)),
                                   (80, 36, 48, (3, 2, 2, 9, 4, 16, 16))):
        w = rng.normal(0, 0.05, (n_alloc, 9, ldw))
        w[:, :, C:] = 0
        d, ysc = dx3_weights(w, C)
        assert d.shape == shape and d.dtype == np.uint16
        f = d.view(np.float16).astype(np.float64)
        back = (f[:, :, 0] + f[:, :, 1]) * ysc               # slab, group, tap, nf, out, ch
        nft = shape[1] * shape[4]
        back = back.transpose(1, 3, 4, 2, 0, 5).reshape(nft * 16, 9, shape[0] * 16)
        assert np.abs(back[:n_alloc, :, :C] - w[:, :, :C]).max() <= 2.0 ** -20 * np.abs(w).max()
        assert not back[:, :, C:].any() and not back[n_alloc:].any()
    g = golden("flow_t1_idflows_2lvl.npz")
    cfg = yaml.safe_load(bytes(g["cfg_yaml"]).decode())
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    depth = cfg["couple"]["nn"]["depth"]
    assert depth >= 3
    pre = "blocks.0.flows.1.dense."
    full = pack_dense_block(sd, pre, depth, fold=True, wino=True, wx3=True, dx3=True)
    assert len(full.dx3_w) == depth
    k_in = full.geom.k_in
    part = pack_dense_block(sd, pre, depth, fold=True, wino=True, wx3=True, dx3=True,
                            dx3_cmax=k_in[1])
    assert len(part.dx3_w) == 2
    for a, b in zip(part.dx3_w, full.dx3_w):
        assert np.array_equal(a, b)


def test_bitstream_conv_flag_round_trips():
    import torch
    from idfcodec.codec import Bitstream
    st = torch.tensor([1 << 32, 5], dtype=torch.int64)
    nw = torch.tensor([1, 2], dtype=torch.int64)
    w = torch.tensor([7, 8, 9], dtype=torch.int32)
    for mode in ("x3", "f32", "halo", "gemm", "unfold", "bf16"):
        bs = Bitstream(1, [(6, 4, 4), (12, 2, 2)], st, nw, w, meta={"n_subpixels": 48, "conv": mode})
        back = Bitstream.from_bytes(bs.to_bytes())
        assert back.meta["conv"] == mode
    legacy = Bitstream(1, [(6, 4, 4), (12, 2, 2)], st, nw, w)  # no conv in meta: exact f32
    back = Bitstream.from_bytes(legacy.to_bytes())
    assert back.meta["conv"] == "f32"
    assert torch.equal(back.host_nwords, nw) and not back.host_nwords.is_cuda


def test_version1_container_without_conv_field():
    """ADVICE r2 (codec.py:432): version-1 files with flags 0 were written by every engine
    before the conv field existed.  They read as conv 'unrecorded', which every engine but a
    split-f16 one accepts (the pre-field behaviour); version-1 files with a conv code and
    version-2 files keep the exact check; an unrecorded file cannot be re-written as v2."""
    import struct
    from idfcodec.codec import VERSION, Bitstream
    shapes = [(6, 4, 4), (12, 2, 2)]
    st = torch.zeros(4, dtype=torch.int64)
    nw = torch.ones(4, dtype=torch.int64)
    raw = Bitstream(2, shapes, st, nw, torch.zeros(4, dtype=torch.int32),
                    meta={"conv": "f32"}).to_bytes()
    assert struct.unpack_from("<H", raw, 4)[0] == VERSION == 2
    v1 = raw[:4] + struct.pack("<HH", 1, 0) + raw[8:]
    old = Bitstream.from_bytes(v1)
    assert old.meta["conv"] == "unrecorded"
    for fam in ("f32", "halo", "gemm", "unfold", "bf16"):
        _codec_for(shapes, family=fam, wx3=False).check_bitstream(old)
    with pytest.raises(ValueError, match="predates the conv field"):
        _codec_for(shapes, family="x3").check_bitstream(old)
    with pytest.raises(ValueError, match="re-encode"):
        old.to_bytes()
    v1_x3 = raw[:4] + struct.pack("<HH", 1, 1) + raw[8:]
    assert Bitstream.from_bytes(v1_x3).meta["conv"] == "x3"
    with pytest.raises(ValueError, match="coded with 'bf16'"):
        _codec_for(shapes, family="x3").check_bitstream(
            Bitstream.from_bytes(raw[:4] + struct.pack("<HH", 2, 5) + raw[8:]))


def _codec_for(levels, family="x3", wx3=True):
    from types import SimpleNamespace
    from idfcodec.codec import ImageCodec
    c = ImageCodec.__new__(ImageCodec)
    # an fp32 engine without dx3 weights (FlowEngine.can_run's rule for it)
    c.engine = SimpleNamespace(levels=[SimpleNamespace(z=z, h=h, w=w) for z, h, w in levels],
                               conv_family=family, wx3=wx3,
                               can_run=lambda conv: conv == "f32" or (conv == "x3" and wx3))
    return c


def test_decode_rejects_mismatched_container():
    """A truncated, corrupted or other-config container raises before any device launch
    (the rANS decode indexes streams by (level, image): no out-of-bounds reads)."""
    import pytest
    import torch
    from idfcodec.codec import Bitstream
    shapes = [(6, 4, 4), (12, 2, 2)]
    c = _codec_for(shapes)

    def bs(n_img=2, ns=4, nwords=None, nw_total=None, sh=shapes, conv="x3"):
        nw = torch.tensor(nwords if nwords is not None else [1] * ns, dtype=torch.int64)
        tot = int(nw.sum()) if nw_total is None else nw_total
        return Bitstream(n_img, sh, torch.zeros(ns, dtype=torch.int64), nw,
                         torch.zeros(tot, dtype=torch.int32), meta={"conv": conv})
    c.check_bitstream(bs())  # well-formed
    c.check_bitstream(bs(conv="f32"))  # switchable mode
    with pytest.raises(ValueError, match="level shapes"):
        c.check_bitstream(bs(sh=[(6, 4, 4), (12, 4, 4)]))
    with pytest.raises(ValueError, match="level shapes"):
        c.check_bitstream(bs(sh=shapes[:1], ns=2))
    with pytest.raises(ValueError, match="streams"):
        c.check_bitstream(bs(ns=3))
    with pytest.raises(ValueError, match="negative"):
        c.check_bitstream(bs(nwords=[1, -1, 1, 1]))
    with pytest.raises(ValueError, match="word table"):
        c.check_bitstream(bs(nw_total=2))
    with pytest.raises(ValueError, match="coded with 'bf16'"):
        c.check_bitstream(bs(conv="bf16"))
    with pytest.raises(ValueError, match="coded with 'x3'"):
        _codec_for(shapes, family="f32", wx3=False).check_bitstream(bs())
    # a truncated container does not parse
    good = bs().to_bytes()
    with pytest.raises(ValueError):
        Bitstream.from_bytes(good[:-3])
    bad = bytearray(good)
    bad[6] = 0x3F  # unknown conv code in the flags
    with pytest.raises(ValueError):
        Bitstream.from_bytes(bytes(bad))


def test_earlier_build_fixture_headers(golden):
    """The earlier builds' fixtures (tests/golden/make_conv_fixture.py) read with their conv codes
    -- 6 ("dx3w16"), 7 ("dx3") -- and re-serialise byte for byte; their decodes are
    tests/test_gpu_codec.py's."""
    from idfcodec.codec import Bitstream
    for name, conv in (("imagenet64_code6_r4.npz", "dx3w16"), ("imagenet64_code7_r5.npz", "dx3")):
        d = golden(name)
        bs = Bitstream.from_bytes(d["bitstream"].tobytes())
        assert bs.meta["conv"] == conv and bs.n_images == d["images"].shape[0] == 4
        assert bs.to_bytes() == d["bitstream"].tobytes()  # re-serialises byte for byte


def test_fused_block_geometries():
    """The fused DenseBlock launch (idf_dx3_block_supported) takes exactly the geometries whose
    tiles hold whole images, with one output group and no split K: 16x16 and the packed 4x4
    images -- not 8x8 (split K: the per-layer launches are faster), 32x32 (four tiles an
    image), 27x23 or 2x2 (gutter bands crossing tiles), nor 128 outputs (two output groups)."""
    from idfcodec import _lib
    sup = _lib.lib().idf_dx3_block_supported
    for (H, W, N, bf), want in [((16, 16, 48, 0), 1), ((8, 8, 48, 0), 0), ((4, 4, 32, 0), 1),
                                ((16, 16, 48, 1), 1), ((8, 8, 48, 1), 0), ((32, 32, 48, 0), 0),
                                ((27, 23, 32, 0), 0), ((2, 2, 32, 0), 0), ((4, 4, 128, 0), 0),
                                ((64, 64, 48, 0), 0)]:
        assert sup(H, W, N, bf) == want, (H, W, N, bf)


# ------------------------------------------------------------------ fp32 GEMM dispatch
def test_gemm_launch_info_tile_n_matches_packing():
    """packing.tile_n restates the C tile_n "must match": it does, for every N in 1..1024, against
    the BN the launches use (idf_gemm_launch_info); a mismatch would under-allocate weight rows."""
    from idfcodec import _lib
    from idfcodec.packing import round_up, tile_n
    for N in range(1, 1025):
        info = _lib.gemm_launch_info(100, N)
        assert info["BN"] == tile_n(N), N
        assert info["n_tiles"] == -(-N // info["BN"]) and info["m_tiles"] == 2
        assert info["n_alloc_min"] == round_up(N, tile_n(N)) == info["n_tiles"] * info["BN"]
    out = (ctypes.c_int32 * len(_lib.GEMM_INFO_FIELDS))()
    L = _lib.lib()
    assert L.idf_gemm_launch_info(1, 1, None) == 1
    assert L.idf_gemm_launch_info(0, 1, out) == 1 and L.idf_gemm_launch_info(1, 0, out) == 1
    assert L.idf_gemm_launch_info(-5, 16, out) == 1 and L.idf_gemm_launch_info(1, 1, out) == 0


def _dense_blocks(sd):
    """(prefix, depth) of every DenseBlock in a state dict."""
    tail = "layers.0.layers.0.weight"
    out = []
    for k in sorted(sd):
        if k.endswith("." + tail):
            p = k[:-len(tail)]
            depth = 0
            while f"{p}layers.{depth}.layers.0.weight" in sd:
                depth += 1
            out.append((p, depth))
    return out


def _check_block_rows(pb):
    """The rows pack_dense_block allocates for w1, w3 and wh are the n_alloc_min of the launches
    dense_block_run makes with them (N = k_in[i], g_pad, n_head)."""
    from idfcodec._lib import gemm_launch_info
    g = pb.geom
    for P in (1, 300000):  # n_alloc_min does not depend on the row count
        for i in range(g.depth):
            assert pb.w1[i].shape[0] == pb.b1[i].shape[0] == pb.n1_alloc[i] == \
                gemm_launch_info(P, g.k_in[i])["n_alloc_min"], (i, g.k_in[i])
            assert pb.w3[i].shape[0] == pb.b3[i].shape[0] == pb.g_alloc == \
                gemm_launch_info(P, g.g_pad)["n_alloc_min"], (i, g.g_pad)
        assert pb.wh.shape[0] == pb.bh.shape[0] == pb.nh_alloc == \
            gemm_launch_info(P, g.n_head)["n_alloc_min"], g.n_head


@pytest.mark.parametrize("name", ["t1_idflows_2lvl", "t2_idflows_3lvl_leaky", "t3_cond_convcond",
                                  "t4_cond_s1_odd"])
def test_gemm_n_alloc_min_matches_packed_rows_golden(golden, name):
    from idfcodec.packing import pack_dense_block
    d = golden(f"flow_{name}.npz")
    sd = {k[3:]: d[k] for k in d.files if k.startswith("sd/")}
    blocks = _dense_blocks(sd)
    assert blocks
    for prefix, depth in blocks:
        for fold in (False, True):
            _check_block_rows(pack_dense_block(sd, prefix, depth, fold=fold))


def test_gemm_n_alloc_min_matches_packed_rows_imagenet64():
    from idfcodec import configs, synthetic
    from idfcodec.packing import pack_dense_block
    sd = {k: v.numpy() for k, v in synthetic.build_model(configs.get("imagenet64")).state_dict().items()}
    blocks = _dense_blocks(sd)
    assert len(blocks) == 27  # 3 levels x (8 couplings + 1 prior)
    for prefix, depth in blocks:
        _check_block_rows(pack_dense_block(sd, prefix, depth))


def test_gemm_bm_rule_thresholds():
    """The row tile is the tallest of 256 / 128 whose grid still has 1024 blocks, else 64: for
    each BN the smallest P that reports BM = 128 and BM = 256 (bisected from the info; BM never
    falls as P grows), the closed form of the rule, and the P just below each.  BN = 128 has BM 64
    and 128 only.  The dense case rows reach every BN and both arms of the block remap."""
    import gemm_cases as T
    from idfcodec._lib import gemm_launch_info

    def first(N, bm):
        lo, hi = 1, 1 << 22  # info(lo) < bm <= info(hi)
        assert gemm_launch_info(lo, N)["BM"] < bm <= gemm_launch_info(hi, N)["BM"]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if gemm_launch_info(mid, N)["BM"] >= bm:
                hi = mid
            else:
                lo = mid
        return hi

    seen = set()
    for N in list(T.WIDEST_N.values()) + [130, 200, 1]:
        bn = gemm_launch_info(1, N)["BN"]
        nt = gemm_launch_info(1, N)["n_tiles"]
        assert gemm_launch_info(1, N)["BM"] == 64
        p128 = first(N, 128)
        assert p128 == T.first_p(128, nt)
        assert gemm_launch_info(p128 - 1, N)["BM"] == 64
        info = gemm_launch_info(p128, N)
        assert info["BM"] == 128 and info["m_tiles"] * info["n_tiles"] >= T.MIN_BLOCKS
        seen |= {(64, bn), (128, bn)}
        if bn == 128:
            assert gemm_launch_info(1 << 30, N)["BM"] == 128
            continue
        p256 = first(N, 256)
        assert p256 == T.first_p(256, nt) and p256 > p128
        assert gemm_launch_info(p256 - 1, N)["BM"] == 128
        info = gemm_launch_info(p256, N)
        assert info["BM"] == 256 and info["m_tiles"] * info["n_tiles"] >= T.MIN_BLOCKS
        assert info["m_tiles"] == -(-p256 // 256)
        seen.add((256, bn))
    assert seen == T.ALL_TILES
    assert {bn: N for bn, N in T.WIDEST_N.items()} == \
        {gemm_launch_info(1, N)["BN"]: N for N in T.WIDEST_N.values()}
    # the dense table: every listed N, K, P at least once, every BN, both 64-vs-128 arms past 64,
    # a grid of fewer than 8 blocks and one of more than 8 that is no multiple of 8
    assert {r.N for r in T.DENSE} == set(T.DENSE_N) and {r.K for r in T.DENSE} == set(T.DENSE_K)
    assert {r.P for r in T.DENSE} == set(T.DENSE_P)
    infos = [gemm_launch_info(r.P, r.N) for r in T.DENSE]
    assert {i["BN"] for i in infos} == set(T.BNS) and {i["BM"] for i in infos} == {64}
    assert {gemm_launch_info(1, N)["BN"] for N in (65, 130, 200)} == {64, 128}
    grids = [i["m_tiles"] * i["n_tiles"] for i in infos]
    assert any(g < 8 for g in grids) and any(g > 8 and g % 8 for g in grids)
    # the 3x3 large-P rows: B = 64 at 64 x 64 is BM = 256, and some batch lands on BM = 128
    H, W, _, N = T.CONV3_LARGE
    assert gemm_launch_info(T.CONV3_LARGE_B256 * H * W, N)["BM"] == 256
    assert any(gemm_launch_info(B * H * W, N)["BM"] == 128 for B in range(1, 64))


def test_fold_interior_bias_is_the_tap_order_sum(golden):
    """pack_dense_block(fold=True): bfull[i] is, bit for bit, the fp32 sum b3 + vtap[0] + ... +
    vtap[8] in tap order -- the order of the kernel's border loop (flow_kernels.hip EPI_ACT_FOLD),
    so a border pixel with all nine taps in the image would get the interior pixels' bias."""
    from idfcodec.packing import pack_dense_block
    d = golden("flow_t2_idflows_3lvl_leaky.npz")
    cfg = yaml.safe_load(bytes(d["cfg_yaml"]).decode())
    sd = {k[3:]: d[k] for k in d.files if k.startswith("sd/")}
    n = 0
    for prefix, depth in _dense_blocks(sd):
        pb = pack_dense_block(sd, prefix, depth, cfg["couple"]["nn"]["layer"]["act"], fold=True)
        assert len(pb.bfull) == len(pb.vtap) == depth
        for i in range(depth):
            s = pb.b3[i].astype(np.float32)
            for tap in range(9):
                s = np.add(s, pb.vtap[i][tap], dtype=np.float32)
            assert pb.bfull[i].dtype == np.float32 and pb.bfull[i].shape == (pb.g_alloc,)
            assert np.array_equal(s.view(np.uint32), pb.bfull[i].view(np.uint32)), (prefix, i)
            # and the order matters for these weights: some other order gives other bits
            n += int(not np.array_equal(
                pb.bfull[i], np.add(pb.b3[i], pb.vtap[i][::-1].sum(0, dtype=np.float32),
                                    dtype=np.float32)))
    assert n > 0
