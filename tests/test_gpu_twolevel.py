"""TwoLevelFlows on the device: the split / merge kernels against the reference's tensors and
the integer restatement, forward against the sub-models and the reference's bpd, the codec's
exact round trip with grouped fine streams, the streams against the C oracle, batch invariance,
decode / encode lanes over whole groups, and sampling.  Tiny models only."""
import math

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(golden):
    return golden("twolevel_tiny.npz")


@pytest.fixture(scope="module")
def models(tiny):
    """{16: source 15x13 pad (1, 3), 2x2 windows, 4 patches; 32: source 30x27 pad (2, 5), 4x4
    windows, 16 patches} -- the fixture's sub-models under both paddings."""
    from idfcodec import synthetic
    cfg = yaml.safe_load(bytes(tiny["cfg_yaml"]).decode())
    cfg32 = dict(cfg, H=30, W=27, pad=[2, 5])
    return {16: synthetic.build_model(cfg).cuda(), 32: synthetic.build_model(cfg32).cuda()}


def _images(model, B, seed):
    from idfcodec import synthetic
    return synthetic.images(B, 3, model.H - model.pad[0], model.W - model.pad[1], seed=seed).cuda()


def _dequant(u8):
    k = u8.to(torch.int32)
    return (k + (k >= 128)).float() / 256


def _same_streams(a, b):
    assert a.group == b.group and a.n_images == b.n_images
    assert torch.equal(a.states, b.states) and torch.equal(a.nwords, b.nwords)
    assert torch.equal(a.words, b.words)
    assert a.meta["conv"] == b.meta["conv"]


# ------------------------------------------------------------------ 1. split / merge kernels
@pytest.mark.parametrize("which", ["2x2", "4x4"])
def test_split_kernel_equals_reference(tiny, which):
    from idfcodec.twolevel import Geometry, split_nchw
    if which == "2x2":
        u8, rx, px, g = tiny["image_u8"], tiny["rx"], tiny["px"], Geometry(3, 15, 13, 16, 16, 8, 8,
                                                                           8, 8)
    else:
        u8, rx, px = tiny["set2/image_u8"], tiny["set2/rx"], tiny["set2/px"]
        g = Geometry(3, 30, 27, 32, 32, 8, 8, 8, 8)
    u8 = torch.from_numpy(u8).cuda()
    for src in (u8, _dequant(u8)):
        got_rx, got_px, bad = split_nchw(g, src)
        assert int(bad.item()) == 0
        assert np.array_equal(got_rx.cpu().numpy(), rx), (which, src.dtype)
        assert np.array_equal(got_px.cpu().numpy(), px), (which, src.dtype)


@pytest.mark.parametrize("geom", [(3, 16, 16, 16, 16, 8, 8, 8, 8),     # no pad
                                  (3, 24, 24, 24, 24, 4, 8, 8, 8),     # 6x3 windows
                                  (3, 21, 19, 24, 24, 4, 8, 4, 12),    # 6x3 windows over a pad
                                  (1, 5, 7, 6, 9, 2, 3, 3, 3)],        # 3x3 windows, one channel
                         ids=["nopad16", "win6x3", "win6x3pad", "win3x3"])
def test_split_kernel_equals_restatement(geom):
    from idfcodec import synthetic
    from idfcodec.twolevel import Geometry, split_host, split_nchw
    g = Geometry(*geom)
    u8 = synthetic.images(3, g.C, g.Hs, g.Ws, seed=11)
    u8[0, :, :2, :3] = 255  # saturated windows
    u8[1, :, :6, :3] = torch.tensor([0, 1, 0], dtype=torch.uint8)  # 6x3 window sum 6: 1/3
    rx, px, _ = split_host(u8.numpy(), (g.Hp - g.Hs, g.Wp - g.Ws), (g.rh, g.rw), (g.fh, g.fw))
    for src in (u8.cuda(), _dequant(u8.cuda())):
        got_rx, got_px, bad = split_nchw(g, src)
        assert int(bad.item()) == 0
        assert np.array_equal(got_rx.cpu().numpy(), rx)
        assert np.array_equal(got_px.cpu().numpy(), px)


@pytest.mark.parametrize("geom", [(3, 15, 13, 16, 16, 8, 8, 8, 8), (3, 30, 27, 32, 32, 8, 8, 8, 8),
                                  (3, 24, 24, 24, 24, 4, 8, 8, 8)])
def test_merge_inverts_split_and_counts_off_grid(geom):
    from idfcodec import synthetic
    from idfcodec.twolevel import Geometry, device_merge, device_split
    g = Geometry(*geom)
    B = 3
    u8 = synthetic.images(B, g.C, g.Hs, g.Ws, seed=12).cuda()
    u8[0, 0, 0, :4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    rpm = torch.empty(B * g.rh * g.rw * 4, device="cuda")
    fpm = torch.empty(B * g.Hp * g.Wp * 4, device="cuda")
    device_split(g, u8, rpm, fpm)
    out = torch.empty_like(u8)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    device_merge(g, B, rpm, fpm, out, bad)
    assert int(bad.item()) == 0 and torch.equal(out, u8)
    # f32 output: the dequantised source
    outf = torch.empty(u8.shape, device="cuda")
    device_merge(g, B, rpm, fpm, outf)
    assert torch.equal(outf, _dequant(u8))
    # fine values half a grid step off: exactly the touched source pixels are counted.  Patch 0
    # is the image's top-left patch; its pixels (0, 0), (0, 1), (1, 0) lie inside the source.
    touched = [(0 * g.fw + 0) * 4 + 0, (0 * g.fw + 1) * 4 + 1, (1 * g.fw + 0) * 4 + 2]
    for i in touched:
        fpm[i] += 1.0 / 512
    if g.Wp > g.Ws:  # a pad column (patch 1 of the first patch row ends at x = Wp - 1 when there
        # are two patch columns): never written, never counted
        last_patch = g.Wp // g.fw - 1
        fpm[((last_patch * g.fh + 0) * g.fw + g.fw - 1) * 4] += 1.0 / 512
    bad.zero_()
    device_merge(g, B, rpm, fpm, out, bad)
    assert int(bad.item()) == len(touched)
    assert int((out != u8).sum().item()) <= len(touched)
    # f32 input off the grid is counted by the split, per source pixel
    x = _dequant(u8)
    x[1, 2, g.Hs - 1, g.Ws - 1] += 1.0 / 1024  # the corner the pad replicates
    x[2, 0, 0, 0] = float("nan")
    bad.zero_()
    device_split(g, x, rpm, fpm, bad)
    assert int(bad.item()) == 2


# ------------------------------------------------------------------ 2. forward
# bpd / bpd1 / bpd2 against the reference's recorded values (fp32 torch on the CPU).  The bound
# is max(2 x the difference seen on the first MI355X run, 1e-4), as the flip bounds of
# test_gpu_flow.py were set; that run differed by 5.1e-6 / 1.4e-6 / 3.5e-6 (of 16.46 / 10.08 /
# 10.02 bits per sub-pixel), so the floor holds.
BPD_BOUND = 1e-4


def test_forward_equals_submodels_and_reference_bpd(tiny, models):
    model = models[16]
    assert model.batchsize == 3
    x = torch.from_numpy(tiny["input"]).cuda()
    lat, mean, logs, bpd, bpd1, bpd2, logv = model.forward(x, "logv", train=False)
    assert logv == "logv"
    rx, px = model.split(x)
    assert np.array_equal(rx.cpu().numpy(), tiny["rx"])
    assert np.array_equal(px.cpu().numpy(), tiny["px"])
    assert px.shape[0] == 8  # chunks of 3, 3 and 2: every patch's latents come back
    r = model.rough.forward(rx, None)
    f = model.fine.forward(px, None)
    for i, part in enumerate((r, f)):
        assert torch.equal(lat[i], part[0][0]), i
        assert torch.equal(mean[i], part[1][0]), i
        assert torch.equal(logs[i], part[2][0]), i
    assert lat[1].shape == (8, 12, 4, 4) and lat[0].shape == (2, 3, 8, 8)
    # the reference formula (flows.py:219-241) over the mirror's own log_likelihood
    logP, _ = model.rough.log_likelihood(*r[:3])
    want1 = torch.mean(-logP, dim=0).item() / math.log(2)
    want2 = 0.0
    for i in range(3):
        sl = slice(3 * i, 3 * i + 3)
        logP, _ = model.fine.log_likelihood([f[0][0][sl]], [f[1][0][sl]], [f[2][0][sl]])
        want2 += torch.mean(-logP, dim=0).item() / math.log(2) * logP.shape[0]
    want2 /= 8
    want = (want1 * 8 * 8 + want2 * 16 * 16) / 15 / 13
    assert (bpd, bpd1, bpd2) == (want, want1, want2)
    # against the reference's recorded values (fp32 torch on the CPU, batchsize 3)
    ref = tiny["bpd_bs3"]
    diffs = [abs(a - float(b)) for a, b in zip((bpd, bpd1, bpd2), ref)]
    print("bpd / bpd1 / bpd2:", (bpd, bpd1, bpd2), "reference:", ref.tolist(), "diff:", diffs)
    assert max(diffs) < BPD_BOUND, diffs


# ------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("size", [16, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_round_trip_exact(models, size, B):
    from idfcodec.twolevel import TwoLevelBitstream
    model = models[size]
    n = model.ratio[0] * model.ratio[1]
    row = model.W // model.fine.W
    img = _images(model, B, seed=20 + B)
    for group in (1, row, n):
        tbs = model.encode(img, group=group)
        assert tbs.group == group and tbs.fine.n_streams == B * n // group
        assert tbs.rough.n_streams == B and tbs.rough.group == 1
        raw = tbs.to_bytes()
        back = TwoLevelBitstream.from_bytes(raw, device="cuda")
        assert back.group == group
        out, info = model.decode(back)
        assert info["ok"], (size, B, group)
        assert out.dtype == torch.uint8 and torch.equal(out, img), (size, B, group)
        assert tbs.bits() == 64 * (B + B * n // group) + 32 * (
            tbs.rough.total_words() + tbs.fine.total_words())
    assert model.encode(img).group == row  # the default: one row of the patch grid
    with pytest.raises(ValueError, match="group"):
        model.encode(img, group=3)  # 4 and 16 patches per image
    with pytest.raises(ValueError, match="group"):
        model.encode(img, group=2 * n)  # would span two images
    with pytest.raises(ValueError, match="shape"):
        model.encode(img[:, :, :-1])


# ------------------------------------------------------------------ 4. the oracle
def test_fine_streams_equal_oracle_and_ungrouped_codec(models, oracle):
    from idfcodec.codec import grouped_stream_offsets
    model = models[32]
    B, G, n = 3, 4, 16
    img = _images(model, B, seed=31)
    fc = model.fine.codec()
    assert fc.enc_lanes == 1
    tbs = model.encode(img, group=G)
    assert tbs.fine.n_streams == 12
    feng = model.fine.engine()
    ws = feng.workspace(B * n, 0)  # the one-pass encode's workspace: the device's own latents
    off = np.asarray(grouped_stream_offsets([L.n_sym for L in feng.levels], B * n, G))
    assert np.array_equal(off, fc.coder.sym_off(B * n, G).cpu().numpy())
    assert off.size == 13 and off[1] == 4 * 192
    fs, words, nw, status = oracle.encode_streams(off, ws["lat"].cpu().numpy(),
                                                  ws["mean"].cpu().numpy(),
                                                  ws["scale"].cpu().numpy())
    assert (status == 0).all()
    assert np.array_equal(tbs.fine.states.cpu().numpy().view(np.uint64), fs)
    assert np.array_equal(tbs.fine.nwords.cpu().numpy(), nw)
    got = tbs.fine.words.cpu().numpy().view(np.uint32)
    woff = np.concatenate([[0], np.cumsum(nw)])
    assert woff[-1] == got.size and got.size > 0
    for k in range(12):
        assert np.array_equal(got[woff[k]:woff[k + 1]], words[off[k]:off[k] + nw[k]]), k
    # one patch per stream: the fine part is the plain codec's stream of the patches
    one = model.encode(img, group=1)
    _, px = model.split(_dequant(img))
    plain = fc.encode_nchw(px)
    _same_streams(one.fine, plain)
    assert one.fine.to_bytes() == plain.to_bytes()
    rx, _ = model.split(_dequant(img))
    _same_streams(one.rough, model.rough.codec().encode_nchw(rx))


# ------------------------------------------------------------------ 5. batch invariance
@pytest.mark.parametrize("group", [4, 16])
def test_image_codes_identically_alone(models, group):
    model = models[32]
    img = _images(model, 3, seed=41)
    full = model.encode(img, group=group)
    alone = model.encode(img[1:2].contiguous(), group=group)
    per = 16 // group
    for part, k in ((full.rough, 1), (full.fine, per)):
        a = alone.rough if part is full.rough else alone.fine
        sl = slice(k * 1, k * 2)
        assert torch.equal(part.states[sl], a.states)
        assert torch.equal(part.nwords[sl], a.nwords)
        wo = part.word_offsets()
        w0 = int(wo[sl][0])
        assert torch.equal(part.words[w0:w0 + int(a.nwords.sum())], a.words)
        assert int(a.nwords.sum()) > 0
    out, info = model.decode(alone)
    assert info["ok"] and torch.equal(out, img[1:2])


# ------------------------------------------------------------------ 6. lanes
def test_lanes_hold_whole_groups(models):
    model = models[32]
    fc = model.fine.codec()
    img = _images(model, 3, seed=51)  # 48 fine patches
    calls = []
    enc_lanes = fc._encode_lanes

    def spy(*a, **k):
        calls.append(a[2])  # nl
        return enc_lanes(*a, **k)

    fc._encode_lanes = spy
    lanes, enc = fc.lanes, fc.enc_lanes
    try:
        for G, nl in ((4, 2), (16, 1)):
            assert fc._n_lanes(48, G) == nl  # lanes of 24 patches: no multiple of 16
            fc.enc_lanes = 1
            ref = model.encode(img, group=G)
            fc.lanes = 1
            ref_out, ref_info = model.decode(ref)
            assert ref_info["ok"] and torch.equal(ref_out, img)
            fc.lanes = 2
            out, info = model.decode(ref)
            torch.cuda.synchronize()
            assert info["ok"] and torch.equal(out, img), G
            for key in ("final_states", "status"):
                assert torch.equal(info["fine"][key], ref_info["fine"][key]), (G, key)
            # the encode side (IDF_ENC_LANES=2 through the codec attribute)
            calls.clear()
            fc.enc_lanes = 2
            got = model.encode(img, group=G)
            torch.cuda.synchronize()
            assert calls == ([2] if nl == 2 else []), (G, calls)
            _same_streams(got.fine, ref.fine)
            _same_streams(got.rough, ref.rough)
            assert torch.equal(got.fine.status, ref.fine.status)
            out, info = model.decode(got)
            assert info["ok"] and torch.equal(out, img), G
    finally:
        fc.lanes, fc.enc_lanes = lanes, enc
        del fc._encode_lanes


# ------------------------------------------------------------------ 7. sampling
def test_generated_from_noise_composes_submodels(models):
    from idfcodec.twolevel import merge_host
    model = models[16]
    g = torch.Generator().manual_seed(7)
    B = 2
    zr = torch.randn(B, 3, 8, 8, generator=g).cuda()
    zf = torch.randn(B, 12 * 4, 4, 4, generator=g).cuda()
    x = model.generated_from_noise([zr, zf])
    assert x.shape == (B, 3, 15, 13) and x.dtype == torch.float32
    rx = model.rough.generated_from_noise([zr])
    fx = model.fine.generated_from_noise([zf.view(-1, 12, 4, 4)])
    want = merge_host(rx.cpu().numpy(), fx.cpu().numpy(), model.pad, (model.H, model.W))
    assert np.array_equal(x.cpu().numpy(), want)
    model.inverse()  # flows.py:272-274: forwards to both sub-models
