"""tests/golden/make_golden_twolevel.py -- generates tests/golden/twolevel_tiny.npz.

Runs ONLY where the reference tree exists (the build container; the same place as
make_golden.py reads it from, IDF_REFERENCE overrides it): the reference's TwoLevelFlows
(flows.py:184-274) is imported from there with a `colorama` stub, bytecode writing disabled so
nothing is written into that tree.  The fixture holds data only
(config, weights, inputs, the reference's outputs); no reference source travels.
Re-run:  python tests/golden/make_golden_twolevel.py

Model: source 15x13, pad (1, 3) -> 16x16; rough IDFlows 8x8 (scale 1, 2x2 pool windows), fine
IDFlows 8x8 patches (scale 2); batchsize 3 (the 8 patches of B = 2 images make chunks of 3, 3
and 2).  Weights and images: the seeded recipe of make_golden.py / idfcodec.synthetic.
A second image set at 30x27, pad (2, 5) -> 32x32 pins the 4x4 windows (u8, rx, px only).
"""
from __future__ import annotations

import copy
import os
import random
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("IDF_REFERENCE", "/root/reference")

sys.modules.setdefault("colorama", types.SimpleNamespace(reinit=None))
sys.path.insert(0, REF)

import flows as ref_flows  # noqa: E402
import yaml  # noqa: E402
from extenddim import Patching  # noqa: E402

torch.set_num_threads(8)


def dense(growth, depth, act="ReLU"):
    return {"name": "DenseBlock", "growth_channel": growth, "depth": depth,
            "layer": {"name": "DenseLayer", "act": act}}


def flows_cfg(nflows, H, W, cg, cd, pg, pd, scale):
    return {"name": "IDFlows", "nflows": nflows, "nbits": 8, "nsplit": 1, "H": H, "W": W, "C": 3,
            "couple": {"name": "AdditiveCouple", "split": 0.75, "nn": dense(cg, cd),
                       "round": {"name": "Round", "nbits": 8}},
            "extenddim": {"name": "ExtendDim", "scale": scale},
            "prior": {"name": "Prior", "round": {"name": "Round", "nbits": 8},
                      "nn": dense(pg, pd)},
            "distribution": {"name": "DLogistic"},
            "round": {"name": "Round", "nbits": 8}}


CFG = {"name": "TwoLevelFlows", "H": 15, "W": 13, "C": 3, "pad": [1, 3],
       "fine_flows": flows_cfg(2, 8, 8, 24, 3, 16, 2, 2),
       "rough_flows": flows_cfg(2, 8, 8, 16, 2, 16, 2, 1),
       "batchsize": 3}
SET2 = {"H": 30, "W": 27, "pad": [2, 5]}  # 32x32: 4x4 windows over the same 8x8 rough image


def build_model(cfg):
    cfg = copy.deepcopy(cfg)
    random.seed(0)
    torch.manual_seed(0)
    model = ref_flows.NNFlows.get(cfg.pop("name"))(**cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _, m in model.named_modules():
            if type(m).__name__ == "DenseBlock":
                head = m.layers[-1]
                head.weight.copy_(torch.randn(head.weight.shape, generator=g) * 0.05)
                head.bias.copy_(torch.randn(head.bias.shape, generator=g) * 0.05)
    return model.eval()


def dequant(u8):
    """trainer.py:101,131-136: ToTensor (k/255) then Round(nbits=8)."""
    x = u8.to(torch.float32) / 255.0
    return torch.round(x * 256) / 256


def images(B, C, H, W, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, C, H, W), generator=g, dtype=torch.uint8)


def split_reference(x, pad, rough_hw, fine_hw):
    """flows.py:213-215, 225 with the reference's own modules."""
    xp = torch.nn.ReplicationPad2d(padding=(0, pad[1], 0, pad[0]))(x)
    H, W = xp.shape[2:]
    rx = ref_flows.Round(nbits=8)(torch.nn.AdaptiveAvgPool2d(tuple(rough_hw))(xp))
    fx = xp - torch.nn.AdaptiveAvgPool2d((H, W))(rx)
    px, _ = Patching(H, W, fine_hw[0], fine_hw[1])(fx, None)
    return xp, rx, fx, px


def count_ties(u8, pad, rough_hw):
    """pool windows whose mean lies exactly between two grid values"""
    k = u8.numpy().astype(np.int64)
    k = k + (k >= 128)
    kp = np.pad(k, ((0, 0), (0, 0), (0, pad[0]), (0, pad[1])), mode="edge")
    B, C, H, W = kp.shape
    wh, ww = H // rough_hw[0], W // rough_hw[1]
    S = kp.reshape(B, C, rough_hw[0], wh, rough_hw[1], ww).sum(axis=(3, 5))
    return int((2 * (S % (wh * ww)) == wh * ww).sum())


def main():
    model = build_model(CFG)
    B = 2
    u8 = images(B, 3, CFG["H"], CFG["W"], seed=2)
    x = dequant(u8)
    out = {"cfg_yaml": np.frombuffer(yaml.safe_dump(CFG).encode(), np.uint8),
           "image_u8": u8.numpy(), "input": x.numpy()}
    out.update({"sd/" + k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    out["latents_shape"] = np.asarray(model.latents_shape, np.int64)
    out["ratio"] = np.asarray(model.ratio, np.int64)
    out["padded_hw"] = np.asarray([model.H, model.W], np.int64)
    rough_hw, fine_hw = (model.rough.H, model.rough.W), (model.fine.H, model.fine.W)
    with torch.no_grad():
        xp, rx, fx, px = split_reference(x, CFG["pad"], rough_hw, fine_hw)
        # the model's own plumbing gives the same tensors
        assert torch.equal(model.pad2d(x), xp) and torch.equal(model.round(model.pool(xp)), rx)
        assert torch.equal(xp - model.invpool(rx), fx)
        out.update(x_pad=xp.numpy(), rx=rx.numpy(), fx=fx.numpy(), px=px.numpy())
        # bpd at the config's batchsize 3 (three chunks; line 242 then returns only the last
        # chunk's latents, so the tensors are recorded from a one-chunk pass below)
        _, _, _, bpd, bpd1, bpd2, _ = model.forward(x, None, train=False)
        out["bpd_bs3"] = np.asarray([bpd, bpd1, bpd2], np.float64)
        model.batchsize = px.shape[0]
        lat, mean, logs, bpd, bpd1, bpd2, _ = model.forward(x, None, train=False)
        model.batchsize = CFG["batchsize"]
        out["bpd_one_chunk"] = np.asarray([bpd, bpd1, bpd2], np.float64)
        for i in range(2):
            out[f"latent{i}"] = lat[i].numpy()
            out[f"mean{i}"] = mean[i].numpy()
            out[f"logscale{i}"] = logs[i].numpy()
        assert lat[1].shape[0] == px.shape[0] == B * model.ratio[0] * model.ratio[1]
    ties = count_ties(u8, CFG["pad"], rough_hw)
    assert ties >= 1, "the 2x2 set holds no exact rounding tie"
    out["n_ties"] = np.int64(ties)
    # 4x4 windows
    u8b = images(B, 3, SET2["H"], SET2["W"], seed=2)
    with torch.no_grad():
        _, rxb, _, pxb = split_reference(dequant(u8b), SET2["pad"], rough_hw, fine_hw)
    tiesb = count_ties(u8b, SET2["pad"], rough_hw)
    assert tiesb >= 1, "the 4x4 set holds no exact rounding tie"
    out.update({"set2/image_u8": u8b.numpy(), "set2/rx": rxb.numpy(), "set2/px": pxb.numpy(),
                "set2/pad": np.asarray(SET2["pad"], np.int64), "set2/n_ties": np.int64(tiesb)})
    path = os.path.join(HERE, "twolevel_tiny.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "ties", ties, tiesb)


if __name__ == "__main__":
    main()
