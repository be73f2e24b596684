"""Throughput and stream overhead of the TwoLevelFlows codec on one GPU.

configs/config_twolevel.yaml's geometry (215x178 images padded to 216x184; a 27x23 rough
image, 621 fine 8x8 patches per image), seeded synthetic weights (the config's checkpoint is
absent), a batch of 8 synthetic uint8 images resident in HBM.  One step = TwoLevelCodec.encode
then decode at the default stream group (one row of the patch grid, 23 patches).  Prints one
JSON line: encode / decode ms and Mpx/s of the source pixels, the exactness of every timed
round trip, and for stream groups 1, 23 and 621 the bits of the two parts, the bits per
sub-pixel and the share the streams' final states take.  With random weights and random pixels
the bits per sub-pixel say nothing about a trained model; the differences between groups do
(the words hardly change, the 64-bit states go from one per patch to one per image).

  python tools/bench_twolevel.py [--batch B] [--steps K] [--warmup W]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "finalproject-losslessimagecompression_amd"))

import torch  # noqa: E402

GROUPS = (1, 23, 621)


def run(batch: int = 8, steps: int = 5, warmup: int = 1) -> dict:
    from idfcodec import configs, synthetic
    from idfcodec.twolevel import TwoLevelBitstream
    cfg = configs.get_twolevel("config_twolevel")
    model = synthetic.build_model(cfg).cuda()
    Hs, Ws = cfg["H"], cfg["W"]
    img = synthetic.images(batch, 3, Hs, Ws, seed=2).cuda()
    codec = model.codec()
    n = codec.geometry.patches
    for _ in range(warmup):
        codec.decode(codec.encode(img))
    torch.cuda.synchronize()
    te = td = 0.0
    n_exact = 0
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tbs = codec.encode(img)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out, info = codec.decode(tbs, verify=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        te += t1 - t0
        td += t2 - t1
        n_exact += int(torch.equal(out, img))
    groups = {}
    for G in GROUPS:
        t = codec.encode(img, group=G)
        back = TwoLevelBitstream.from_bytes(t.to_bytes(), device="cuda")
        out, info = codec.decode(back)
        nsub_fine = batch * n * 3 * codec.geometry.fh * codec.geometry.fw
        groups[str(G)] = {
            "fine_streams": t.fine.n_streams, "rough_bits": t.rough.bits(),
            "fine_bits": t.fine.bits(), "bits": t.bits(), "bpd": round(t.bpd(), 5),
            "fine_state_bits_per_padded_subpixel": round(64 * t.fine.n_streams / nsub_fine, 5),
            "state_share": round(64 * (t.fine.n_streams + t.rough.n_streams) / t.bits(), 5),
            "container_bytes": len(t.to_bytes()),
            "round_trip_exact": bool(info["ok"]) and bool(torch.equal(out, img))}
    px = batch * Hs * Ws
    return {
        "metric": "encode+decode Mpixels/s (config_twolevel, bit-exact round trip)",
        "value": round(px * steps / (te + td) / 1e6, 4), "unit": "Mpx/s", "n_gpus": 1,
        "batch": batch, "image": [3, Hs, Ws], "coded_image": [3, model.H, model.W],
        "patches_per_image": n, "default_group": codec.default_group(),
        "steps": steps, "warmup": warmup, "round_trip_exact_steps": f"{n_exact}/{steps}",
        "encode_ms": round(te / steps * 1e3, 2), "decode_ms": round(td / steps * 1e3, 2),
        "encode_mpx_s": round(px * steps / te / 1e6, 4),
        "decode_mpx_s": round(px * steps / td / 1e6, 4),
        "conv": {"rough": tbs.rough.meta["conv"], "fine": tbs.fine.meta["conv"]},
        "groups": groups, "data": "synthetic uint8, seeded weights"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(run(a.batch, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
