"""tests/golden/make_golden_tiled.py -- generates tests/golden/tiled_tiny.npz.

Runs ONLY where the reference tree exists (the build container; IDF_REFERENCE overrides its
place), as make_golden_twolevel.py does: the reference's Patching (extenddim.py:41-57) is imported
from there with bytecode writing disabled, so nothing is written into that tree.  The fixture
holds data only: seeded uint8 images of several sizes and, for each, the output of the
reference's own modules -- nn.ReplicationPad2d((0, pw, 0, ph)) (trainer.py:62) up to the next
multiple of the tile, then Patching(Hp, Wp, th, tw).forward -- which idfcodec.tiled's rule
restates.  No reference source travels.
Re-run:  python tests/golden/make_golden_tiled.py

Sets: three-channel images of (1,1), (16,16), (17,16), (5,40), (37,21) cut at 16x16; a
one-channel image of (25,9) cut at 12x8.  Images of four pixels or more start with the bytes
0, 127, 128, 255 (both sides of the dequantiser's step at 128); (17,16) and (37,21) end in 128
at the corner that the pad replicates.
"""
from __future__ import annotations

import os
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

from extenddim import Patching  # noqa: E402

SETS = [  # (C, th, tw, [(H, W)])
    (3, 16, 16, [(1, 1), (16, 16), (17, 16), (5, 40), (37, 21)]),
    (1, 12, 8, [(25, 9)]),
]


def image(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (C, H, W), generator=g, dtype=torch.uint8)
    if H * W >= 4:
        u8.view(C, -1)[:, :4] = torch.tensor([0, 127, 128, 255], dtype=torch.uint8)
    if (H, W) in ((17, 16), (37, 21)):
        u8[:, -1, -1] = 128
    return u8


def tiles_reference(u8, th, tw):
    C, H, W = u8.shape
    Hp, Wp = -(-H // th) * th, -(-W // tw) * tw
    x = u8.to(torch.float32)[None]
    xp = torch.nn.ReplicationPad2d(padding=(0, Wp - W, 0, Hp - H))(x)
    px, _ = Patching(Hp, Wp, th, tw)(xp, None)
    out = px.to(torch.uint8)
    assert torch.equal(out.to(torch.float32), px)
    return out


def main():
    out = {}
    k = 0
    for C, th, tw, sizes in SETS:
        for H, W in sizes:
            u8 = image(C, H, W, seed=70 + k)
            out[f"img{k}"] = u8.numpy()
            out[f"tiles{k}"] = tiles_reference(u8, th, tw).numpy()
            out[f"tile_hw{k}"] = np.asarray([th, tw], np.int64)
            k += 1
    out["n"] = np.int64(k)
    path = os.path.join(HERE, "tiled_tiny.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "images", k)


if __name__ == "__main__":
    main()
