"""Where a dx3 block spends its time outside the slab loop (a tools/dx3_build_knobs.sh build with
-DIDF_DX3_TL=1, loaded through IDF_LIB_PATH).  Block timelines (s_memrealtime, 100 MHz), p50 over
the blocks of the last launch, microseconds:

* the per-layer kernel at the 32 x 32 level (128 images: 256 two-tile blocks) at c = 12 / 232 /
  496 and at the 8 x 8 level (256 images, split K) at a layer of four slabs a chunk: prologue
  (entry -> the first slab's DMA issued), slab-0 wait, k-loop, the epilogue's output loop (outputs
  formed, fp32 and split stores issued), its tail (head sums and their stores), the block;
* the fused DenseBlock kernel at the 16 x 16 level (imagenet64's first coupling block there, 256
  images): per layer the set-up (layer start -> past the first slab's barrier), the loop, the
  epilogue with its drain and barrier, and the gap from a layer's loop end to the next layer's
  first slab barrier."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "finalproject-losslessimagecompression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402

import kbench  # noqa: E402
from idfcodec import _lib  # noqa: E402
from idfcodec._lib import dx3_launch_info, lib  # noqa: E402


def p50(vals):
    vals = sorted(v / 100.0 for v in vals)
    return vals[len(vals) // 2] if vals else float("nan")


def layer_rows(lvl, layer, B):
    hw, a = ((32, 9), (16, 18), (8, 36))[lvl]
    c = (a + 3) // 4 * 4 + layer * 44
    os.environ.update(KB_ONLY="dx3", KB_LEVELS=str(lvl), KB_LAYERS=str(layer), KB_B=str(B), KB_REPS="3")
    kbench.main()
    torch.cuda.synchronize()
    info = dx3_launch_info(B, hw, hw, c, 44)
    nblk = -(-info["ntiles"] // info["T"]) * info["ngroup"] * info["nchunk"]
    buf = (ctypes.c_ulonglong * (4096 * 8))()
    assert lib().idf_dx3_timeline(buf) == 0
    rows = [[buf[b * 8 + j] for j in range(8)] for b in range(min(nblk, 4096))]
    rows = [r for r in rows if r[0]]
    # blocks that ran the epilogue in THIS launch (split K: the tile's last block -- another
    # block's epilogue stamps are left over from an earlier launch and lie before its hand-off)
    done = [r for r in rows if r[5] > max(r[3], r[6])]
    for r in done:
        r[4] = r[4] if r[4] > r[3] else 0
    print(f"layer kernel {hw}x{hw} B={B} c={c} blocks={len(rows)} ({len(done)} with an epilogue) "
          f"chunks={info['nchunk']}")
    print(f"  prologue {p50(r[1] - r[0] for r in rows):6.2f}  slab-0 wait {p50(r[2] - r[1] for r in rows):6.2f}"
          f"  prologue+wait {p50(r[2] - r[0] for r in rows):6.2f}  k-loop {p50(r[3] - r[2] for r in rows):7.2f}"
          f"  output loop {p50(r[7] - (r[4] or r[3]) for r in done):6.2f}"
          f"  tail {p50(r[5] - r[7] for r in done):6.2f}"
          f"  epilogue {p50(r[5] - (r[4] or r[3]) for r in done):6.2f}"
          f"  block {p50(max(r[5], r[6], r[3]) - r[0] for r in rows):7.2f}", flush=True)


def block_rows(B=256):
    from idfcodec import configs, synthetic
    from idfcodec._lib import IdfHeadOut, ptr
    model = synthetic.build_model(configs.get("imagenet64")).cuda()
    eng = model.engine()
    Lv, blk = eng.levels[1], eng.couple[1][0]
    assert blk.desc.fuse_layers == 1 and lib().idf_dx3_block_supported(Lv.h, Lv.w, blk.geom.g_pad, 0) == 1
    P = B * Lv.h * Lv.w
    k0 = blk.geom.k_in[0]
    ws = eng.workspace(B, 1)
    g = torch.Generator().manual_seed(11)
    x = (torch.randint(-64, 64, (P, k0), generator=g).float() / 256).cuda()
    x[:, Lv.a:] = 0.0
    ws["feat"].view(-1, eng.ld_feat)[:P, :k0] = x
    out = torch.zeros(P, 16, device="cuda")
    h = IdfHeadOut()
    h.mode, h.out, h.ld_out = _lib.EPI_STORE, ptr(out), 16
    for _ in range(3):
        blk.run(_lib.stream_ptr(), B, Lv.h, Lv.w, ptr(ws["feat"]), eng.ld_feat, ptr(ws["tmp"]),
                eng.tmp_pitch(ws, P), h)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (1024 * 16 * 4))()
    assert lib().idf_dx3_timeline_ml(buf) == 0
    depth = blk.geom.depth
    t = [[[buf[(b * 16 + li) * 4 + j] for j in range(4)] for li in range(depth)] for b in range(min(B, 1024))]
    print(f"fused block kernel {Lv.h}x{Lv.w} B={B} layers={depth} blocks={len(t)}")
    tot = [0.0] * 4
    for li in range(depth):
        setup = p50(b[li][1] - b[li][0] for b in t)
        loop = p50(b[li][2] - b[li][1] for b in t)
        epi = p50(b[li][3] - b[li][2] for b in t)
        gap = p50(b[li + 1][1] - b[li][2] for b in t) if li + 1 < depth else float("nan")
        for i, v in enumerate((setup, loop, epi, gap)):
            tot[i] += 0.0 if v != v else v
        print(f"  layer {li:2d} c={blk.geom.k_in[li]:4d}  set-up {setup:6.2f}  loop {loop:7.2f}  "
              f"epilogue+drain {epi:6.2f}  gap to next first-slab barrier {gap:6.2f}")
    print(f"  sums        set-up {tot[0]:6.2f}  loop {tot[1]:7.2f}  epilogue+drain {tot[2]:6.2f}  "
          f"gaps {tot[3]:6.2f}  block {p50(b[depth - 1][3] - b[0][0] for b in t):7.2f}", flush=True)


if __name__ == "__main__":
    print("lib", _lib.LIB_PATH)
    for lvl, layer, B in ((0, 0, 128), (0, 5, 128), (0, 11, 128), (2, 5, 256)):
        layer_rows(lvl, layer, B)
    block_rows()
