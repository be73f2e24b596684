"""N-way interleaved rANS streams (Bitstream.ways) against the one-state streams, on one GPU.

  python tools/bench_ways.py [--lib PATH] [--reps 20] [--steps 5] [--warmup 2] [--skip-e2e]

(a) Kernel level: imagenet64's three levels at B = 256 (256 streams of 6144, 3072 and 3072
    symbols), latents and priors from one real encode of seeded synthetic images.  Per level and
    ways in 1, 8, 16, 32, 64: the device time (events) of one encode call (prep + chain) and one
    decode call, 20 launches after 3 warm-ups, the ways alternating launch by launch inside one
    process; every decode is checked against the latents.  --lib PATH: the one-state (ways = 1)
    calls are taken from another build of the library, loaded beside this one (a build from
    before the interleaved kernels joined rans_kernels.hip: the yardstick is then code that
    this change cannot have touched).
(b) End to end: model.encode / model.decode at B = 256 and B = 4 and one decode_region over
    4 tiles of a 256x256 image, ways 1, 8, 64 alternating step by step, every round trip
    checked; bits and state bits per sub-pixel.
Prints one JSON line.  With seeded weights and random pixels the bits per sub-pixel say nothing
about a trained model; the state bits do not depend on the data.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "finalproject-losslessimagecompression_amd"))

import torch  # noqa: E402

WAYS = (1, 8, 16, 32, 64)
L = 1 << 32


def _one_way_lib(path):
    """The library whose one-state entry points are timed: this build's, or another build's."""
    from idfcodec import _lib
    if not path:
        return _lib.lib()
    lib = ctypes.CDLL(path)
    for name in ("idf_rans_encode_streams", "idf_rans_decode_streams",
                 "idf_rans_encode_workspace_bytes", "idf_rans_decode_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def kernel_level(one, reps: int) -> dict:
    from idfcodec import _lib, configs, synthetic
    from idfcodec._lib import check, lib, ptr
    B = 256
    model = synthetic.build_model(configs.get("imagenet64")).cuda()
    codec, eng = model.codec(), model.engine()
    codec.encode(synthetic.images(B, seed=5).cuda())
    ws = eng.workspace(B)
    torch.cuda.synchronize()
    s = _lib.stream_ptr(torch.device("cuda"))
    res = {}
    for l in range(eng.nsplit):
        base, nsym, rel = codec.coder.level_streams(B, l)
        lat, mean, scale = (ws[k][base:base + nsym].clone() for k in ("lat", "mean", "scale"))
        wbytes = lib().idf_rans_encode_workspace_bytes(nsym)
        wsp = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        dws = torch.empty(256, dtype=torch.uint8, device="cuda")
        init = torch.full((B,), L, dtype=torch.int64, device="cuda")
        st = {w: (torch.empty(B * w, dtype=torch.int64, device="cuda"),       # states
                  torch.empty(nsym, dtype=torch.int32, device="cuda"),        # words at sym offsets
                  torch.empty(B, dtype=torch.int64, device="cuda"),           # counts
                  torch.empty(B, dtype=torch.int32, device="cuda"),           # status
                  torch.empty(B * w, dtype=torch.int64, device="cuda"),       # decode's final states
                  torch.empty(nsym, dtype=torch.float32, device="cuda"))      # decode's symbols
              for w in WAYS}

        def enc(w):
            fs, words, nw, status, _, _ = st[w]
            if w == 1:
                check(one.idf_rans_encode_streams(s, B, nsym, ptr(rel), ptr(lat), ptr(mean),
                                                  ptr(scale), ptr(init), ptr(fs), ptr(words),
                                                  ptr(nw), ptr(status), ptr(wsp), wbytes), "enc")
            else:
                check(lib().idf_rans_encode_streams_ways(s, w, B, nsym, ptr(rel), ptr(lat),
                                                         ptr(mean), ptr(scale), ptr(fs),
                                                         ptr(words), ptr(nw), ptr(status),
                                                         ptr(wsp), wbytes), "enc ways")

        def dec(w):
            fs, words, nw, status, dfs, out = st[w]
            if w == 1:
                check(one.idf_rans_decode_streams(s, B, nsym, ptr(rel), ptr(rel), ptr(nw),
                                                  ptr(words), ptr(mean), ptr(scale), ptr(fs),
                                                  ptr(dfs), ptr(out), ptr(status), ptr(dws), 256),
                      "dec")
            else:
                check(lib().idf_rans_decode_streams_ways(s, w, B, nsym, ptr(rel), ptr(rel),
                                                         ptr(nw), ptr(words), ptr(mean),
                                                         ptr(scale), ptr(fs), ptr(dfs), ptr(out),
                                                         ptr(status)), "dec ways")

        t = {(k, w): [] for k in ("enc", "dec") for w in WAYS}
        for it in range(3 + reps):
            for kind, fn in (("enc", enc), ("dec", dec)):
                for w in WAYS:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(w)
                    b.record()
                    torch.cuda.synchronize()
                    if it >= 3:
                        t[(kind, w)].append(a.elapsed_time(b))
        n_per = nsym // B
        lev = {"streams": B, "symbols_per_stream": n_per}
        for w in WAYS:
            fs, words, nw, status, dfs, out = st[w]
            exact = bool(torch.equal(out, lat)) and bool((dfs == L).all()) and not bool(
                status.any())
            e, d = statistics.median(t[("enc", w)]), statistics.median(t[("dec", w)])
            lev[f"ways{w}"] = {
                "encode_ms": round(e, 4), "decode_ms": round(d, 4),
                "encode_ms_min_max": [round(min(t[("enc", w)]), 4), round(max(t[("enc", w)]), 4)],
                "decode_ms_min_max": [round(min(t[("dec", w)]), 4), round(max(t[("dec", w)]), 4)],
                # the chain: time per symbol of one stream, and per step of `ways` symbols
                "decode_ns_per_symbol": round(d * 1e6 / n_per, 2),
                "decode_ns_per_step": round(d * 1e6 / (n_per / w), 1),
                "encode_ns_per_symbol": round(e * 1e6 / n_per, 2),
                "words": int(nw.sum()), "exact": exact}
        for w in WAYS[1:]:
            lev[f"ways{w}"]["decode_speedup_vs_ways1"] = round(
                lev["ways1"]["decode_ms"] / lev[f"ways{w}"]["decode_ms"], 3)
            lev[f"ways{w}"]["encode_speedup_vs_ways1"] = round(
                lev["ways1"]["encode_ms"] / lev[f"ways{w}"]["encode_ms"], 3)
        res[f"level{l}"] = lev
    return res


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _ms(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3),
            "ms_max": round(max(v), 3)}


def end_to_end(steps: int, warmup: int) -> dict:
    from idfcodec import configs, synthetic
    model = synthetic.build_model(configs.get("imagenet64")).cuda()
    ways = (1, 8, 64)
    res = {}
    for B in (256, 4):
        img = synthetic.images(B, seed=6).cuda()
        t = {(k, w): [] for k in ("enc", "dec") for w in ways}
        exact = {w: 0 for w in ways}
        bits = {}
        for step in range(warmup + steps):
            for w in ways:
                bs, te = _timed(lambda: model.encode(img, ways=w))
                (out, _), td = _timed(lambda: model.decode(bs, verify=False))
                if step < warmup:
                    continue
                t[("enc", w)].append(te)
                t[("dec", w)].append(td)
                exact[w] += int(torch.equal(out, img))
                bits[w] = (bs.bpd(), 64 * bs.states.numel() / bs.n_subpixels())
        res[f"B{B}"] = {f"ways{w}": {"encode": _ms(t[("enc", w)]), "decode": _ms(t[("dec", w)]),
                                     "round_trip_exact_steps": f"{exact[w]}/{steps}",
                                     "bpd": round(bits[w][0], 5),
                                     "state_bits_per_subpixel": round(bits[w][1], 5)}
                        for w in ways}
    # a crop over 4 tiles of a 256x256 image (16 tiles)
    big = [synthetic.images(1, 3, 256, 256, seed=7)[0].cuda()]
    tbs = {w: model.tiled(ways=w).encode(big) for w in ways}
    tc = model.tiled()
    t = {w: [] for w in ways}
    exact = {w: 0 for w in ways}
    for step in range(warmup + steps):
        for w in ways:
            (crop, info), ms = _timed(lambda: tc.decode_region(tbs[w], 0, 96, 96, 64, 64))
            if step < warmup:
                continue
            t[w].append(ms)
            exact[w] += int(bool(info["ok"]) and info["tiles"] == 4
                            and torch.equal(crop, big[0][:, 96:160, 96:160]))
    res["region_4_tiles"] = {f"ways{w}": dict(_ms(t[w]), exact_steps=f"{exact[w]}/{steps}",
                                              state_bits_per_subpixel=round(
                                                  tbs[w].state_bits_per_subpixel(), 5))
                             for w in ways}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=None,
                    help="another build of libidfcodec.so for the one-state (ways = 1) kernels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    res = {"metric": "rANS interleaved ways vs one state per stream (imagenet64, seeded weights)",
           "one_way_lib": a.lib or "this build", "reps": a.reps,
           "kernels": kernel_level(_one_way_lib(a.lib), a.reps)}
    if not a.skip_e2e:
        res["end_to_end"] = dict(end_to_end(a.steps, a.warmup), steps=a.steps, warmup=a.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
