"""Lossless codec of TwoLevelFlows (flows.py:184-274; configs/config_twolevel.yaml).

encode: uint8 images at the source size -> idf_twolevel_split (replication pad, dequant,
        integer average pool + round to the rough image, residual against the replicated
        rough image, Patching of the residual; one kernel, straight into the pixel-major
        inputs of the two FlowEngines) -> the rough IDFlows' rANS streams (one per image and
        level) -> the fine IDFlows' streams over the 8x8-style patches, `group` patches per
        stream (codec.Bitstream.group) -> TwoLevelBitstream (container IDF2).
decode: the rough streams and the fine streams through their engines, then
        idf_twolevel_merge: uint8 at the source size (the pad is never written).

The pool is defined in integers on the 1/256 grid (split_host is the numpy restatement the
kernels are tested against): k' = k + [k >= 128], a window of n padded pixels sums to S,
rough * 256 = round_half_even(S / n).  For power-of-two windows this is the reference's
round(AdaptiveAvgPool2d(x)) bit for bit; for other windows it is the definition (the decoder
reads the rough image from its own stream, so nothing depends on matching torch there).

Why groups: a fine patch is a batch entry of C*fh*fw symbols (192 at 3x8x8), and every rANS
stream ends in 64 bits of state -- 0.33 bits per sub-pixel if each patch had its own stream.
The latents are level-major, entry-minor, so `group` consecutive patches are one contiguous
symbol run and share a stream with no new kernel.  A group divides the patches of one image:
no stream spans two images, and an image codes identically alone or in a batch.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .codec import Bitstream, streams_ok

MAGIC = b"IDF2"
VERSION = 1
_HDR = "<4sHH" + "I" * 11 + "QQ"


class Geometry(NamedTuple):
    C: int
    Hs: int     # source (unpadded) size
    Ws: int
    Hp: int     # replication-padded size
    Wp: int
    rh: int     # rough image
    rw: int
    fh: int     # fine patch
    fw: int

    @property
    def patches(self) -> int:
        """fine patches per image"""
        return (self.Hp // self.fh) * (self.Wp // self.fw)

    @property
    def window(self) -> tuple:
        return (self.Hp // self.rh, self.Wp // self.rw)

    @classmethod
    def of(cls, model) -> "Geometry":
        return cls(model.C, model.H - model.pad[0], model.W - model.pad[1], model.H, model.W,
                   model.rough.H, model.rough.W, model.fine.H, model.fine.W)


# ------------------------------------------------------------------ host restatement
def round_half_even_div(s: np.ndarray, n: int) -> np.ndarray:
    """round_half_even(s / n) in integers (n > 0, s of either sign)."""
    s = np.asarray(s, np.int64)
    q = s // n
    r = s - q * n
    return q + ((2 * r > n) | ((2 * r == n) & (q % 2 == 1)))


def split_host(u8: np.ndarray, pad, rough_hw, fine_hw):
    """numpy restatement of idf_twolevel_split for uint8 NCHW images: returns (rough image
    [B,C,rh,rw], fine patches [B*n,C,fh,fw] in Patching order, padded image), all float32 on
    the 1/256 grid."""
    k = np.asarray(u8).astype(np.int64)
    k = k + (k >= 128)
    kp = np.pad(k, ((0, 0), (0, 0), (0, int(pad[0])), (0, int(pad[1]))), mode="edge")
    B, C, Hp, Wp = kp.shape
    (rh, rw), (fh, fw) = rough_hw, fine_hw
    if Hp % rh or Wp % rw or Hp % fh or Wp % fw:
        raise ValueError(f"padded size {(Hp, Wp)} is no multiple of {rough_hw} and {fine_hw}")
    wh, ww = Hp // rh, Wp // rw
    q = round_half_even_div(kp.reshape(B, C, rh, wh, rw, ww).sum(axis=(3, 5)), wh * ww)
    res = kp - np.repeat(np.repeat(q, wh, axis=2), ww, axis=3)
    px = res.reshape(B, C, Hp // fh, fh, Wp // fw, fw).transpose(0, 2, 4, 1, 3, 5)
    px = px.reshape(-1, C, fh, fw)
    f = lambda a: (a.astype(np.float64) / 256).astype(np.float32)  # noqa: E731
    return f(q), f(px), f(kp)


def merge_host(rx: np.ndarray, px: np.ndarray, pad, padded_hw) -> np.ndarray:
    """numpy restatement of idf_twolevel_merge's f32 variant: replicate(rx) + unpatch(px),
    cropped to the source size."""
    rx, px = np.asarray(rx, np.float32), np.asarray(px, np.float32)
    Hp, Wp = padded_hw
    B, C, rh, rw = rx.shape
    fh, fw = px.shape[2:]
    up = np.repeat(np.repeat(rx, Hp // rh, axis=2), Wp // rw, axis=3)
    fx = px.reshape(B, Hp // fh, Wp // fw, C, fh, fw).transpose(0, 3, 1, 4, 2, 5)
    x = up + fx.reshape(B, C, Hp, Wp)
    return x[:, :, :Hp - int(pad[0]), :Wp - int(pad[1])]


# ------------------------------------------------------------------ device calls
def device_split(g: Geometry, src: torch.Tensor, rough_pm: torch.Tensor, fine_pm: torch.Tensor,
                 bad: torch.Tensor | None = None):
    """src: uint8 or float32 NCHW [B, C, Hs, Ws] (contiguous, device) -> the pixel-major
    (ld 4) rough and fine buffers.  bad: int32[1], the off-grid count of f32 input."""
    B = src.shape[0]
    if tuple(src.shape[1:]) != (g.C, g.Hs, g.Ws):
        raise ValueError(f"image shape {tuple(src.shape[1:])}: the model takes "
                         f"{(g.C, g.Hs, g.Ws)}")
    if rough_pm.numel() < B * g.rh * g.rw * 4 or fine_pm.numel() < B * g.Hp * g.Wp * 4:
        raise ValueError("split output buffers are too small")
    u8 = src.dtype == torch.uint8
    if not u8 and (src.dtype != torch.float32 or bad is None):
        raise TypeError("idf_twolevel_split takes uint8, or float32 with an off-grid counter")
    check(lib().idf_twolevel_split(
        _lib.stream_ptr(src.device), B, g.C, g.Hs, g.Ws, g.Hp, g.Wp, g.rh, g.rw, g.fh, g.fw,
        ptr(src) if u8 else None, None if u8 else ptr(src), ptr(rough_pm), 4, ptr(fine_pm), 4,
        ptr(bad)), "twolevel split")


def device_merge(g: Geometry, B: int, rough_pm: torch.Tensor, fine_pm: torch.Tensor,
                 out: torch.Tensor, bad: torch.Tensor | None = None):
    """The pixel-major rough and fine buffers -> out, uint8 or float32 NCHW [B, C, Hs, Ws]."""
    if tuple(out.shape) != (B, g.C, g.Hs, g.Ws) or not out.is_contiguous():
        raise ValueError("merge output must be contiguous [B, C, Hs, Ws]")
    if rough_pm.numel() < B * g.rh * g.rw * 4 or fine_pm.numel() < B * g.Hp * g.Wp * 4:
        raise ValueError("merge input buffers are too small")
    u8 = out.dtype == torch.uint8
    if not u8 and out.dtype != torch.float32:
        raise TypeError("idf_twolevel_merge writes uint8 or float32")
    if u8 and bad is None:
        raise TypeError("the uint8 merge needs an off-grid counter")
    check(lib().idf_twolevel_merge(
        _lib.stream_ptr(out.device), B, g.C, g.Hs, g.Ws, g.Hp, g.Wp, g.rh, g.rw, g.fh, g.fw,
        ptr(rough_pm), 4, ptr(fine_pm), 4, ptr(out) if u8 else None, None if u8 else ptr(out),
        ptr(bad)), "twolevel merge")


def split_nchw(g: Geometry, x: torch.Tensor):
    """uint8 NCHW images, or float ones on the grid -> (rough NCHW, fine patches NCHW,
    off-grid count of the float input)."""
    _lib.require_device(x, "TwoLevelFlows input")
    x = x.contiguous() if x.dtype == torch.uint8 else x.float().contiguous()
    B, dev = x.shape[0], x.device
    s = _lib.stream_ptr(dev)
    rpm = torch.empty(B * g.rh * g.rw * 4, dtype=torch.float32, device=dev)
    fpm = torch.empty(B * g.Hp * g.Wp * 4, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    device_split(g, x, rpm, fpm, bad)
    rx = torch.empty((B, g.C, g.rh, g.rw), dtype=torch.float32, device=dev)
    px = torch.empty((B * g.patches, g.C, g.fh, g.fw), dtype=torch.float32, device=dev)
    check(lib().idf_pm_to_nchw(s, B, g.C, g.rh, g.rw, ptr(rpm), 4, ptr(rx)), "pm->nchw")
    check(lib().idf_pm_to_nchw(s, B * g.patches, g.C, g.fh, g.fw, ptr(fpm), 4, ptr(px)),
          "pm->nchw")
    return rx, px, bad


def merge_nchw(g: Geometry, rx: torch.Tensor, px: torch.Tensor) -> torch.Tensor:
    """(rough NCHW, fine patches NCHW) -> float32 NCHW images at the source size."""
    _lib.require_device(rx, "rough image")
    _lib.require_device(px, "fine patches")
    rx, px = rx.float().contiguous(), px.float().contiguous()
    B, dev = rx.shape[0], rx.device
    if tuple(rx.shape[1:]) != (g.C, g.rh, g.rw) or tuple(px.shape) != (B * g.patches, g.C, g.fh,
                                                                       g.fw):
        raise ValueError("rough / fine shapes do not match the model's geometry")
    s = _lib.stream_ptr(dev)
    rpm = torch.empty(B * g.rh * g.rw * 4, dtype=torch.float32, device=dev)
    fpm = torch.empty(B * g.Hp * g.Wp * 4, dtype=torch.float32, device=dev)
    check(lib().idf_nchw_to_pm(s, B, g.C, g.rh, g.rw, ptr(rx), ptr(rpm), 4), "nchw->pm")
    check(lib().idf_nchw_to_pm(s, B * g.patches, g.C, g.fh, g.fw, ptr(px), ptr(fpm), 4),
          "nchw->pm")
    out = torch.empty((B, g.C, g.Hs, g.Ws), dtype=torch.float32, device=dev)
    device_merge(g, B, rpm, fpm, out)
    return out


# ------------------------------------------------------------------ container
@dataclass
class TwoLevelBitstream:
    rough: Bitstream            # one stream per (image, level)
    fine: Bitstream             # `group` patches per stream (fine.group)
    n_images: int
    image_shape: tuple          # (C, H_src, W_src)
    pad: tuple                  # (bottom, right) replication pad
    rough_hw: tuple
    fine_hw: tuple

    @property
    def group(self) -> int:
        return self.fine.group

    def bits(self) -> int:
        """both parts, the reference's accounting (64 bits per stream + 32 per word)"""
        return self.rough.bits() + self.fine.bits()

    def bpd(self) -> float:
        """bits per sub-pixel of the unpadded images (the denominator of flows.py:241)"""
        C, H, W = self.image_shape
        n = self.n_images * C * H * W
        return self.bits() / n if n else float("nan")

    def to_bytes(self) -> bytes:
        C, H, W = self.image_shape
        rb, fb = self.rough.to_bytes(), self.fine.to_bytes(grouped=True)
        hdr = struct.pack(_HDR, MAGIC, VERSION, 0, self.n_images, C, H, W, self.pad[0],
                          self.pad[1], self.rough_hw[0], self.rough_hw[1], self.fine_hw[0],
                          self.fine_hw[1], self.group, len(rb), len(fb))
        return hdr + rb + fb

    @classmethod
    def from_bytes(cls, buf: bytes, device=None) -> "TwoLevelBitstream":
        n_hdr = struct.calcsize(_HDR)
        if len(buf) < n_hdr:
            raise ValueError("truncated two-level bitstream (header)")
        (magic, ver, flags, n, C, H, W, ph, pw, rh, rw, fh, fw, group, lr,
         lf) = struct.unpack_from(_HDR, buf, 0)
        if magic != MAGIC:
            raise ValueError("not an IDF two-level bitstream")
        if ver != VERSION:
            raise ValueError(f"unknown two-level bitstream version {ver}")
        if flags:
            raise ValueError(f"unknown two-level bitstream flags {flags:#x}")
        if len(buf) != n_hdr + lr + lf:
            raise ValueError(f"two-level bitstream holds {len(buf) - n_hdr} payload bytes, its "
                             f"header names {lr} + {lf}")
        if group < 1 or min(rh, rw, fh, fw) < 1:
            raise ValueError("two-level bitstream header holds a zero size")
        try:
            rough = Bitstream.from_bytes(buf[n_hdr:n_hdr + lr], device)
            fine = Bitstream.from_bytes(buf[n_hdr + lr:n_hdr + lr + lf], device, group=group)
        except struct.error as e:
            raise ValueError(f"truncated two-level bitstream ({e})") from None
        return cls(rough, fine, n, (C, H, W), (ph, pw), (rh, rw), (fh, fw))


# ------------------------------------------------------------------ codec
class TwoLevelCodec:
    """uint8 images [B, C, H_src, W_src] <-> TwoLevelBitstream with a flows.TwoLevelFlows."""

    def __init__(self, model):
        self.model = model
        self.geometry = Geometry.of(model)
        self._bufs = {}

    def _parts(self):
        return self.model.rough.codec(), self.model.fine.codec()

    def _buf(self, name: str, n: int, dev) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or t.numel() < n or t.device != dev:
            t = self._bufs[name] = torch.empty(n, dtype=torch.float32, device=dev)
        return t

    def default_group(self) -> int:
        """one row of the patch grid"""
        return self.geometry.Wp // self.geometry.fw

    @torch.no_grad()
    def encode(self, img_u8: torch.Tensor, group: int | None = None) -> TwoLevelBitstream:
        _lib.require_device(img_u8, "image batch")
        if img_u8.dtype != torch.uint8:
            raise TypeError("TwoLevelCodec.encode expects uint8 images")
        g = self.geometry
        if img_u8.dim() != 4 or tuple(img_u8.shape[1:]) != (g.C, g.Hs, g.Ws):
            raise ValueError(f"image shape {tuple(img_u8.shape[1:])}: the model takes "
                             f"{(g.C, g.Hs, g.Ws)}")
        n = g.patches
        group = self.default_group() if group is None else int(group)
        if group < 1 or n % group:
            raise ValueError(f"stream group {group} does not divide the {n} patches of an image")
        img_u8 = img_u8.contiguous()
        B = img_u8.shape[0]
        rc, fc = self._parts()
        reng, feng = rc.engine, fc.engine

        def fill():  # one pass: the source bytes into both engines' input buffers
            rws, fws = reng.workspace(B, 0), feng.workspace(B * n, 0)
            device_split(g, img_u8, rws["img"], fws["img"])
            return rws, fws

        rws, fws = fill()
        # each part's load: the split has filled its workspace (a flow only reads ws['img'], so
        # the range guard's exact-f32 recompute finds it intact); run it again only if the
        # engine has dropped that workspace set meanwhile
        rough = rc._encode_guarded(lambda: rws if reng.workspace(B, 0) is rws else fill()[0],
                                   B, None, True)
        px4 = g.fh * g.fw * 4
        fimg = fws["img"]

        def lane_src(i, p0, m):  # an encode lane's patches, read in place
            return fimg[p0 * px4:(p0 + m) * px4]

        fine = fc._encode_guarded(lambda: fws if feng.workspace(B * n, 0) is fws else fill()[1],
                                  B * n, None, True, lane_src=lane_src, group=group)
        return TwoLevelBitstream(rough, fine, B, (g.C, g.Hs, g.Ws),
                                 (g.Hp - g.Hs, g.Wp - g.Ws), (g.rh, g.rw), (g.fh, g.fw))

    def check_bitstream(self, tbs: TwoLevelBitstream):
        if tbs.rough.ways != 1 or tbs.fine.ways != 1:
            raise ValueError(f"two-level bitstream with interleaved streams (ways "
                             f"{tbs.rough.ways}, {tbs.fine.ways}): the two-level codec codes "
                             "ways = 1 only")
        g = self.geometry
        want = ((g.C, g.Hs, g.Ws), (g.Hp - g.Hs, g.Wp - g.Ws), (g.rh, g.rw), (g.fh, g.fw))
        have = (tuple(tbs.image_shape), tuple(tbs.pad), tuple(tbs.rough_hw), tuple(tbs.fine_hw))
        if have != want:
            raise ValueError(f"two-level bitstream geometry {have} does not match the model's "
                             f"{want}")
        B, n = tbs.n_images, g.patches
        if tbs.rough.n_images != B or tbs.fine.n_images != B * n:
            raise ValueError(f"two-level bitstream of {B} images holds {tbs.rough.n_images} "
                             f"rough images and {tbs.fine.n_images} patches ({n} per image)")
        if tbs.rough.group != 1 or tbs.fine.group < 1 or n % tbs.fine.group:
            raise ValueError(f"stream groups ({tbs.rough.group}, {tbs.fine.group}) do not fit "
                             f"{n} patches per image")

    @torch.no_grad()
    def decode(self, tbs: TwoLevelBitstream, verify: bool = True):
        """-> (uint8 images at the source size, info); info['ok'] combines both parts' final
        states and stream status with the merge's off-grid count."""
        self.check_bitstream(tbs)
        g = self.geometry
        rc, fc = self._parts()
        dev = rc.engine.device
        B = tbs.n_images
        rpm = self._buf("rough", B * g.rh * g.rw * 4, dev)
        fpm = self._buf("fine", B * g.Hp * g.Wp * 4, dev)
        rinfo = rc.decode_into(tbs.rough, rpm)
        finfo = fc.decode_into(tbs.fine, fpm)
        img = torch.empty((B, g.C, g.Hs, g.Ws), dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        device_merge(g, B, rpm, fpm, img, bad)
        info = {"rough": rinfo, "fine": finfo, "off_grid": bad}
        if verify:
            info["ok"] = int(bad.item()) == 0 and all(
                streams_ok(part["final_states"], part["status"]) for part in (rinfo, finfo))
        return img, info
