"""Flow models (mirror of flows.py:19-361): IDFlows and ConditionalFlows with the
reference's constructor kwargs, registry names, submodule tree and parameter
creation order -- the same YAML configs build them, the same state_dicts load,
and `random.seed(0); torch.manual_seed(0)` gives the same initial weights.

forward / generated_from_latents / log_likelihood keep the reference
signatures; the whole pass runs in idfcodec.FlowEngine (HIP kernels, pixel-major
activations, one feature buffer per DenseBlock).  encode / decode -- empty
placeholders in the reference (flows.py:177-181) -- are the real lossless codec
here: uint8 images <-> rANS bitstreams (idfcodec.codec).

TwoLevelFlows (flows.py:184-274; configs/config_twolevel.yaml) codes an image
larger than a flow's input with two IDFlows and no VQ-VAE: a "rough" average-
pooled image and the residual against it as small patches.  The pad / pool /
residual / patch plumbing runs as idf_twolevel_split / idf_twolevel_merge, and
encode / decode are idfcodec.twolevel.TwoLevelCodec (grouped rANS streams for
the patches).  Inference only: forward(train=True) raises.
"""
import math
from copy import deepcopy

import torch
from torch import nn

import moduleregister
from couplelib import NNCouple  # noqa: F401  (registers AdditiveCouple)
from distlib import NNDistribution
from extenddim import ExtendDim, NNExtendDim, Patching
from invertible import InvertibleModuleList, Permute
from priorlib import NNPrior
from roundlib import NNRound, Round  # noqa: F401
from idfcodec._lib import require_device


class NNFlows(moduleregister.Register):
    def __init__(self):
        super().__init__()


@NNFlows.register
class IDFlows(nn.Module):
    def __init__(self, nflows=8, nbits=8, nsplit=3, H=64, W=64, C=3, couple=None, extenddim=None,
                 prior=None, distribution=None, round=None, batch_squeeze=0):
        super().__init__()
        self.nflows = nflows
        self.nbits = nbits
        self.nsplit = nsplit
        self.blocks = nn.ModuleList()
        self.latents_shape = []
        self.C, self.H, self.W = C, H, W
        couple, extenddim, prior = dict(couple), dict(extenddim), dict(prior)
        distribution, round = dict(distribution), dict(round)
        self.couple_type = NNCouple.get(couple.pop("name"))
        self.prior_type = NNPrior.get(prior.pop("name"))
        self.extenddim_type = NNExtendDim.get(extenddim.pop("name"))
        self.dist_type = NNDistribution.get(distribution.pop("name"))
        self.round_type = NNRound.get(round.pop("name"))
        self.batch_squeeze = batch_squeeze
        channel = C * batch_squeeze if batch_squeeze else C
        h, w = H, W
        s = extenddim.get("scale")
        for split_level in range(nsplit):
            channel *= s * s
            h //= s
            w //= s
            flow_module = InvertibleModuleList()
            for _ in range(nflows):
                flow_module.append(Permute(dim=channel))
                flow_module.append(self.couple_type(channel=channel, **deepcopy(couple)))
            flow_module.append(Permute(dim=channel))
            if split_level < nsplit - 1:
                prior_nn = self.prior_type(channel // 2, channel - channel // 2, **deepcopy(prior))
                self.latents_shape.append((channel // 2, h, w))
                channel -= channel // 2
            else:
                prior_nn = self.prior_type(channel, 0, **deepcopy(prior))
                self.latents_shape.append((channel, h, w))
            self.blocks.append(nn.ModuleDict(dict(
                extend=self.extenddim_type(**deepcopy(extenddim)), flows=flow_module, prior=prior_nn)))
        self.dist = self.dist_type(**distribution)
        self.round = self.round_type(**round)
        self._engine = None
        self._engine_key = None

    # ------------------------------------------------------------ engine
    def engine(self):
        """The device engine for the current parameters (rebuilt when they change)."""
        from idfcodec.engine import FlowEngine
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("idfcodec: move the model to the HIP device (.cuda()) first; "
                               "there is no CPU path")
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + (
            getattr(self, "idf_precision", "f32"),)
        if self._engine is None or self._engine_key != key:
            self._engine = FlowEngine(self, dev)
            self._engine_key = key
        return self._engine

    def codec(self):
        from idfcodec.codec import ImageCodec
        eng = self.engine()
        if getattr(self, "_codec", None) is None or self._codec.engine is not eng:
            self._codec = ImageCodec(eng)
        return self._codec

    def tiled(self, max_batch=None, ways=1):
        """The codec of images of any size as tiles of this model's input
        (idfcodec.tiled.TiledCodec; max_batch: entries per engine batch, default 256; ways:
        interleaved rANS states per stream), cached and rebuilt when the engine is."""
        from idfcodec.tiled import TiledCodec
        eng = self.engine()
        t = getattr(self, "_tiled", None)
        if t is None or self._tiled_engine is not eng or ways != t.ways or (
                max_batch is not None and int(max_batch) != t.max_batch):
            t = TiledCodec(self, **({} if max_batch is None else {"max_batch": max_batch}),
                           ways=ways)
            self._tiled, self._tiled_engine = t, eng
        return t

    def tiled_safe(self, max_batch=None, ways=1, predict=False, predict_ways=1, seal=False):
        """tiled() with the raw-tile escape (idfcodec.safe.SafeTiledCodec): every tile is coded
        by the flow or, where that would lose data or cost more than asked, stored as its bytes.
        predict=True: the escaped tiles are coded by a MED predictor and rANS where that is
        smaller (idfcodec.predict.PredictiveTileCodec, IDFP files); predict="colour": that coder
        also tries planes 0 and 2 as differences to plane 1 and keeps the smaller coding of each
        tile (C >= 3, IDFQ files).  predict_ways: 8, 16, 32 or 64 interleaved states per
        predictive stream, its symbols along a pixel wavefront, so that a wave decodes that many
        pixels a step (`ways` stays the flow streams' own); it needs predict.  Cached as tiled()
        is, the three kinds apart.  seal=True: the idfcodec.integrity.SealedCodec around exactly
        the codec the same call returns without it (IDFC files around IDFS, IDFP or IDFQ), cached
        on the codec it wraps, each kind apart; without predict that is tiled_sealed()."""
        if isinstance(predict, str) and predict != "colour":
            raise ValueError(f"predict is False, True or 'colour', not {predict!r}")
        if predict:
            colour = isinstance(predict, str)
            t = self._tiled_predict(max_batch, ways, predict_ways, colour=colour)
            if not seal:
                return t
            from idfcodec.integrity import SealedCodec
            slot = "_tiled_pred_colour_sealed" if colour else "_tiled_pred_sealed"
            s = getattr(self, slot, None)
            if s is None or s.codec is not t:
                s = SealedCodec(t)
                setattr(self, slot, s)
            return s
        if predict_ways != 1:
            raise ValueError(f"predict_ways {predict_ways!r} needs predict=True or 'colour'")
        if seal:
            return self.tiled_sealed(max_batch, ways, safe=True)
        from idfcodec.safe import SafeTiledCodec
        eng = self.engine()
        t = getattr(self, "_tiled_safe", None)
        if t is None or self._tiled_safe_engine is not eng or ways != t.ways or (
                max_batch is not None and int(max_batch) != t.max_batch):
            t = SafeTiledCodec(self, **({} if max_batch is None else {"max_batch": max_batch}),
                               ways=ways)
            self._tiled_safe, self._tiled_safe_engine = t, eng
        return t

    def _tiled_predict(self, max_batch, ways, predict_ways=1, colour=False):
        from idfcodec.predict import PredictiveTileCodec
        eng = self.engine()
        slot = "_tiled_pred_colour" if colour else "_tiled_pred"
        t = getattr(self, slot, None)
        if t is None or getattr(self, slot + "_engine") is not eng or ways != t.ways or (
                predict_ways != t.predict_ways) or (
                max_batch is not None and int(max_batch) != t.max_batch):
            t = PredictiveTileCodec(self, **({} if max_batch is None else
                                             {"max_batch": max_batch}), ways=ways, colour=colour,
                                    predict_ways=predict_ways)
            setattr(self, slot, t)
            setattr(self, slot + "_engine", eng)
        return t

    def tiled_sealed(self, max_batch=None, ways=1, safe=True):
        """tiled_safe() (safe=False: tiled()) writing sealed files
        (idfcodec.integrity.SealedCodec): a CRC-32 per tile, computed on the device at encode and
        at decode, and this model's fingerprint, so a damaged tile is named and a file written by
        other weights is refused.  Cached on the codec it wraps."""
        from idfcodec.integrity import SealedCodec
        inner = (self.tiled_safe if safe else self.tiled)(max_batch, ways)
        s = getattr(self, "_tiled_sealed", None)
        if s is None or s.codec is not inner:
            s = self._tiled_sealed = SealedCodec(inner)
        return s

    def tiled_planes(self, channels, base=None, predict_ways=1, max_batch=None):
        """The codec of images of `channels` channels, whatever this model's C
        (idfcodec.planes.PlaneSetCodec, IDFM files): grey, grey + alpha, RGBA and more.  With
        channels >= C the first C channels go to `base` -- tiled(), tiled_safe() or
        tiled_safe(predict=...) of this model; default tiled_safe(max_batch, predict=True) -- and
        the others are extra planes; with fewer, all are extra planes and no flow runs.  An extra
        plane of a tile is stored as one byte where it is constant, else coded by the predictive
        coder at predict_ways states or stored as its bytes, whichever is smaller.  A sealed base
        is refused: the seal would not cover the extra planes."""
        from idfcodec.planes import PlaneSetCodec
        return PlaneSetCodec(self, channels, base=base, predict_ways=predict_ways,
                             max_batch=max_batch)

    def _check_batch_squeeze(self):
        if self.batch_squeeze:
            raise NotImplementedError("batch_squeeze (flows.py:92-95) is not used by the north-star "
                                      "configs and is not implemented")

    # ------------------------------------------------------------ reference API
    def forward(self, x, logv):
        """flows.py:87-116 -> (latents, means, logscales, logv), NCHW per level."""
        require_device(x, "IDFlows input")
        self._check_batch_squeeze()
        eng = self.engine()
        B = x.shape[0]
        ws = eng.load_nchw(x)
        eng.forward_pm(B)
        lat = [t.clone() for t in eng.level_views(ws, B, "lat")]
        mean = [t.clone() for t in eng.level_views(ws, B, "mean")]
        logs = [t.clone() for t in eng.level_views(ws, B, "logscale")]
        return lat, mean, logs, logv

    def generated_from_latents(self, latents):
        """flows.py:139-152: invert the flows given every level's latent."""
        self._check_batch_squeeze()
        eng = self.engine()
        B = latents[0].shape[0]

        def put(l, ws):
            eng.level_views(ws, B, "lat")[l].copy_(latents[l])

        ws = eng.inverse_pm(B, put, priors=False)
        return eng.image_nchw(ws, B)

    def generated_from_noise(self, latents):
        """flows.py:118-137 (sampling/visualisation; not on the coding path)."""
        eng = self.engine()
        B = latents[0].shape[0]

        def put(l, ws):
            m = eng.level_views(ws, B, "mean")[l]
            ls = eng.level_views(ws, B, "logscale")[l]
            z = latents[l].to(m.device) * torch.exp(ls) + m
            eng.level_views(ws, B, "lat")[l].copy_(torch.round(z * 256) / 256)

        ws = eng.inverse_pm(B, put, priors=True)
        return eng.image_nchw(ws, B)

    def log_likelihood(self, latents, means, logscales):
        """flows.py:154-169: per image, the log-probabilities of every level summed (per-level
        means in log_Ps), divided by H*W*C -- one idf_log_prob launch per level, the
        per-(level, image) sums reduced on the device in a fixed order (f64)."""
        from distlib import DLogistic, dlogistic_log_prob
        if not isinstance(self.dist, DLogistic):
            raise NotImplementedError("log_likelihood supports the DLogistic prior only")
        B = latents[0].shape[0]
        dev = latents[0].device
        require_device(latents[0], "latents")
        total = torch.zeros(B, dtype=torch.float64, device=dev)
        log_Ps = []
        for z, m, ls in zip(latents, means, logscales):
            z, m, ls = torch.broadcast_tensors(z.to(dev), m.to(dev), ls.to(dev))
            sums = dlogistic_log_prob(z, m, ls, self.nbits, groups=B)
            log_Ps.append((sums / (z.numel() // B)).float())
            total += sums
        return (total / (self.H * self.W * self.C)).float(), log_Ps

    def inverse(self):
        for block in self.blocks:
            block["extend"].inverse()
            for flow in block["flows"]:
                flow.inverse()

    # ------------------------------------------------------------ the codec
    def encode(self, x, ways=1):
        """uint8 images [B, C, H, W] (device) -> idfcodec.Bitstream.  ways: interleaved rANS
        states per stream (1, 8, 16, 32 or 64: a ways times shorter serial chain for
        64 (ways - 1) more bits per stream); decode follows the bitstream."""
        return self.codec().encode(x, ways=ways)

    def decode(self, bitstream, verify=True):
        """Bitstream -> (uint8 images, info) -- exact inverse of encode()."""
        return self.codec().decode(bitstream, verify=verify)


@NNFlows.register
class TwoLevelFlows(nn.Module):
    """flows.py:184-274.  x -> replication pad -> rough = round(avgpool(x)) coded by `rough`,
    fine = x - upsample(rough) coded as fine.H x fine.W patches by `fine`.

    Supported geometry: the padded size is an integer multiple of the rough image and of the
    fine patch (ValueError otherwise).  At non-integer ratios the reference's adaptive up-pool
    averages neighbouring rough pixels, the residual leaves the 1/256 grid and the model cannot
    be coded losslessly.  At integer ratios the up-pool is plain replication, and the pool is
    computed in integers on the grid (idfcodec.twolevel): bit for bit the reference's
    round(AdaptiveAvgPool2d(x)) for power-of-two windows, ties included."""

    def __init__(self, H, W, C, pad, fine_flows, rough_flows, batchsize=256, nbits=8):
        super().__init__()
        self.H = H + pad[0]
        self.W = W + pad[1]
        self.C = C
        self.pad = pad
        # copies: the reference pops 'name' from the caller's dicts in place
        fine_flows, rough_flows = dict(fine_flows), dict(rough_flows)
        self.fine = NNFlows.get(fine_flows.pop("name"))(**fine_flows)
        self.rough = NNFlows.get(rough_flows.pop("name"))(**rough_flows)
        for what, m in (("rough image", self.rough), ("fine patch", self.fine)):
            if self.H % m.H or self.W % m.W:
                raise ValueError(f"TwoLevelFlows: the padded size {self.H}x{self.W} is not an "
                                 f"integer multiple of the {what} {m.H}x{m.W}; such a model has "
                                 "an off-grid residual and cannot be coded losslessly")
            if m.C != C or m.nsplit != 1:
                raise ValueError(f"TwoLevelFlows: the {what} flow must have C={C} and nsplit=1 "
                                 "(flows.py:188)")
        self.patching = Patching(self.H, self.W, self.fine.H, self.fine.W)
        self.latents_shape = [deepcopy(self.rough.latents_shape[0]),
                              deepcopy(self.fine.latents_shape[0])]
        self.latents_shape[1] = (self.latents_shape[1][0] * (self.H // self.fine.H)
                                 * (self.W // self.fine.W),
                                 self.latents_shape[1][1], self.latents_shape[1][2])
        self.batchsize = batchsize
        self.ratio = (self.H // self.fine.H, self.W // self.fine.W)
        self.round = Round(nbits=nbits)
        self._tl_codec = None

    def _geometry(self):
        from idfcodec.twolevel import Geometry
        return Geometry.of(self)

    def split(self, x):
        """x: float NCHW at the unpadded size, on the 1/256 grid -> (rough image rx, fine
        patches px in Patching order), flows.py:213-215 + :225 as one device kernel.  Raises if
        x is off the grid (the integer pool is defined on it)."""
        from idfcodec.twolevel import split_nchw
        rx, px, bad = split_nchw(self._geometry(), x)
        if int(bad.item()):
            raise ValueError(f"TwoLevelFlows input: {int(bad.item())} values off the 1/256 grid")
        return rx, px

    def forward(self, x, logv, train=True):
        """flows.py:209-245 -> (latents, means, logscales, bpd, bpd1, bpd2, logv) with
        latents = [rough latent, fine latents of every patch], bpd by the reference's formula
        (:241), bpd2 accumulated over chunks of `batchsize` patches.  There is no backward pass
        here: train=True (the reference's default, which calls loss.backward() inside) raises.

        One deliberate difference: reference line 242 concatenates `flatent` (the last chunk's
        one-element list) instead of `flatents`, so with more than one chunk it returns only
        the last chunk's fine latents; this returns all of them, in patch order."""
        if train:
            raise NotImplementedError("TwoLevelFlows.forward(train=True) runs loss.backward() in "
                                      "the reference; this package has no backward pass -- "
                                      "call forward(x, logv, train=False)")
        require_device(x, "TwoLevelFlows input")
        rx, px = self.split(x)
        rlatent, rmean, rlogscale, logv = self.rough.forward(rx, logv)
        logP, _ = self.rough.log_likelihood(rlatent, rmean, rlogscale)
        bpd1 = torch.mean(-logP, dim=0).item() / math.log(2)
        flatents, fmeans, flogscales = [], [], []
        nums, bs = px.shape[0], self.batchsize
        bpd2 = 0.
        for i in range((nums + bs - 1) // bs):
            bpx = px[bs * i: bs * i + bs]
            flatent, fmean, flogscale, logv = self.fine.forward(bpx, logv)
            logP, _ = self.fine.log_likelihood(flatent, fmean, flogscale)
            bpd2 += torch.mean(-logP, dim=0).item() / math.log(2) * bpx.shape[0]
            flatents.append(flatent[0])
            fmeans.append(fmean[0])
            flogscales.append(flogscale[0])
        bpd2 /= nums
        bpd = ((bpd1 * self.rough.H * self.rough.W + bpd2 * self.H * self.W)
               / (self.H - self.pad[0]) / (self.W - self.pad[1]))
        latents = [rlatent[0], torch.cat(flatents, dim=0)]
        means = [rmean[0], torch.cat(fmeans, dim=0)]
        logscales = [rlogscale[0], torch.cat(flogscales, dim=0)]
        return latents, means, logscales, bpd, bpd1, bpd2, logv

    def generated_from_noise(self, latents):
        """flows.py:247-270: latents = [rough [B, c, rh, rw], fine [B, c * patches, fh, fw]
        (or one row per patch)] -> images at the unpadded size."""
        from idfcodec.twolevel import merge_nchw
        rx = self.rough.generated_from_noise([latents[0]])
        zc = self.fine.latents_shape[0][0]
        flatents = latents[1].reshape(-1, zc, latents[1].shape[2], latents[1].shape[3])
        bs, nums = self.batchsize, flatents.shape[0]
        fx = [self.fine.generated_from_noise([flatents[i * bs: i * bs + bs]])
              for i in range((nums + bs - 1) // bs)]
        return merge_nchw(self._geometry(), rx, torch.cat(fx, dim=0))

    def inverse(self):
        self.fine.inverse()
        self.rough.inverse()

    # ------------------------------------------------------------ the codec
    def codec(self):
        from idfcodec.twolevel import TwoLevelCodec
        if self._tl_codec is None:
            self._tl_codec = TwoLevelCodec(self)
        return self._tl_codec

    def encode(self, x_u8, group=None):
        """uint8 images [B, C, H - pad[0], W - pad[1]] (device) -> idfcodec.TwoLevelBitstream;
        group: fine patches per rANS stream (default: one row of the patch grid)."""
        return self.codec().encode(x_u8, group=group)

    def decode(self, bitstream, verify=True):
        """TwoLevelBitstream -> (uint8 images, info) -- exact inverse of encode()."""
        return self.codec().decode(bitstream, verify=verify)


@NNFlows.register
class ConditionalFlows(IDFlows):
    """flows.py:277-361: priors see cat(x, cond) where cond is the VQ-VAE
    reconstruction squeezed (conv_for_cond False) or passed through stride-2
    convs (conv_for_cond True)."""

    def __init__(self, conv_for_cond=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        ch = self.C
        self.conv_for_cond = conv_for_cond
        if conv_for_cond:
            self.convs = nn.ModuleList()
        # the reference's IDFlows.__init__ popped 'name' from kwargs['prior'] in place
        prior_kw = {k: v for k, v in dict(kwargs.get("prior")).items() if k != "name"}
        for split_level in range(self.nsplit):
            block = self.blocks[split_level]
            scale = block["extend"].scale
            ch *= scale * scale
            prior = block["prior"]
            block["prior"] = self.prior_type(
                prior.out_channel,
                prior.cond_channel + ch if prior.cond_channel > 0 else prior.out_channel + ch,
                **deepcopy(prior_kw))
            if conv_for_cond:
                self.convs.append(nn.Conv2d(ch // scale // scale, ch, 4, 2, 1))

    def forward(self, x, logv, cond):
        require_device(x, "ConditionalFlows input")
        eng = self.engine()
        B = x.shape[0]
        ws = eng.load_nchw(x)
        eng.forward_pm(B, cond=cond.contiguous().float())
        lat = [t.clone() for t in eng.level_views(ws, B, "lat")]
        mean = [t.clone() for t in eng.level_views(ws, B, "mean")]
        logs = [t.clone() for t in eng.level_views(ws, B, "logscale")]
        return lat, mean, logs, logv

    def encode(self, x, cond, ways=1):
        return self.codec().encode(x, cond=cond.contiguous().float(), ways=ways)

    def decode(self, bitstream, cond, verify=True):
        return self.codec().decode(bitstream, cond=cond.contiguous().float(), verify=verify)
