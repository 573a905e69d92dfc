"""CPU emulation of the bf16 conv stack (cwt_backbone_set_precision(CWT_CONV_BF16)) for the bars of
tests/test_gpu_bf16.py, on the oracle's block geometry and state keys.  What run_extract does
to a bf16 backbone: every conv but the stem's first reads bf16-rounded weights, every conv writes
its output rounded to bf16 -- after the fp32 BN fold, residual and ReLU in eval mode; in the
training-mode pass once raw, before the batch statistics, and again after BN, residual and ReLU
-- the max-pool is exact, and the head from layer4's output on is fp32 (the bottleneck conv reads
bf16 weights over its layer4 channels, fp32 ones over its PPM channels, and writes fp32).

The accumulation runs in `dtype` (torch.float32 or torch.float64).  Near-tie roundings flip
between two accumulation orders and spread through the layers, so an emulated chain is not a
tight oracle of the device; its distance from the exact float64 network is the yardstick."""
import torch
import torch.nn.functional as F

from oracle import cwt_oracle as O


def r16(t):
    """Round to bf16 (nearest even), kept in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def state64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in O.to_torch_state(sd).items()}


def exact_chain(x, sd64, layers, mom=None):
    """The oracle's backbone in float64 -> (layer2, layer3, layer4) outputs."""
    y = O.stem(x.double(), sd64, mom)
    outs = []
    for li, nblk in enumerate(O.RESNET_BLOCKS[layers], start=1):
        for b in range(nblk):
            y = O.bottleneck(y, sd64, li, b, mom)
        outs.append(y)
    return outs[1], outs[2], outs[3]


class _Chain:
    def __init__(self, sd, dtype, mom):
        self.sd, self.dtype, self.mom = sd, dtype, mom

    def conv_bn(self, x, wname, bn, stride=1, pad=0, dil=1, res=None, relu=True, w16=True):
        sd, dt = self.sd, self.dtype
        w = sd[wname].float()
        y = F.conv2d(x, (r16(w) if w16 else w).to(dt), None, stride, pad, dil)
        g, b = sd[bn + ".weight"].float(), sd[bn + ".bias"].float()
        if self.mom is None:  # the device's fp32 fold (load_conv)
            sc = g * (1.0 / torch.sqrt(sd[bn + ".running_var"].float() + O.BN_EPS))
            sh = b - sd[bn + ".running_mean"].float() * sc
            y = y * sc.to(dt)[None, :, None, None] + sh.to(dt)[None, :, None, None]
        else:  # raw conv output stored as bf16, then BN on its batch statistics (sd's running ones move)
            y = F.batch_norm(r16(y), sd[bn + ".running_mean"], sd[bn + ".running_var"], g.to(dt), b.to(dt), True,
                             self.mom, O.BN_EPS)
        if res is not None:
            y = y + res
        return r16(F.relu(y) if relu else y)

    def backbone(self, x, layers):
        c = self.conv_bn
        y = c(x.to(self.dtype), "layer0.0.weight", "layer0.1", 2, 1, w16=False)
        y = c(y, "layer0.3.weight", "layer0.4", 1, 1)
        y = c(y, "layer0.6.weight", "layer0.7", 1, 1)
        y = F.max_pool2d(y, 3, 2, 1)
        outs = []
        for li, nblk in enumerate(O.RESNET_BLOCKS[layers], start=1):
            for bi in range(nblk):
                p = f"layer{li}.{bi}"
                s, d, ds = O.block_geometry(li, bi)
                t = c(y, p + ".conv1.weight", p + ".bn1")
                t = c(t, p + ".conv2.weight", p + ".bn2", s, d, d)
                res = c(y, p + ".downsample.0.weight", p + ".downsample.1", ds, relu=False) if bi == 0 else y
                y = c(t, p + ".conv3.weight", p + ".bn3", res=res)
            outs.append(y)
        return outs[1], outs[2], outs[3]


def _running_to(sd, dtype):
    """A copy of the state whose running statistics are `dtype` tensors of their own (the
    training-mode chain moves them in place)."""
    out = dict(O.to_torch_state(sd))
    for k in out:
        if k.endswith(".running_mean") or k.endswith(".running_var"):
            out[k] = out[k].to(dtype).clone()
    return out


def bf16_chain(x, sd, layers, dtype):
    """Eval-mode bf16 backbone, accumulated in dtype -> (layer2, layer3, layer4) outputs."""
    with torch.no_grad():
        return _Chain(O.to_torch_state(sd), dtype, None).backbone(x, layers)


def head(l4, sd, dtype, mom=None, drop2d_scale=None):
    """The extractor from layer4's output on, as the bf16 backbone runs it: PPM and bottleneck in
    dtype with nothing rounded in between; the bottleneck weight's layer4 half (its first 2048
    input channels) is bf16, its PPM half fp32.  mom: training-mode BN (sd's statistics move)."""
    with torch.no_grad():
        sdt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if not k.startswith("layer")}
        for k in sdt:  # running statistics: the caller's own tensors, moved in place
            if k.endswith(".running_mean") or k.endswith(".running_var"):
                sdt[k] = sd[k] if sd[k].dtype == dtype else sd[k].to(dtype)
        w = sd["bottleneck.0.weight"].float().clone()
        w[:, :2048] = r16(w[:, :2048])
        sdt["bottleneck.0.weight"] = w.to(dtype)
        f = O.ppm(l4.to(dtype), sdt, mom=mom)
        f = F.relu(O._bn(O._conv(f, sdt, "bottleneck.0.weight", 1, 1), sdt, "bottleneck.1", mom))
        if drop2d_scale is not None:
            f = f * drop2d_scale[:, :, None, None].to(dtype)
        return f


def bf16_train(x, sd, layers, dtype, mom):
    """One training-mode extraction of the bf16 backbone (Dropout2d off), accumulated in dtype ->
    (features, the state with its running statistics moved)."""
    with torch.no_grad():
        sdm = _running_to(sd, dtype)
        l4 = _Chain(sdm, dtype, mom).backbone(x, layers)[2]
        return head(l4, sdm, dtype, mom), sdm
