"""The float64 reference of the fusion trainer's arithmetic (reference src/train_fuse.py:173-186,
FuseNet1 of src/model/transformer.py:286-330 over CenterPivotConv4d, src/model/conv4d.py:27-62) and
the fixtures its tests share -- a helper, not a test.  Plain torch on the CPU; nothing here runs device
code, so the kernels are never their own reference.

cp4d_strided        CenterPivotConv4d written from F.conv2d, any stride on the support plane (its
                    `prune_from` / `pad` arguments exist to build the WRONG variants the CPU tests separate)
cp4d_direct         the same layer as a loop over its definition
stack / stack_sided FuseNet1.conv4d on one correlation; the sided form leaves the ReLU units float64
                    cannot settle for fp32 open to the caller (match_ref.corr_forward_sided's rule)
fusenet1            FuseNet1.forward (the cat of 3 m^2 + 4 channels, att, softmax)
support_mask        train_fuse.py:173-175 / :319-321 (+ transformer.py:318-319's pool)
blend, fuse_loss    train_fuse.py:178, :180-186; fuse_counts :195-205
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from match_ref import TOL_FWD, TOL_GRAD, SEPARATION, rel, rand  # noqa: F401  (the project's bars, re-exported)

NEAR_CAP = 1e-3   # at most 0.1 % of a layer's units may lie inside the near-zero margin

CONV_NAMES = ("conv4d.0.conv1.weight", "conv4d.0.conv1.bias", "conv4d.0.conv2.weight", "conv4d.0.conv2.bias",
              "conv4d.2.conv1.weight", "conv4d.2.conv1.bias", "conv4d.2.conv2.weight", "conv4d.2.conv2.bias")
ATT_NAMES = ("att.0.weight", "att.0.bias", "att.2.weight", "att.2.bias")
PARAM_NAMES = CONV_NAMES + ATT_NAMES

# (hA, wA, hB, wB) -> the seed of its fixture: 20-90 % of layer 2's units alive (test_fuse_ref_cpu asserts it)
STACK_SHAPES = [(5, 7, 8, 8), (9, 4, 7, 7), (4, 5, 5, 5), (3, 3, 3, 3), (13, 17, 12, 12)]
# 24 * 24 * 36 = 20736 units: more than the 1024 * 16 positions one pass of the stack's backward grid covers, so
# its workgroups take their grid stride (no shape above does: 7956 units, 498 workgroups, one position per slot)
BIG_SHAPE = (24, 24, 12, 12)
STACK_SEEDS = {(5, 7, 8, 8): 5, (9, 4, 7, 7): 13, (4, 5, 5, 5): 3, (3, 3, 3, 3): 5, (13, 17, 12, 12): 13, BIG_SHAPE: 13}


# ---- the strided centre-pivot layer ----
def cp4d_strided(x, w1, b1, w2, b2, stride=1, prune_from=0, pad=1):
    """x [B, C, ha, wa, hb, wb] -> [B, O, ha, wa, ceil(hb/stride), ceil(wb/stride)]: conv1 (w1, b1) over
    (ha, wa) of the pruned tensor (support positions prune_from, prune_from + stride, ...; the reference
    prunes from 0), conv2 (w2, b2) over (hb, wb) with that stride and zero padding `pad` (the reference: 1)."""
    B, C, ha, wa, hb, wb = x.shape
    O = w1.shape[0]
    xp = x[..., prune_from::stride, prune_from::stride] if stride > 1 else x
    mb, nb = xp.shape[-2:]
    xa = xp.permute(0, 4, 5, 1, 2, 3).reshape(B * mb * nb, C, ha, wa)
    ya = F.conv2d(xa, w1, b1, padding=1).reshape(B, mb, nb, O, ha, wa).permute(0, 3, 4, 5, 1, 2)
    xb = x.permute(0, 2, 3, 1, 4, 5).reshape(B * ha * wa, C, hb, wb)
    if pad == 0:   # the WRONG variant: no leading zero, the taps read x[stride b' + db] (far side padded to keep the size)
        xb = F.pad(xb, (0, 2, 0, 2))
    yb = F.conv2d(xb, w2, b2, stride=stride, padding=pad)
    yb = yb.reshape(B, ha, wa, O, yb.shape[-2], yb.shape[-1]).permute(0, 3, 1, 2, 4, 5)
    return ya + yb


def cp4d_direct(x, w1, b1, w2, b2, stride):
    """The layer as a loop over its definition (kernel 3, padding 1):
    out[o][a][b'] = b1[o] + b2[o] + sum_{c,da} w1[o][c][da] x[c][a + da][stride b']
                                  + sum_{c,db} w2[o][c][db] x[c][a][stride b' + db]."""
    B, C, ha, wa, hb, wb = x.shape
    O = w1.shape[0]
    mb, nb = (hb + stride - 1) // stride, (wb + stride - 1) // stride
    out = torch.zeros(B, O, ha, wa, mb, nb, dtype=x.dtype)
    for ya in range(ha):
        for xa in range(wa):
            for yb in range(mb):
                for xb in range(nb):
                    acc = (b1 + b2).unsqueeze(0).repeat(B, 1)
                    for dy in range(3):
                        for dx in range(3):
                            qy, qx = ya + dy - 1, xa + dx - 1
                            if 0 <= qy < ha and 0 <= qx < wa:
                                acc = acc + x[:, :, qy, qx, stride * yb, stride * xb] @ w1[:, :, dy, dx].t()
                            sy, sx = stride * yb + dy - 1, stride * xb + dx - 1
                            if 0 <= sy < hb and 0 <= sx < wb:
                                acc = acc + x[:, :, ya, xa, sy, sx] @ w2[:, :, dy, dx].t()
                    out[:, :, ya, xa, yb, xb] = acc
    return out


# ---- the stack ----
def _relu_sided(pre, side, info):
    """pre * [pre > 0] with the units within TOL_FWD max|pre| of 0 taken from `side` (bool, pre's shape)
    when it is given; info receives (units inside the margin, units OUTSIDE it where side disagrees)."""
    on = pre.detach() > 0
    if side is not None:
        near = pre.detach().abs() < TOL_FWD * pre.detach().abs().max()
        if info is not None:
            info.append((int(near.sum()), int((on != side)[~near].sum()), pre.numel()))
        on = torch.where(near, side, on)
    return pre * on.to(pre.dtype)


def stack_sided(x, p, sides=None, info=None, prune_from=0, pad=1):
    """x [B, ha, wa, hb, wb], p the eight tensors of CONV_NAMES -> y2 [B, ha wa, mb nb].
    sides = (on1 [B, 16, ha, wa, mb, nb], on2 [B, 1, ha, wa, mb, nb]): the device's own ReLU outputs > 0."""
    B, ha, wa = x.shape[:3]
    pre1 = cp4d_strided(x.unsqueeze(1), p[0], p[1], p[2], p[3], stride=2, prune_from=prune_from, pad=pad)
    y1 = _relu_sided(pre1, sides[0] if sides is not None else None, info)
    pre2 = cp4d_strided(y1, p[4], p[5], p[6], p[7], stride=1)
    y2 = _relu_sided(pre2, sides[1] if sides is not None else None, info)
    return y2.reshape(B, ha * wa, -1)


def stack(x, p, **kw):
    return stack_sided(x, p, None, None, **kw)


def stack_pre(x, p):
    """(pre1, pre2): the two layers' pre-activations"""
    pre1 = cp4d_strided(x.unsqueeze(1), p[0], p[1], p[2], p[3], stride=2)
    return pre1, cp4d_strided(torch.relu(pre1), p[4], p[5], p[6], p[7], stride=1)


def device_sides(y1, X_cols, shape):
    """The device's ReLU gates in the reference's layout: y1 [B, NA, NB2, 16] (cwt_fuse_stack's saved
    buffer) and its y2 columns [B NA, NB2] -> (on1 [B, 16, ha, wa, mb, nb], on2 [B, 1, ha, wa, mb, nb])"""
    B, ha, wa, mb, nb = shape
    on1 = (y1.cpu() > 0).reshape(B, ha, wa, mb, nb, 16).permute(0, 5, 1, 2, 3, 4)
    on2 = (X_cols.cpu() > 0).reshape(B, 1, ha, wa, mb, nb)
    return on1, on2


# ---- FuseNet1 ----
def fusenet1(corr_lst, s_mask, pd_lst, sd, sides=None, att_side=None, info=None, swap_mask_pd=False, hidden_out=None):
    """FuseNet1.forward in float64: corr_lst two [1, h, w, hs, ws], s_mask [1, 1, m, m] (or [2m, 2m]),
    pd_lst two [1, 2, h, w], sd name -> parameter.  sides: per correlation, stack_sided's sides;
    att_side: the hidden ReLU's gates [h w, mid].  swap_mask_pd builds the WRONG variant that reads the
    mask's and the predictions' weight columns in exchanged places."""
    B, h, w = corr_lst[0].shape[:3]
    p = [sd[n] for n in CONV_NAMES]
    att_in = []
    for i, c in enumerate(corr_lst):
        y2 = stack_sided(c, p, sides[i] if sides is not None else None, info)      # [B, hw, m^2]
        att_in.append(y2.reshape(B, h, w, -1).permute(0, 3, 1, 2))
    m2 = att_in[0].shape[1]
    if s_mask.shape[-1] ** 2 == 4 * m2:
        s_mask = F.avg_pool2d(s_mask, 2, 2)
    att_in.append(s_mask.reshape(B, m2, 1, 1).expand(-1, -1, h, w))
    att_in += list(pd_lst)
    x = torch.cat(att_in, 1)                                                        # [B, 3 m^2 + 4, h, w]
    W = sd["att.0.weight"].reshape(sd["att.0.weight"].shape[0], -1)
    if swap_mask_pd:   # the last 4 columns and the first 4 of the mask's block exchanged
        W = torch.cat([W[:, :2 * m2], W[:, 3 * m2:], W[:, 2 * m2 + 4:3 * m2], W[:, 2 * m2:2 * m2 + 4]], 1)
    tok = x.permute(0, 2, 3, 1).reshape(B * h * w, -1)
    pre = tok @ W.t() + sd["att.0.bias"]
    if hidden_out is not None:
        hidden_out.append(pre.detach())
    hid = _relu_sided(pre, att_side, info)
    z = hid @ sd["att.2.weight"].reshape(2, -1).t() + sd["att.2.bias"]
    return torch.softmax(z, 1).reshape(B, h, w, 2).permute(0, 3, 1, 2)


def support_mask(label, m, align_corners, pool=False):
    """label [H, W] int64 -> [1, 1, m, m] float64 (train_fuse.py:173-175, :319-321); pool: resized to
    [2m, 2m], then FuseNet1's AvgPool2d(2, 2) (the resize passed through fp32, as the reference holds it)"""
    s = label.clone()
    s[s == 255] = 0
    size = (2 * m, 2 * m) if pool else (m, m)
    r = F.interpolate(s[None, None].double(), size, mode="bilinear", align_corners=align_corners)
    return F.avg_pool2d(r.float().double(), 2, 2) if pool else r


def blend(wv, fq, wt):
    return wv * wt[:, 0:1] + fq * wt[:, 1:2]


def _up(pd, S):
    return F.interpolate(pd, size=(S, S), mode="bilinear", align_corners=True)


def fuse_loss(pd_q, pd_q0, pd_q1, label, count_ignored=True):
    """train_fuse.py:180-186: label [1, S, S].  count_ignored False builds the WRONG variant that leaves
    the ignored pixels out of sum(wt_mask)."""
    S = label.shape[-1]
    pred_q, pred_q0, pred_q1 = _up(pd_q, S), _up(pd_q0, S), _up(pd_q1, S)
    wt_mask = ((pred_q0.argmax(1) != pred_q1.argmax(1)) & (label != 255)).to(pd_q.dtype)
    wt_mask[wt_mask == 0.0] = 0.001
    ce = F.cross_entropy(pred_q, label, ignore_index=255, reduction="none")
    den = wt_mask.sum() if count_ignored else wt_mask[label != 255].sum()
    return (ce * wt_mask).sum() / den


def fuse_counts(pd_q, pd_q0, pd_q1, label):
    """-> (iut [3, 3, 2] = {intersection, union, target} x class of pred_q, pred_q0, pred_q1
    (intersectionAndUnionGPU, util.py:280-308, ignore 255), the disagreeing labelled pixels)"""
    S = label.shape[-1]
    out = torch.zeros(3, 3, 2, dtype=torch.float64)
    preds = [_up(p, S).argmax(1) for p in (pd_q, pd_q0, pd_q1)]
    ok = label != 255
    for i, pr in enumerate(preds):
        for k in range(2):
            inter = ((pr == k) & (label == k)).sum()
            o, t = ((pr == k) & ok).sum(), (label == k).sum()
            out[i, 0, k], out[i, 1, k], out[i, 2, k] = inter, o + t - inter, t
    return out, int(((preds[1] != preds[2]) & ok).sum())


# ---- fixtures ----
def _uniform(shape, g, bound):
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().double()


def stack_params(seed):
    """The eight conv parameters at nn.Conv2d's default bounds (1/3 for layer 1, 1/12 for layer 2),
    through float32: the values the device holds"""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for cout, cin in ((16, 1), (1, 16)):
        bound = (9 * cin) ** -0.5
        for _ in range(2):
            out += [_uniform((cout, cin, 3, 3), g, bound), _uniform((cout,), g, bound)]
    return out


def stack_case(shape, seed=None):
    """(x [1, hA, wA, hB, wB] in [0, 1), params, the gradient at y2 [hA wA, mB nB] in [-1, 1))"""
    hA, wA, hB, wB = shape
    seed = STACK_SEEDS[shape] if seed is None else seed
    x = rand((1, hA, wA, hB, wB), seed).float().double()
    G = rand((hA * wA, ((hB + 1) // 2) * ((wB + 1) // 2)), seed + 50, -1, 1).float().double()
    return x, stack_params(seed), G


def stack_case_b2(shape):
    """stack_case with a batch of two different correlations: (x [2, ...], params, G [2 hA wA, mB nB])"""
    x0, p, G0 = stack_case(shape)
    x1, _, G1 = stack_case(shape, STACK_SEEDS[shape] + 100)
    return torch.cat([x0, x1], 0), p, torch.cat([G0, G1], 0)


def att_params(m, mid, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    K = 3 * m * m + 4
    return {"att.0.weight": _uniform((mid, K, 1, 1), g, K ** -0.5), "att.0.bias": _uniform((mid,), g, K ** -0.5),
            "att.2.weight": _uniform((2, mid, 1, 1), g, mid ** -0.5), "att.2.bias": _uniform((2,), g, mid ** -0.5)}


def label_case(S, seed, ignore=True):
    """[S, S] int64 in {0, 1} with a band of 255s when asked for"""
    g = torch.Generator().manual_seed(3000 + seed)
    lbl = (torch.rand(S, S, generator=g) < 0.4).long()
    if ignore:
        lbl[S // 3: S // 3 + 3, : S // 2] = 255
    return lbl


def head_case(shape, mid, seed=None):
    """A FuseNet1 case on a stack shape (m = ceil(hB/2); hB == wB): corr_lst, s_mask, pd_lst, sd and
    the gradient at wt"""
    hA, wA, hB, wB = shape
    seed = STACK_SEEDS[shape] if seed is None else seed
    m = (hB + 1) // 2
    x, p, _ = stack_case(shape, seed)
    xh = rand((1, hA, wA, hB, wB), seed + 7).float().double()
    sd = dict(zip(CONV_NAMES, p))
    sd.update(att_params(m, mid, seed))
    s_mask = support_mask(label_case(4 * m + 1, seed), m, True).float().double()
    pd = [rand((1, 2, hA, wA), seed + 11 + i, -2, 2).float().double() for i in range(2)]
    G = rand((1, 2, hA, wA), seed + 20, -1, 1).float().double()
    return dict(corr=[x, xh], s_mask=s_mask, pd=pd, sd=sd, G=G, m=m)


def loss_case(h, S, kind, seed=0):
    """pd_q, pd_q0, pd_q1 [1, 2, h, h] and label [1, S, S].  kind: 'mixed' (255 band, disagreements),
    'ignored' (every pixel 255), 'agree' (pd_q1 = pd_q0: every m_i is 0.001), 'edge' (everything 255
    but the last row, the last column and so the corner)"""
    pd = [rand((1, 2, h, h), 4000 + seed + i, -2, 2).float().double() for i in range(3)]
    lbl = label_case(S, seed, ignore=(kind == "mixed"))
    if kind == "ignored":
        lbl[:] = 255
    elif kind == "agree":
        pd[2] = pd[1].clone()
    elif kind == "edge":
        keep = lbl.clone()
        lbl[:] = 255
        lbl[-1, :], lbl[:, -1] = keep[-1, :], keep[:, -1]
    return pd[0], pd[1], pd[2], lbl[None]
