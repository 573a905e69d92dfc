"""incremental.incremental_episode from random features (h = 5, S = 33, N = 17, no Trans): its
relabelled support, its adapted W and its IoU table equal the composition of the float64 pieces
(tests/nway_pixel_ref.py, tests/adapt_nway_ref.py)."""
import numpy as np
import pytest
import torch

import adapt_nway_ref as R
import nway_pixel_ref as P

pytestmark = pytest.mark.gpu


def test_incremental_episode_is_the_composition():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from few_shot_seg_cwt_amd.incremental import incremental_episode
    dev = torch.device("cuda", 0)
    h, S, ntr, n = 5, 33, 16, 2
    idx = ntr
    rng = np.random.default_rng(33)
    f_s = torch.from_numpy(rng.standard_normal((n, R.C, h, h)).astype(np.float32))
    f_q = torch.from_numpy(rng.standard_normal((1, R.C, h, h)).astype(np.float32))
    W_base = torch.from_numpy((0.3 * rng.standard_normal((ntr, R.C))).astype(np.float32))
    s_label = torch.from_numpy(rng.choice([0, 1, 255], size=(n, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64))
    q_label = torch.from_numpy(rng.choice([0, 1, 255], size=(1, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64))
    args = dict(cls_lr=0.1, adapt_iter=20, tp=1.1)
    torch.manual_seed(5)
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    r = incremental_episode(args, cl(f_s), s_label.to(dev), cl(f_q), q_label.to(dev), W_base.to(dev), idx)
    torch.cuda.synchronize()
    # the composition, in float64: the same fresh row (host RNG), then the pieces
    torch.manual_seed(5)
    std = 1.0 / np.sqrt(R.C)
    W0 = torch.cat([W_base, torch.empty(R.C).uniform_(-std, std)[None]])
    hi_s = P.upsample(torch.einsum("kc,nchw->nkhw", W0.double(), f_s.double()), S)
    hi_s[:, idx] = -1000.0
    assert P.gap_of(hi_s)[0] > P.GAP
    new_label = P.reset_spt_label_literal(s_label, hi_s, idx)
    assert torch.equal(r["s_label"].cpu(), new_label)
    W_ref = R.adapt_nway_loop(f_s, new_label, W0, 0.1, 20, idx, 1.1)
    e32 = R.err(R.inner_adapt_nway_ref(f_s, new_label, W0, 0.1, 20, idx, 1.1, dtype=torch.float32), W_ref, W0)
    e = R.err(r["W"].cpu(), W_ref, W0)
    print(f"err {e:.3g} e32 {e32:.3g}")
    assert e <= max(4 * e32, R.FLOOR)
    # the IoU table of the DEVICE's W (a table of W_ref's could differ by a pixel on a near-tie)
    hi_q = P.upsample(torch.einsum("kc,nchw->nkhw", r["W"].cpu().double(), f_q.double()), S)
    assert P.gap_of(hi_q)[0] > P.GAP
    iut, ce = P.metrics_ref(hi_q, q_label, idx)
    assert torch.equal(r["iut0"].cpu().double(), iut)
    assert float((r["ce0"].cpu()[0, 0] - ce[0, 0]).abs() / ce[0, 0]) <= 1e-5   # pred_q0 itself is an fp32 GEMM


def _near_tie_slack(hi_ref, diff):
    """Hi-res pixels whose top-two gap in the reference is within 2 x diff: the only pixels where
    logits that differ by at most diff can give another argmax."""
    top = hi_ref.topk(2, 1).values
    return int(((top[:, 0] - top[:, 1]) <= 2 * diff).sum())


def _mmn_inputs(dev):
    """The MMN head of test_gpu_match.test_mmn_forward (rmid l34, agg cat, wa True), 2 shots, h = 8."""
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    args = dict(rmid="l34", layers=50, all_lr="l", temp=20.0, att_wt=0.2, conv4d="red")
    net = MMN(args, agg="cat", wa=True, red_dim=False, device=dev)
    init_match_params(net, seed=5)
    net.eval()
    g = torch.Generator().manual_seed(29)
    h, n = 8, 2
    t = {k: torch.rand(*shape, generator=g) for k, shape in dict(
        q3=(1, 1024, h, h), q4=(1, 2048, h, h), s3=(n, 1024, h, h), s4=(n, 2048, h, h), f_q=(1, R.C, h, h),
        f_s=(n, R.C, h, h)).items()}
    return net, t, h, n


def test_trans_path_is_the_reference_composition():
    """With the MMN head: pred_q1 = W . att_fq and pred_q = W . (f_q (1 - att_wt) + att_fq att_wt)
    (train_cca.py:331-345), att_fq from the float64 oracle of the head, W the device's; the loss is
    the NLL of pred_q1.  Counts may differ from the float64 ones only by pixels whose top-two gap
    is within twice the logits' own difference."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from few_shot_seg_cwt_amd.incremental import incremental_episode
    from oracle import match_oracle as M
    dev = torch.device("cuda", 0)
    net, t, h, n = _mmn_inputs(dev)
    S, ntr = 8 * (h - 1) + 1, 16
    rng = np.random.default_rng(41)
    W_base = torch.from_numpy((0.3 * rng.standard_normal((ntr, R.C))).astype(np.float32))
    s_label = torch.from_numpy(rng.choice([0, 1, 255], size=(n, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64))
    q_label = torch.from_numpy(rng.choice([0, 1, 255], size=(1, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64))
    cl = lambda x: x.to(dev).contiguous(memory_format=torch.channels_last)
    fq_lst = {3: [t["q3"].to(dev)], 4: [t["q4"].to(dev)]}
    fs_lst = {3: [t["s3"].to(dev)], 4: [t["s4"].to(dev)]}
    torch.manual_seed(9)
    r = incremental_episode(dict(cls_lr=0.1, adapt_iter=5, tp=1.0), cl(t["f_s"]), s_label.to(dev), cl(t["f_q"]),
                            q_label.to(dev), W_base.to(dev), ntr, net, fs_lst, fq_lst)
    torch.cuda.synchronize()
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    wa = {b: M.wa_params_from_state(sd, f"wa_{b}.") for b in (3, 4)}
    layers = M.layers_from_state(sd, prefix="corr_net.NeighConsensus.conv.")
    d = lambda x: x.double().cpu()
    fqo, atto = M.mmn_forward({3: d(t["q3"]), 4: d(t["q4"])}, {3: d(t["s3"]), 4: d(t["s4"])}, d(t["f_q"]),
                              d(t["f_s"]), [3, 4], wa, layers, 20.0, 0.2)
    assert float((fqo - (0.8 * d(t["f_q"]) + 0.2 * atto)).abs().max()) < 1e-12   # the blend, att_wt = 0.2
    W = r["W"].cpu().double()
    for key, feat in (("1", atto), ("", fqo)):
        lo = torch.einsum("kc,nchw->nkhw", W, feat)
        got = r["pred_q" + key].cpu().double()
        diff = float((got - lo).abs().max())
        print(f"pred_q{key}: max abs diff {diff:.3g} of {float(lo.abs().max()):.3g}")
        assert diff <= 1e-4 * float(lo.abs().max())   # the head's own bar is 2e-5 of its output
        hi = P.upsample(lo, S)
        iut, ce = P.metrics_ref(hi, q_label, ntr)
        slack = _near_tie_slack(hi, diff)
        assert float((r["iut" + key].cpu().double() - iut).abs().max()) <= slack, slack
        assert abs(float(r["ce" + key].cpu()[0, 0] - ce[0, 0])) <= 1e-4 * float(ce[0, 0])
        assert torch.equal(r["ce" + key].cpu()[:, 1], ce[:, 1])
    blend = 0.8 * r["pred_q0"] + 0.2 * r["pred_q1"]
    assert float((r["pred_q"] - blend).abs().max()) <= 1e-5 * float(blend.abs().max())


class _StubModel:
    """extract_features as PSPNet's: (f [B,512,h,w], {layer: [features]}), from the image alone."""

    def __init__(self, h, dev):
        g = torch.Generator().manual_seed(3)
        self.h, self.proj = h, torch.randn(R.C, 3, generator=g).to(dev)
        self.p3, self.p4 = torch.randn(1024, 3, generator=g).to(dev), torch.randn(2048, 3, generator=g).to(dev)

    def eval(self):
        return self

    def extract_features(self, imgs):
        x = torch.nn.functional.adaptive_avg_pool2d(imgs, self.h)
        mk = lambda p: torch.einsum("kc,nchw->nkhw", p, x).contiguous(memory_format=torch.channels_last)
        return mk(self.proj), {3: [mk(self.p3).abs()], 4: [mk(self.p4).abs()]}


@pytest.mark.parametrize("with_trans", [False, True])
def test_validate_epoch_meters(with_trans):
    """validate_epoch over a stub loader (7 items a batch, as the reference's) and a stub model whose
    extract_features returns PSPNet's tuple: its class-wise meters and loss are those of the
    episodes' own iut / ce."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from few_shot_seg_cwt_amd.incremental import validate_epoch
    dev = torch.device("cuda", 0)
    net = _mmn_inputs(dev)[0] if with_trans else None
    h, n, ntr = 5, 2, 16
    S = 8 * (h - 1) + 1
    g = torch.Generator().manual_seed(77)
    lab = lambda *shape: torch.tensor([0, 1, 255])[torch.multinomial(torch.tensor([0.6, 0.3, 0.1]), int(np.prod(shape)),
                                                                     True, generator=g)].reshape(shape)
    loader = [(torch.rand(1, 3, S, S, generator=g), lab(1, S, S), torch.rand(1, n, 3, S, S, generator=g), lab(1, n, S, S),
               [torch.tensor(cls)], None, None) for cls in (3, 7, 3)]
    W_base = (0.3 * torch.randn(ntr, R.C, generator=g)).to(dev)
    eps = []
    res = validate_epoch(dict(cls_lr=0.1, adapt_iter=3, tp=1.0, num_classes_tr=ntr), loader, _StubModel(h, dev), W_base,
                         net, episodes_out=eps)
    assert len(eps) == 3
    for k in ("0", "1", "") if with_trans else ("0",):
        iut = [e["iut" + k].cpu().double()[0] for e in eps]
        want = {3: float((iut[0][0, 1] + iut[2][0, 1]) / (iut[0][1, 1] + iut[2][1, 1] + 1e-10)),
                7: float(iut[1][0, 1] / (iut[1][1, 1] + 1e-10))}
        assert res["class_iou" + k] == pytest.approx(want, rel=1e-12)
        assert res["mIoU" + k] == pytest.approx(np.mean(list(want.values())), rel=1e-12)
    ces = [e["ce1" if with_trans else "ce0"].cpu()[0] for e in eps]
    assert res["loss"] == pytest.approx(float(np.mean([float(c[0] / c[1]) for c in ces])), rel=1e-12)
    assert ("mIoU1" in res) == with_trans
