"""PSPNet.extract_features with all_lr naming layers (get_feat_list, pspnet.py:272-287): every
bottleneck's output of a named layer, the last block's of the others (cwt_extract_features_blocks: one
XS_MID_COPY per requested block in the extractor's plan).  Synthetic R50 state at S = 65, N = 2 against
a float64 chain of the oracle's stem / bottleneck composed here block by block (bar 1e-4, as
tests/test_gpu_match.py test_extract_mid_features); the feature map and each layer's last entry must be
the bits of the plain / all_lr 'l' extractor -- the request changes no conv of the plan."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

S, N, SEED = 65, 2, 2021


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _img(dev, S_=S):
    from few_shot_seg_cwt_amd import synthetic as syn
    return torch.from_numpy(syn.normal(SEED, "blocks_img", (N, 3, S_, S_), 1.0)).to(dev)


def _extract(sd, x, **args):
    from few_shot_seg_cwt_amd import PSPNet
    net = PSPNet(dict(args))
    net.load_state_dict(sd)
    out = net.extract_features(x)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def r50(dev):
    """The state, the image, the plain and the all_lr 'l' extractions, and the float64 outputs of every
    block of layers 2-4 (computed once)."""
    from few_shot_seg_cwt_amd import synthetic as syn
    from oracle.cwt_oracle import RESNET_BLOCKS, bottleneck, stem, to_torch_state
    sd = syn.make_pspnet_state(50, SEED)
    x = _img(dev)
    f0, empty = _extract(sd, x, layers=50)
    assert empty == []
    _, last = _extract(sd, x, layers=50, rmid="l34", all_lr="l")
    sd64 = {k: v.double() for k, v in to_torch_state(sd).items()}
    y = stem(x.double().cpu(), sd64)
    ref = {}
    for li, nblk in enumerate(RESNET_BLOCKS[50], start=1):
        for b in range(nblk):
            y = bottleneck(y, sd64, li, b)
            if li >= 2:
                ref.setdefault(li, []).append(y)
    return dict(sd=sd, x=x, f0=f0, last=last, ref=ref)


def _check_bits(f, lst, f0, last):
    assert torch.equal(f, f0)
    for k in (2, 3, 4):
        assert len(last[k]) == 1 and torch.equal(lst[k][-1], last[k][0]), k


@pytest.mark.parametrize("all_lr,lengths", [("34", {2: 1, 3: 6, 4: 3}), ("234", {2: 4, 3: 6, 4: 3})])
def test_every_block_r50(dev, r50, all_lr, lengths):
    f, lst = _extract(r50["sd"], r50["x"], layers=50, rmid="l34", all_lr=all_lr)
    assert {k: len(v) for k, v in lst.items()} == lengths
    _check_bits(f, lst, r50["f0"], r50["last"])
    h = (S - 1) // 8 + 1
    errs = {}
    for k in (2, 3, 4):
        refs = r50["ref"][k][-lengths[k]:]   # every block, or the last one
        for b, (t, r) in enumerate(zip(lst[k], refs)):
            assert tuple(t.shape) == (N, {2: 512, 3: 1024, 4: 2048}[k], h, h)
            errs[f"l{k}.{b if lengths[k] > 1 else 'last'}"] = rel(t, r)
    print(f"all_lr={all_lr}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) < 1e-4, errs


def test_every_block_r101(dev):
    from few_shot_seg_cwt_amd import synthetic as syn
    sd = syn.make_pspnet_state(101, SEED)
    x = _img(dev, 33)
    f0, _ = _extract(sd, x, layers=101)
    _, last = _extract(sd, x, layers=101, rmid="l234", all_lr="l")
    f, lst = _extract(sd, x, layers=101, rmid="l234", all_lr="234")
    assert {k: len(v) for k, v in lst.items()} == {2: 4, 3: 23, 4: 3}
    _check_bits(f, lst, f0, last)


def test_every_block_bf16(dev, r50):
    sd, x = r50["sd"], r50["x"]
    f0, _ = _extract(sd, x, layers=50, conv_dtype="bf16")
    _, last = _extract(sd, x, layers=50, conv_dtype="bf16", rmid="l34", all_lr="l")
    f, lst = _extract(sd, x, layers=50, conv_dtype="bf16", rmid="l34", all_lr="34")
    assert {k: len(v) for k, v in lst.items()} == {2: 1, 3: 6, 4: 3}
    _check_bits(f, lst, f0, last)
    assert not torch.equal(lst[3][0], lst[3][-1])


def test_blocks_entry_rejects_bad_requests(dev, r50):
    """cwt_extract_features_blocks: a block past the layer's count, a layer outside 2..4 and a pair named
    twice are CWT_EARG; training-mode extraction with mid features keeps raising."""
    from few_shot_seg_cwt_amd import PSPNet, _lib
    net = PSPNet(dict(layers=50, rmid="l34", all_lr="34"))
    net.load_state_dict(r50["sd"])
    x = r50["x"]
    h = (S - 1) // 8 + 1
    feat = torch.empty(N, h, h, 512, device=dev)
    buf = torch.empty(N, h, h, 2048, device=dev)

    def call(layers, blocks):
        n = len(layers)
        return _lib.lib().cwt_extract_features_blocks(
            _lib.ctx(dev.index), net._handle, _lib.ptr(x), N, S, _lib.ptr(feat), n, (C.c_int * n)(*layers),
            (C.c_int * n)(*blocks), (C.c_void_p * n)(*[buf.data_ptr()] * n), _lib.stream_ptr(dev))

    assert call([3], [6]) == 1001 and call([4], [3]) == 1001 and call([2], [4]) == 1001
    assert call([1], [0]) == 1001 and call([5], [0]) == 1001 and call([3], [-1]) == 1001
    assert call([3, 3], [2, 2]) == 1001
    assert call([4], [2]) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf.permute(0, 3, 1, 2), r50["last"][4][0])
    net.train()
    with pytest.raises(NotImplementedError):
        net.extract_features(x)


def test_mid_entry_is_the_last_blocks_request(dev, r50):
    """cwt_extract_features_mid (unchanged signature) maps l2 / l3 / l4 onto the last blocks' bits of the
    per-block request: called directly, with every buffer and with l3 alone, it gives the bits of the
    all_lr 'l' extraction."""
    from few_shot_seg_cwt_amd import PSPNet, _lib
    net = PSPNet(dict(layers=50))
    net.load_state_dict(r50["sd"])
    x = r50["x"]
    h = (S - 1) // 8 + 1
    for want in ((2, 3, 4), (3,)):
        feat = torch.empty(N, h, h, 512, device=dev)
        bufs = {k: torch.full((N, h, h, c), float("nan"), device=dev) for k, c in ((2, 512), (3, 1024), (4, 2048))}
        ptr = lambda k: _lib.ptr(bufs[k]) if k in want else None  # noqa: E731
        _lib.check(_lib.lib().cwt_extract_features_mid(
            _lib.ctx(dev.index), net._handle, _lib.ptr(x), N, S, _lib.ptr(feat), ptr(2), ptr(3), ptr(4),
            _lib.stream_ptr(dev)), "cwt_extract_features_mid")
        torch.cuda.synchronize()
        assert torch.equal(feat.permute(0, 3, 1, 2), r50["f0"])
        for k in (2, 3, 4):
            if k in want:
                assert torch.equal(bufs[k].permute(0, 3, 1, 2), r50["last"][k][0]), k
            else:
                assert bool(torch.isnan(bufs[k]).all()), k


def test_detr_reads_the_last_block(dev, r50):
    """DeTr keeps one feature per layer, the last block: on the lists of an all_lr '34' extraction
    (six entries for layer3, three for layer4) it gives the bits it gives on the all_lr 'l' lists."""
    from few_shot_seg_cwt_amd.detr import DeTr
    from few_shot_seg_cwt_amd.match import init_match_params
    _, every = _extract(r50["sd"], r50["x"], layers=50, rmid="l34", all_lr="34")
    assert len(every[3]) == 6 and len(every[4]) == 3 and not torch.equal(every[3][0], every[3][-1])
    torch.manual_seed(1)
    net = DeTr(dict(rmid="l34", temp=20.0, att_wt=0.2), sf_att=True, cs_att=True, reduce_dim=512, device=dev)
    init_match_params(net.cross_trans, 22)
    f_q, f_s = r50["f0"][:1], r50["f0"][1:]
    outs = []
    with torch.no_grad():
        for lst in (every, r50["last"]):
            fq_lst = {k: [t[:1] for t in v] for k, v in lst.items()}
            fs_lst = {k: [t[1:] for t in v] for k, v in lst.items()}
            outs.append(net(fq_lst, fs_lst, f_q, f_s))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with torch.no_grad():   # the check can tell: the first blocks give another result
        first = net({k: [v[0][:1]] for k, v in every.items()}, {k: [v[0][1:]] for k, v in every.items()}, f_q, f_s)
    assert not torch.equal(first[0], outs[0][0])
    assert float(outs[0][0].abs().max()) > 0
