"""MMN / MatchNet construction with every-bottleneck features (mmn.py:36-40: one correlation channel
per (layer, bottleneck) pair of the layers all_lr names), on the CPU: channel counts, the first
consensus layer's parameter shapes and the reference's state-dict key names.  No device needed: the
modules only hold parameters here."""
import pytest
import torch

CPU = torch.device("cpu")
NC_KEYS = [f"NeighConsensus.conv.{i}.{c}.{p}" for i in (0, 2, 4) for c in ("conv1", "conv2") for p in ("weight", "bias")]


def _mmn(agg="cat", **kw):
    from few_shot_seg_cwt_amd.match import MMN
    args = dict(rmid="l34", layers=50, all_lr="34", temp=20.0, att_wt=0.2, conv4d="red")
    args.update(kw)
    return MMN(args, agg=agg, wa=True, red_dim=False, device=CPU)


@pytest.mark.parametrize("kw,agg,want", [(dict(), "cat", 9), (dict(layers=101), "cat", 26),
                                         (dict(rmid="l234", all_lr="l"), "cat", 3), (dict(), "sum", 1),
                                         (dict(rmid="l234", all_lr="234"), "cat", 13),
                                         (dict(rmid="l234", all_lr="234", layers=101), "cat", 30),
                                         (dict(all_lr="4"), "cat", 4), (dict(all_lr="l"), "cat", 2)])
def test_match_channels(kw, agg, want):
    net = _mmn(agg, **kw)
    assert net.corr_net.in_channel == want
    assert net.corr_net.NeighConsensus.in_channel == want
    sd = net.state_dict()
    for c in ("conv1", "conv2"):
        assert tuple(sd[f"corr_net.NeighConsensus.conv.0.{c}.weight"].shape) == (10, want, 3, 3)
        assert tuple(sd[f"corr_net.NeighConsensus.conv.2.{c}.weight"].shape) == (10, 10, 3, 3)


def test_state_dict_keys_and_shared_modules():
    net = _mmn()
    sd = net.state_dict()
    assert tuple(sd["corr_net.NeighConsensus.conv.0.conv1.weight"].shape) == (10, 9, 3, 3)
    assert [k for k in sd if k.startswith("corr_net.")] == ["corr_net." + k for k in NC_KEYS]
    # one wa_ module per layer, shared by the layer's blocks (mmn.py:27-34)
    assert sorted({k.split(".")[0] for k in sd if not k.startswith("corr_net.")}) == ["wa_3", "wa_4"]


def test_channel_limits():
    from few_shot_seg_cwt_amd.match import MATCH_MAX_L, MatchNet
    assert MATCH_MAX_L == 32
    assert MatchNet(in_channel=32, device=CPU).in_channel == 32
    with pytest.raises(NotImplementedError):
        MatchNet(in_channel=33, device=CPU)
    with pytest.raises(NotImplementedError):
        MatchNet(in_channel=0, device=CPU)
    with pytest.raises(NotImplementedError):   # full Conv4d layers stay at one or two channels
        MatchNet(cv_type="cv4", in_channel=3, device=CPU)
    assert MatchNet(cv_type="cv4", in_channel=2, device=CPU).in_channel == 2


def test_header_declares_the_limit_and_the_entry():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "cwt.h")).read()
    assert "#define CWT_MATCH_MAX_L 32" in text
    assert "int cwt_extract_features_blocks(" in text
