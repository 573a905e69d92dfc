"""The x6 extractor with its two launch fusions (api_extract.hip run_extract): a block's downsample
conv folded into its conv3 (CWT_FUSE_DOWN) and the split-K combine of a conv1 done inside the next
conv's Winograd input transform (CWT_FUSE_SPLITK_WINO).  Both knobs are read per call, so one
process runs both arms.  Each arm is held to the oracle bar tests/test_gpu_parity.py applies to the
x6 extractor's features (1e-5 of max |f|); the fused-vs-unfused difference is printed, not bounded
(DESIGN.md §3 records it)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402

SEED = 2021
BAR_X6 = 1e-5   # tests/test_gpu_parity.py BAR[ARITH_X6]
KNOBS = ("CWT_FUSE_DOWN", "CWT_FUSE_SPLITK_WINO")


def rel(a, b):
    a = a.detach().double().cpu().numpy()
    b = b.detach().double().cpu().numpy()
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


class knobs:
    """Both fusions on ("1") or off ("0") for the duration; the environment is restored after."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        os.environ.update({k: self.value for k in KNOBS})

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def fresh_model():
    from few_shot_seg_cwt_amd import get_model
    m = get_model(syn.cfg_defaults(layers=50, dropout=0.0))
    m.load_state_dict(syn.make_pspnet_state(50, SEED))
    return m


_shared = {}


def shared_model():
    if "m" not in _shared:
        _shared["m"] = fresh_model()
    return _shared["m"]


def extract(m, x, value):
    with knobs(value):
        f, _ = m.extract_features(x)
        torch.cuda.synchronize()
    return f


@pytest.mark.parametrize("S", [33, 65])
def test_both_arms_meet_the_oracle_bar(dev, S):
    from oracle import cwt_oracle as O
    ep = syn.make_episode(SEED, 7, S, 2)
    x = torch.from_numpy(ep["spprt_imgs"][0])
    ref = O.extract_features(x, O.to_torch_state(syn.make_pspnet_state(50, SEED)))
    m = shared_model()
    f_on, f_off = extract(m, x.to(dev), "1"), extract(m, x.to(dev), "0")
    e_on, e_off = rel(f_on, ref), rel(f_off, ref)
    print(f"extract_features S={S}: fused {e_on:.3e}  unfused {e_off:.3e}  fused vs unfused {rel(f_on, f_off):.3e}")
    assert e_on < BAR_X6, e_on
    assert e_off < BAR_X6, e_off


def test_refold_after_train_bn_pass(dev):
    """A training-mode BN pass moves the running statistics, hence the eval folds the fused rows are
    built from: the next eval extraction (fusions on) must match the oracle run on the moved statistics
    (read back from the device), at the same bar."""
    from oracle import cwt_oracle as O
    m = fresh_model()
    ep = syn.make_episode(SEED, 11, 33, 2)
    m.train()
    with knobs("1"):
        m.extract_features(torch.from_numpy(ep["spprt_imgs"][0]).to(dev))
    m.eval()
    q = torch.from_numpy(ep["qry_img"])
    f = extract(m, q.to(dev), "1")
    moved = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    fresh = syn.make_pspnet_state(50, SEED)
    p = "layer1.0.downsample.1.running_mean"
    assert not np.array_equal(moved[p].numpy(), fresh[p])  # the pass did move them
    ref = O.extract_features(q, O.to_torch_state(moved))
    err = rel(f, ref)
    print(f"eval after train-BN pass, fused: {err:.3e}  unfused: {rel(extract(m, q.to(dev), '0'), ref):.3e}")
    assert err < BAR_X6, err
