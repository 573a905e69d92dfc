"""What ran is what the plan says: the profile records of a real extractor pass equal the lines
cwt_debug_extract_plan prints for the same arguments (csrc/extract_plan.h; run_extract executes the
plan the export prints), at every profile level, in every conv family and in the training-mode BN pass."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import _lib  # noqa: E402
from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402

SEED = 2021
X3S, F32, X6 = 0, 1, 2   # CWT_CONV_ARITH_*
# mode -> conv_dtype, conv arithmetic of the context, training-mode BN
MODES = {"x6": ("fp32", X6, False), "x3s": ("fp32", X3S, False), "b16": ("bf16", X6, False),
         "f32d": ("fp32", F32, False), "train_bn": ("fp32", X6, True)}


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from few_shot_seg_cwt_amd import get_model
    m = get_model(syn.cfg_defaults(layers=50, dropout=0.0))
    m.load_state_dict(syn.make_pspnet_state(50, SEED))
    return m


def planned(N, S, dtype, arith, train):
    buf = C.create_string_buffer(1 << 18)
    _lib.check(_lib.lib().cwt_debug_extract_plan(50, N, S, int(dtype == "bf16"), arith, int(train), 0, buf, len(buf)),
               "cwt_debug_extract_plan")
    rows = [ln.split("\t") for ln in buf.value.decode().splitlines()]
    return [(int(r[0]), r[1], float(r[2]), float(r[3])) for r in rows if r[0] not in ("ws", "form")]


@pytest.mark.parametrize("S", [33, 65])
@pytest.mark.parametrize("mode", list(MODES))
def test_records_of_a_pass_equal_the_plan(model, mode, S):
    dtype, arith, train = MODES[mode]
    N = 2
    x = torch.from_numpy(syn.make_episode(SEED, 3, S, N)["spprt_imgs"][0]).cuda()
    assert x.shape == (N, 3, S, S)
    plan = planned(N, S, dtype, arith, train)
    assert {lv for lv, *_ in plan} == ({1, 2, 3} if mode == "x6" else {1, 2})   # only x6 has the Winograd form
    ctx = _lib.ctx(0)
    _lib.check(_lib.lib().cwt_ctx_set_conv_arith(ctx, arith), "cwt_ctx_set_conv_arith")
    model.set_conv_dtype(dtype)
    model.train(train)
    try:
        for level in (3, 2, 1):
            _lib.profile_enable(level)
            model.extract_features(x)
            torch.cuda.synchronize()
            ran = [r[:3] for r in _lib.profile_records()]
            assert ran == [r[1:] for r in plan if r[0] <= level], (mode, S, level)
    finally:
        _lib.profile_enable(0)
        model.train(False)
        model.set_conv_dtype("fp32")
        _lib.check(_lib.lib().cwt_ctx_set_conv_arith(ctx, X6), "cwt_ctx_set_conv_arith")
